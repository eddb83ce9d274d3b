"""Grafting a tree onto a root state that is none of its vertices, without a device.

  * the numpy restatement (tests/graft_ref.py) on the oracle's trees and the
    six roots the GPU tests use: the counts are recorded here, and every case
    exercises what the feature is for (several attached vertices, a kept
    descendant that is not attached, dropped vertices, an attached vertex
    under an attached ancestor);
  * the restated connect action has the oracle's bits, the keep rule is the
    re-root's on the tree with one more vertex;
  * the oracle accepts the restated trees as warm starts, with the figures the
    GPU tests compare the device's continuation with;
  * the C ABI exports the entry points and refuses NULL handles and bad
    arguments before touching a device;
  * csrc/host/gbp_tree_prune.cpp's applyGraftRemap as a stand-alone program
    under AddressSanitizer and UBSan against the restatement.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from tests import graft_ref as G
from tests import prune_ref as R
from tests import reroot_ref as RR
from tests.helpers import bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "global_body_planner_amd", "csrc", "host")

# case -> (candidates, checked, attached, kept, outside, depth,
#          attached vertices with an attached ancestor)
FOUND = {
    "a-mid5-r3": (95, 77, 26, 52, 44, 4, 6),
    "a-mid5-r1": (40, 22, 12, 30, 66, 4, 1),
    "a-start-shift": (93, 79, 13, 70, 26, 6, 6),
    "b-mid5-r3": (70, 49, 14, 49, 26, 6, 2),
    "b-v30-shift": (74, 55, 10, 21, 54, 4, 0),
    "b-goal-shift": (62, 49, 0, 1, 74, 0, 0),
}


def attached_under_attached(parent, attach):
    out = 0
    for i in np.flatnonzero(attach):
        p = int(parent[i])
        while p >= 0 and not attach[p]:
            p = int(parent[p])
        out += p >= 0
    return out


# ---- the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("case", list(G.CASES))
def test_cases_exercise_the_graft(case):
    name, direction, radius = G.CASES[case]
    src = R.search("S")[name]
    assert len(src["parent"]) == (95 if name == "a" else 74)
    parent = np.asarray(src["parent"])
    tree, remap, st, (cand, checked, attach, actions) = G.expected(case)
    att = attach.astype(bool)
    nested = attached_under_attached(parent, att)
    assert (st["n_candidates"], st["n_checked"], st["n_attached"], st["n_kept"], st["n_outside"],
            st["depth"], nested) == FOUND[case]
    assert st["n_kept"] - 1 + st["n_outside"] + st["n_edge_invalid"] + st["n_inherited"] == len(parent)
    assert st["n_edge_invalid"] == st["n_inherited"] == 0        # no edge was tested
    assert not np.any(att & ~checked) and not np.any(checked & ~cand)
    if case == "b-goal-shift":     # the root-alone case
        assert st["n_kept"] == 1 and st["n_attached"] == 0 and np.all(remap < 0)
        assert tree["parent"].tolist() == [-1] and not np.any(tree["act"])
        return
    kept = remap >= 0
    assert st["n_attached"] >= 5
    # an attached vertex with a kept descendant that is not attached itself
    assert any(att[parent[i]] for i in np.flatnonzero(kept & ~att))
    assert np.any(~kept)
    if case == "b-v30-shift":
        # this root attaches no vertex below another attached one (0 found,
        # recorded above); b-mid5-r3 covers that shape on the REVERSE tree
        assert nested == 0
    else:
        assert nested >= 1
    # the tree as stated: the root first, the rest in ascending old index
    assert same_rows(tree["v"][0], G.case_root(case))
    order = np.flatnonzero(kept)
    assert np.array_equal(remap[order], 1 + np.arange(len(order)))
    assert np.array_equal(bits(tree["v"][1:]), bits(src["v"][order]))
    assert np.all(tree["parent"][1:][att[order]] == 0)
    assert np.array_equal(bits(tree["act"][1:][att[order]]), bits(actions[order][att[order]]))
    assert np.array_equal(bits(tree["act"][1:][~att[order]]), bits(src["act"][order][~att[order]]))


def same_rows(x, y):
    return np.array_equal(bits(np.asarray(x)), bits(np.asarray(y)))


def test_roots_are_off_the_trees_and_valid():
    _, O = R.terrain(None)
    for case, (name, direction, _) in G.CASES.items():
        root = G.case_root(case)
        v = R.search("S")[name]["v"]
        assert not any(same_rows(root, row) for row in v), case
        stance = O.valid_states(root[None], 1)[0][0]
        flight = O.valid_states(root[None], 0)[0][0]
        assert stance or (name == "b" and flight), (case, stance, flight)


def test_connect_action_restated_has_the_oracles_bits():
    _, O = R.terrain(None)
    for case in ("a-mid5-r3", "b-mid5-r3"):
        name, direction, _ = G.CASES[case]
        root, v = G.case_root(case), R.search("S")[name]["v"]
        _, _, _, (cand, checked, attach, actions) = G.expected(case)
        for j in np.flatnonzero(attach):
            t_s = oracle.pose_distance(v[j], root) / G.V_NOM
            ends = (root, v[j]) if direction == G.FORWARD else (v[j], root)
            assert same_rows(G.connect_action(*ends, t_s), actions[j]), (case, j)


def test_keep_rule_is_the_reroot_at_one_more_vertex():
    """The graft's keep rule and depth on n vertices are reroot_ref's at vertex
    n of the tree of n + 1 vertices whose attached vertices hang under n."""
    rng = np.random.default_rng(20261101)
    tree = RR.random_recursive_tree(600, seed=20261102)
    n = 600
    attach = (rng.random(n) < 0.03).astype(np.uint8)
    ok = (rng.random(n) >= 0.1).astype(np.uint8)
    assert attach.sum() >= 5
    out, remap, st = G.graft(tree, np.zeros(8), attach, np.ones((n, 10)), ok)
    parent = np.r_[np.where(attach != 0, n, tree["parent"]), -1].astype(np.int32)
    aug = dict(v=np.r_[tree["v"], np.zeros((1, 8))], act=np.r_[tree["act"], np.zeros((1, 10))],
               parent=parent)
    ok2 = np.r_[np.where(attach != 0, 1, ok), 1].astype(np.uint8)
    rtree, rremap, rst = RR.reroot(aug, n, ok2)
    assert np.array_equal(rremap[:n], remap) and rremap[n] == 0
    assert np.array_equal(rtree["parent"], out["parent"])
    for key in ("n_kept", "n_outside", "n_edge_invalid", "n_inherited", "depth"):
        assert rst[key] == st[key], key
    assert 0 < st["n_edge_invalid"] and 0 < st["n_inherited"] and 1 < st["n_kept"] < n


def test_synthetic_decisions():
    tree = RR.random_recursive_tree()
    n = len(tree["parent"])
    root, acts = np.full(8, 0.25), np.ones((n, 10))
    out, remap, st = G.graft(tree, root, np.ones(n, np.uint8), acts)
    assert st["depth"] == 1 and st["n_kept"] == n + 1 and np.all(out["parent"][1:] == 0)
    out, remap, st = G.graft(tree, root, np.zeros(n, np.uint8), acts)
    assert st["n_kept"] == 1 and st["n_outside"] == n and st["depth"] == 0
    one = np.zeros(n, np.uint8)
    one[1] = 1
    assert G.graft(tree, root, one, acts)[2]["n_kept"] == 1 + 3280    # vertex 1 heads 3,280
    st = G.graft(RR.chain_against_the_index_order(4097), root,
                 (np.arange(4097) == 2048).astype(np.uint8), np.ones((4097, 10)))[2]
    assert st["n_kept"] == 1 + 2048 and st["depth"] == 2048


# ---- the oracle's warm start ------------------------------------------------------------
@pytest.mark.parametrize("side", ["a", "b"])
def test_oracle_accepts_the_restated_trees(side):
    ref = G.oracle_continues(side)
    print(side, len(ref["a"]["v"]), len(ref["b"]["v"]), ref["rewires"], ref["found"])
    assert ref["found"]
    assert (len(ref["a"]["v"]), len(ref["b"]["v"]), ref["rewires"]) == G.CONTINUED[side]
    # the grafted tree grew: the search went on from it
    assert len(ref[side]["v"]) > len(G.expected(f"{side}-mid5-r3")[0]["v"])


# ---- the C ABI ---------------------------------------------------------------------
NEW = ["gbp_tree_graft_check_dev", "gbp_tree_graft_dev", "gbp_tree_graft_host",
       "gbp_tree_graft_keep_host", "gbp_tree_graft_last"]


def test_abi_exports_and_null_handles():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (gbp_\w+)", out))
    assert set(NEW) <= exported and set(NEW) <= set(L.EXPORTS)
    txt = open(os.path.join(ROOT, "include", "gbp.h")).read()
    for name in NEW:
        assert f"int {name}(" in txt
    lib = L.load()
    st = L.GraftStats()
    assert ctypes.sizeof(st) == 72
    one = ctypes.c_int64(1)  # stands for any non-NULL array
    p = ctypes.byref(one)
    root = (ctypes.c_double * 8)()
    assert lib.gbp_tree_graft_check_dev(None, None, 1, root, 1.0, 0, 0, p, p, p, None) == -2
    assert lib.gbp_tree_graft_dev(None, 1, root, p, p, None, p, ctypes.byref(st), None) == -2
    k = ctypes.c_int64(7)
    assert lib.gbp_tree_graft_host(None, None, root, 1.0, 0, 0, 0, None, ctypes.byref(st),
                                   ctypes.byref(k)) == -2
    assert k.value == 0
    assert lib.gbp_tree_graft_last(None, None) == -1


# ---- the remap on the host copy ------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("graft")
    exe = str(d / "tree_graft_probe")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe,
                    os.path.join(HERE, "native", "tree_graft_probe.cpp"),
                    os.path.join(HOST, "gbp_tree_prune.cpp")], check=True)
    count = [0]

    def run(remap, parent, attach):
        """-> (kept, parents of the survivors, the old index of each survivor's
        rows, the old index its action names: 1000000 + i for a connect action)."""
        count[0] += 1
        path = str(d / f"in{count[0]}.txt")
        with open(path, "w") as f:
            f.write(f"{len(parent)}\n" + "\n".join(" ".join(str(int(x)) for x in row)
                                                   for row in (remap, parent, attach)) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        tok = [int(t) for t in r.stdout.split()]
        assert len(tok) == 1 + 3 * max(tok[0], 0)
        return tok[0], np.array(tok[1::3], np.int32), np.array(tok[2::3]), np.array(tok[3::3])
    return run


def test_remap_probe_equals_restatement(probe):
    s = R.search("S")
    for case in G.CASES:
        name = G.CASES[case][0]
        parent = s[name]["parent"]
        tree, remap, stats, (_, _, attach, _) = G.expected(case)
        kept, p, src, act = probe(remap, parent, attach)
        assert kept == stats["n_kept"], case
        assert np.array_equal(p, tree["parent"]), case
        order = np.flatnonzero(remap >= 0)
        assert np.array_equal(src, np.r_[-1, order]), case
        assert np.array_equal(act, np.r_[-1, np.where(attach[order] != 0, 1000000 + order, order)])
    big = RR.random_recursive_tree()   # every vertex attached: the rows move up by one
    n = len(big["parent"])
    kept, p, src, act = probe(1 + np.arange(n), big["parent"], np.ones(n, int))
    assert kept == n + 1 and np.all(p[1:] == 0) and np.array_equal(src[1:], np.arange(n))


def test_remap_probe_refuses_what_is_no_graft(probe):
    parent = np.array([-1, 0, 1, 1, 0], np.int32)
    assert probe([-1, 1, 2, 3, -1], parent, [0, 1, 0, 0, 0])[0] == 4     # 1 and what hangs below it
    assert probe([-1, 1, 2, 3, 4], parent, [0, 1, 0, 0, 1])[0] == 5      # two attached
    assert probe([-1, -1, -1, -1, -1], parent, [0, 0, 0, 0, 0])[0] == 1  # the root alone
    assert probe([-1, 0, 1, 2, -1], parent, [0, 1, 0, 0, 0])[0] == -1    # numbered from 0
    assert probe([-1, 1, 2, 3, 4], parent, [0, 1, 0, 0, 0])[0] == -1     # 4 kept under a dropped parent
    assert probe([-1, 1, 3, 2, -1], parent, [0, 1, 0, 0, 0])[0] == -1    # not in ascending order
    assert probe([-1, -1, 1, 2, -1], parent, [0, 1, 0, 0, 0])[0] == -1   # an attached vertex dropped
    assert probe([1, -1, -1, -1, -1], parent, [0, 0, 0, 0, 0])[0] == -1  # the old root kept, not attached
