"""Re-rooting a tree at one of its vertices, without a device.

  * the numpy restatement (tests/reroot_ref.py) on the oracle's trees: at the
    root it returns the tree with the oracle's own g bits, below it g is not
    g - g[k], and the shapes the GPU tests rely on are there (a descendant with
    a smaller index than the new root, a map change that cuts the subtree);
  * the oracle accepts the restated trees as warm starts, with the figures the
    GPU tests compare the device's continuation with;
  * the C ABI exports the two entry points and refuses NULL handles;
  * csrc/host/gbp_tree_prune.cpp (a re-root's remap applied to the host copy
    of a tree) and the start-tree path helpers of csrc/host/gbp_tree_path.cpp
    as a stand-alone program under AddressSanitizer and UBSan.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from tests import prune_ref as R
from tests import reroot_ref as RR
from tests.helpers import bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "global_body_planner_amd", "csrc", "host")


# ---- the restatement -----------------------------------------------------------------
@pytest.mark.parametrize("which", ["S", "C"])
def test_restatement_at_the_root_is_the_oracles_tree(which):
    for name in "ab":
        tree = R.search(which)[name]
        n = len(tree["parent"])
        out, remap, stats = RR.reroot(tree, 0)
        assert np.array_equal(remap, np.arange(n))
        assert stats["n_kept"] == n and stats["n_outside"] == 0
        assert np.array_equal(out["parent"], tree["parent"])
        for k in ("v", "act", "g"):   # g: derived again, the oracle's own bits
            assert np.array_equal(bits(out[k]), bits(tree[k])), (which, name, k)


def test_g_is_derived_not_subtracted():
    """S a below vertex 1: g - g[1] differs from the derivation in the bits of
    35 of the 62 vertices."""
    tree = R.search("S")["a"]
    out, remap, stats = RR.reroot(tree, 1)
    assert stats["n_kept"] == 62 and stats["n_outside"] == 33
    order = np.argsort(np.where(remap >= 0, remap, len(remap)), kind="stable")[:62]
    assert order[0] == 1 and np.array_equal(order[1:], np.sort(order[1:]))
    sub = tree["g"][order] - tree["g"][1]
    assert int(np.sum(bits(sub) != bits(out["g"]))) == 35
    assert np.allclose(sub, out["g"], rtol=0, atol=1e-12)


def test_shapes_the_gpu_tests_rely_on():
    s = R.search("S")
    for name, k in (("a", 36), ("b", 57)):   # a descendant with a smaller index
        out, remap, _ = RR.reroot(s[name], k)
        assert np.flatnonzero(remap >= 0).min() < k
    c = R.search("C")["a"]
    for k in (1, 3):   # RRT-Connect: parents before children, before and after
        p = RR.reroot(c, k)[0]["parent"]
        assert np.all(p[1:] < np.arange(1, len(p)))
    # the best path's chain in S a
    chain, i = [], 66
    while i >= 0:
        chain.append(i)
        i = int(s["a"]["parent"][i])
    assert chain[::-1] == [0, 1, 5, 36, 39, 71, 66]
    # box 1: the subtree of 1 is cut to 4 of 62, that of 36 stands, 5 is alone
    for k, kept, under in ((1, 4, 62), (36, 35, 35), (5, 1, 55)):
        st = RR.expected("S", "a", k, "box1")[2]
        assert st["n_kept"] == kept and st["n_before"] - st["n_outside"] == under
        assert st["n_kept"] + st["n_outside"] + st["n_edge_invalid"] + st["n_inherited"] == 95
    # edge_valid[k] is ignored
    ok = R.edge_valid(R.terrain("box1")[1], s["a"], RR.FORWARD)
    ok2 = ok.copy()
    ok2[36] ^= 1
    assert np.array_equal(RR.reroot(s["a"], 36, ok)[1], RR.reroot(s["a"], 36, ok2)[1])


def test_synthetic_trees():
    big = RR.random_recursive_tree()
    assert RR.reroot(big, 1)[2]["n_kept"] == 3280 and RR.reroot(big, 0)[2]["depth"] == 18
    per, k = RR.permuted(big, 1, 20261021)
    out, remap, stats = RR.reroot(per, k)
    assert stats["n_kept"] == 3280 and np.any(out["parent"] > np.arange(3280))
    st = RR.reroot(RR.chain_against_the_index_order(4099), 4098)[2]
    assert st["depth"] == 4097 and st["n_kept"] == 4098


# ---- the oracle's warm start ------------------------------------------------------------
def _oracle_continues(which, k, star, halves, first):
    r = R.search(which)
    _, O = R.terrain(None)
    _, goal = R.start_goal()
    a = RR.expected(which, "a", k)[0]
    init = tuple({key: t[key] for key in ("v", "act", "parent")} for t in (a, r["b"]))
    cfg = R.SETS[which]
    streams = dict(stream_a=401, stream_b=402) if star else {}
    ref = O.plan(a["v"][0], goal, init_trees=init, star=star, nthreads=16, batch=cfg["batch"],
                 seed=cfg["seed"], max_halves=halves, first_half=first, extend_base=r["ext_counter"],
                 **streams)
    # the warm start derived g from the given tree: the restatement's
    n0 = len(a["parent"])
    if not ref.get("rewires"):
        assert np.array_equal(bits(ref["a"]["g"][:n0]), bits(a["g"]))
    return ref


def test_oracle_accepts_the_restated_trees():
    ref = _oracle_continues("S", 5, True, 100, 300)
    assert (len(ref["a"]["v"]), len(ref["b"]["v"])) == (93, 100)
    assert ref["rewires"] == 18 and ref["found"]
    ref = _oracle_continues("C", 3, False, 40, 200)
    assert (len(ref["a"]["v"]), len(ref["b"]["v"])) == (12, 23) and ref["found"]


# ---- the C ABI ---------------------------------------------------------------------
NEW = ["gbp_tree_reroot_dev", "gbp_tree_reroot_host"]


def test_abi_exports_and_null_handles():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (gbp_\w+)", out))
    assert set(NEW) <= exported and set(NEW) <= set(L.EXPORTS)
    txt = open(os.path.join(ROOT, "include", "gbp.h")).read()
    for name in NEW:
        assert f"int {name}(" in txt
    lib = L.load()
    st = L.RerootStats()
    assert ctypes.sizeof(st) == 48
    one = ctypes.c_int64(1)  # stands for any non-NULL array
    p = ctypes.byref(one)
    assert lib.gbp_tree_reroot_dev(None, 1, 0, None, p, ctypes.byref(st), None) == -2
    k = ctypes.c_int64(7)
    assert lib.gbp_tree_reroot_host(None, None, 0, 0, 0, None, ctypes.byref(st), ctypes.byref(k)) == -2
    assert k.value == 0


# ---- the remap on the host copy ------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("reroot")
    exe = str(d / "tree_reroot_probe")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe,
                    os.path.join(HERE, "native", "tree_reroot_probe.cpp"),
                    os.path.join(HOST, "gbp_tree_prune.cpp"), os.path.join(HOST, "gbp_tree_path.cpp"),
                    os.path.join(HOST, "gbp_planning_math.cpp")], check=True)
    count = [0]

    def run(remap, parent, new_root, meet=0):
        """-> (kept, parents of the survivors, the old index of each survivor's
        rows, the path root -> meet, what findStateAmong gave along it)."""
        count[0] += 1
        path = str(d / f"in{count[0]}.txt")
        with open(path, "w") as f:
            f.write(f"{len(parent)} {int(new_root)} {int(meet)}\n" +
                    " ".join(str(int(x)) for x in remap) + "\n" +
                    " ".join(str(int(x)) for x in parent) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        lines = r.stdout.split("\n")
        chain, found = ([int(t) for t in lines[k].split()] for k in (0, 1))
        tok = [int(t) for t in " ".join(lines[2:]).split()]
        assert len(tok) == 1 + 2 * max(tok[0], 0)
        return tok[0], np.array(tok[1::2], np.int32), np.array(tok[2::2], np.int64), chain, found
    return run


def test_remap_probe_equals_restatement(probe):
    s = R.search("S")
    for name, k in (("a", 0), ("a", 1), ("a", 36), ("b", 57), ("a", 66)):
        parent = s[name]["parent"]
        tree, remap, stats = RR.reroot(s[name], k)
        kept, p, src, _, _ = probe(remap, parent, k)
        assert kept == stats["n_kept"], (name, k)
        assert np.array_equal(p, tree["parent"])
        order = np.r_[k, [i for i in np.flatnonzero(remap >= 0) if i != k]]
        assert np.array_equal(src, order), (name, k)
    tree, remap, stats = RR.expected("S", "a", 1, "box1")   # with the map changed
    kept, p, src, _, _ = probe(remap, s["a"]["parent"], 1)
    assert kept == 4 and np.array_equal(p, tree["parent"])


def test_remap_probe_refuses_what_is_no_reroot(probe):
    parent = np.array([-1, 0, 1, 1, 0], np.int32)
    assert probe([-1, 0, 1, 2, -1], parent, 1)[0] == 3     # the subtree of 1: fine
    assert probe([-1, 0, 0, 1, -1], parent, 1)[0] == -1    # two vertices on 0
    assert probe([-1, 0, -1, 1, 2], parent, 1)[0] == -1    # a kept child of a dropped parent
    assert probe([-1, 1, 0, 2, -1], parent, 1)[0] == -1    # remap[new_root] != 0
    assert probe([-1, 0, 2, 1, -1], parent, 1)[0] == -1    # not in ascending order
    assert probe([-1, 0, 1, 2, -1], parent, 5)[0] == -1    # new_root outside the tree
    assert probe([-1, 0, 1, 2, -1], parent, -1)[0] == -1


def test_start_tree_path_helpers(probe):
    parent = R.search("S")["a"]["parent"]
    n = len(parent)
    _, _, _, chain, found = probe(np.arange(n), parent, 0, meet=66)
    assert chain == [0, 1, 5, 36, 39, 71, 66] and found == chain
    assert probe(np.arange(n), parent, 0, meet=0)[3] == [0]
    assert probe(np.arange(n), parent, 0, meet=n)[3] == []
    assert probe(np.arange(n), parent, 0, meet=-1)[3] == []
    # a parent array that never reaches the root
    assert probe([0, 1, 2], [-1, 2, 1], 0, meet=1)[3] == []
