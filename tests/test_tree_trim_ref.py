"""Trimming a tree by cost, without a device.

  * the numpy restatement (tests/trim_ref.py) pinned on the oracle's trees:
    the session test's search (seed 11, 200 halves) and set S of
    tests/prune_ref.py, the 6,017-vertex tree with 64-way ties at every budget
    the GPU test uses, and the shapes those tests rely on (a best connection
    whose own vertex fails the bound test by 1.3e-15, f that never falls from
    parent to child);
  * the C ABI exports the three entry points and refuses NULL handles;
  * csrc/host/gbp_tree_prune.cpp's applyTrimRemap (a trim's remap applied to a
    dumped tree, and the record a node logs) as a stand-alone program under
    AddressSanitizer and UBSan.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from tests import prune_ref as R
from tests import shared_ref as SR
from tests import trim_ref as TR
from tests.helpers import bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "global_body_planner_amd", "csrc", "host")


def over(tree, other_root, bound):
    return int((TR.f_values(tree, other_root)[1:] > bound).sum())


# ---- the two searches ----------------------------------------------------------------
def test_dead_weight_above_the_best_cost():
    """The share of each tree that no path through it can use with the current g."""
    r = TR.session_search()
    assert (len(r["a"]["parent"]), len(r["b"]["parent"])) == (61, 71)
    assert (r["best_a"], r["best_b"]) == (24, 25) and r["best_cost"] == 3.981266911844149
    assert over(r["a"], r["b"]["v"][0], r["best_cost"]) == 25
    assert over(r["b"], r["a"]["v"][0], r["best_cost"]) == 31
    s = R.search("S")
    assert (len(s["a"]["parent"]), len(s["b"]["parent"])) == (95, 74)
    assert (s["best_a"], s["best_b"]) == (66, 38) and s["best_cost"] == 3.286201250674083
    assert over(s["a"], s["b"]["v"][0], s["best_cost"]) == 71
    assert over(s["b"], s["a"]["v"][0], s["best_cost"]) == 49


def test_session_fixture_bound_only():
    r = TR.session_search()
    best = (r["best_a"], r["best_b"], r["best_cost"])
    want = {"a": (61, 36, 0), "b": (71, 40, 0)}
    for name, other, protect in (("a", "b", best[0]), ("b", "a", best[1])):
        tree, remap, st, keep, f = TR.trim(r[name], r[other]["v"][0], best[2], 0, -1)
        assert (st["n_before"], st["n_kept"], st["n_inherited"]) == want[name]
        assert st["n_over_budget"] == 0 and st["n_protected"] == 0 and st["cut"] == np.inf
        # the best connection's chain passes the bound test by itself, with a margin
        chain = SR.chain(r[name]["parent"], protect)
        assert len(chain) == (4 if name == "a" else 6)
        margin = best[2] - f[chain].max()
        assert abs(margin - (0.21 if name == "a" else 0.29)) < 0.005, margin
        # so protection changes nothing here
        again = TR.trim(r[name], r[other]["v"][0], best[2], 0, protect)
        assert np.array_equal(again[1], remap) and again[2] == st


def test_session_fixture_whole_trim_keeps_the_best_path():
    r = TR.session_search()
    pairs = np.array(sorted(TR.met_pairs(r)), np.int32)
    best = (r["best_a"], r["best_b"], r["best_cost"])
    assert best[:2] in {tuple(p) for p in pairs.tolist()}
    for max_vertices in (0, 40, 24):
        ta, tb, kept, best2, (sa, sb), shared = TR.session_trim(r["a"], r["b"], pairs, best, max_vertices)
        assert bits(best2[2]) == bits(best[2])
        before = SR.join(r["a"], best[0], r["b"], best[1])
        after = SR.join(ta, best2[0], tb, best2[1])
        for x, y in zip(before, after):
            assert np.array_equal(bits(np.asarray(x, np.float64)), bits(np.asarray(y, np.float64)))
        assert shared["n_kept"] >= 1
        if max_vertices:
            assert sa["n_kept"] <= max_vertices + 4 and sb["n_kept"] <= max_vertices + 6
            # 35 and 39 vertices pass the bound: a budget of 40 cuts nothing more, 24 does
            assert (sa["n_over_budget"] > 0 and sb["n_over_budget"] > 0) == (max_vertices == 24)
        print(max_vertices, sa, sb, shared)


def test_set_S_needs_the_protection():
    """The best connection's own start-tree vertex lies 1.3e-15 above the best
    cost: the plain bound test drops the best path's chain."""
    s = R.search("S")
    ta, rb, cost = s["a"], s["b"]["v"][0], s["best_cost"]
    f = TR.f_values(ta, rb)
    assert 0 < f[66] - cost < 2e-15
    plain = TR.trim(ta, rb, cost, 0, -1)
    assert plain[1][66] < 0
    prot = TR.trim(ta, rb, cost, 0, 66)
    chain = SR.chain(ta["parent"], 66)
    assert len(chain) == 7 and np.all(prot[1][chain] >= 0)
    assert prot[2]["n_protected"] >= 1
    assert prot[2]["n_kept"] == plain[2]["n_kept"] + prot[2]["n_protected"] + \
        (plain[2]["n_inherited"] - prot[2]["n_inherited"])
    tb = TR.trim(s["b"], ta["v"][0], cost, 0, 38)
    before = SR.join(ta, 66, s["b"], 38)
    after = SR.join(prot[0], int(prot[1][66]), tb[0], int(tb[1][38]))
    for x, y in zip(before, after):
        assert np.array_equal(bits(np.asarray(x, np.float64)), bits(np.asarray(y, np.float64)))


# ---- 6,017 vertices with 64-way ties ---------------------------------------------------
@pytest.mark.parametrize("permute", [False, True])
def test_big_tree_counts(permute):
    t, rb, cost = TR.big(permute)
    assert len(t["parent"]) == 6017
    if permute:
        assert np.any(t["parent"] > np.arange(6017))
    x = TR.trim(t, rb, cost, 0, -1)
    assert x[2]["n_kept"] == 1473 and x[2]["n_inherited"] == 0
    for max_keep, kept in TR.BUDGETS:
        x = TR.trim(t, rb, np.inf, max_keep, -1)
        assert x[2]["n_kept"] == kept, (max_keep, x[2])
        assert x[2]["n_inherited"] == 0 and x[2]["n_over_bound"] == 0
        assert kept <= max_keep
        assert (x[2]["cut"] == np.inf) == (max_keep >= 6017)
    x = TR.trim(t, rb, np.inf, 1, -1)
    assert x[2]["n_kept"] == 1 and list(np.flatnonzero(x[1] >= 0)) == [0]
    # bound and budget together: the budget counts among all, the bound cuts first
    x = TR.trim(t, rb, cost, 1025, -1)
    assert x[2]["n_over_bound"] == 6017 - 1473 and x[2]["n_over_budget"] > 0
    assert x[2]["n_kept"] + x[2]["n_over_bound"] + x[2]["n_over_budget"] == 6017
    assert x[2]["n_kept"] == 1025


def test_f_never_falls_from_parent_to_child():
    """g grows by the edge's length and h shrinks by that at most, up to
    rounding: in these trees f[child] >= f[parent] holds in the computed
    values too, so a vertex below a dropped one is dropped by its own flag
    (n_inherited = 0; the keep rule under arbitrary flags is the prune's tests')."""
    r, s = TR.session_search(), R.search("S")
    for res in (r, s):
        for name, other in (("a", "b"), ("b", "a")):
            t = res[name]
            f = TR.f_values(t, res[other]["v"][0])
            assert np.all(f[1:] >= f[t["parent"][1:]])


# ---- the C ABI ---------------------------------------------------------------------
NEW = ["gbp_tree_trim_flags_dev", "gbp_tree_trim_host", "gbp_tree_trim_keep_host"]


def test_abi_exports_and_null_handles():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (gbp_\w+)", out))
    assert set(NEW) <= exported and set(NEW) <= set(L.EXPORTS)
    txt = open(os.path.join(ROOT, "include", "gbp.h")).read()
    for name in NEW:
        assert f"int {name}(" in txt
    lib = L.load()
    st = L.TrimStats()
    assert ctypes.sizeof(st) == 64
    one = ctypes.c_int64(1)  # stands for any non-NULL array
    p = ctypes.byref(one)
    assert lib.gbp_tree_trim_flags_dev(None, None, 1, 1.0, 0, -1, p, None, ctypes.byref(st), None) == -2
    assert lib.gbp_tree_trim_host(None, None, 1.0, 0, -1, None, ctypes.byref(st), None) == -2
    assert lib.gbp_tree_trim_keep_host(None, None, 1.0, 0, -1, None, None, 0, ctypes.byref(st), None) == -2


# ---- the remap on the host copy ------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("trim")
    exe = str(d / "tree_trim_probe")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe,
                    os.path.join(HERE, "native", "tree_trim_probe.cpp"),
                    os.path.join(HOST, "gbp_tree_prune.cpp")], check=True)
    count = [0]

    def run(remap, parent, keep):
        """-> (ok, [n_before, n_kept, flagged, inherited], parents of the
        survivors, the old index of each survivor's rows)."""
        count[0] += 1
        path = str(d / f"in{count[0]}.txt")
        with open(path, "w") as f:
            f.write(f"{len(parent)}\n" + "\n".join(" ".join(str(int(x)) for x in row)
                                                   for row in (remap, parent, keep)) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        tok = [int(t) for t in r.stdout.split()]
        if tok[0] == 0:
            return False, None, None, None
        kept = tok[2]
        assert len(tok) == 5 + 2 * kept
        return True, tok[1:5], np.array(tok[5::2], np.int32), np.array(tok[6::2], np.int64)
    return run


def test_trim_remap_probe(probe):
    s = R.search("S")
    ta = s["a"]
    n = len(ta["parent"])
    tree, remap, st, keep, f = TR.trim(ta, s["b"]["v"][0], s["best_cost"], 40, 66)
    ok, rec, p, src = probe(remap, ta["parent"], keep)
    assert ok and rec == [n, st["n_kept"], n - int(keep.sum()), st["n_inherited"]]
    assert np.array_equal(p, tree["parent"]) and np.array_equal(src, np.flatnonzero(remap >= 0))
    # the identity, and the root alone
    ok, rec, p, src = probe(np.arange(n), ta["parent"], np.ones(n))
    assert ok and rec == [n, n, 0, 0] and np.array_equal(p, ta["parent"])
    ok, rec, p, src = probe(np.r_[0, np.full(n - 1, -1)], ta["parent"], np.r_[1, np.zeros(n - 1)])
    assert ok and rec == [n, 1, n - 1, 0] and list(p) == [-1] and list(src) == [0]


def test_trim_remap_probe_refuses_what_is_no_trim(probe):
    parent = np.array([-1, 0, 1, 1], np.int32)
    assert not probe([0, 1, 3, 2], parent, [1, 1, 1, 1])[0]     # not in order
    assert not probe([0, -1, 1, 2], parent, [1, 0, 1, 1])[0]    # kept vertices under a dropped parent
    assert not probe([0, 1, 2, 3], parent, [1, 1, 0, 1])[0]     # a vertex kept against its flag
    ok, rec, p, src = probe([0, -1, -1, -1], parent, [1, 0, 1, 1])   # two go through their parent
    assert ok and rec == [4, 1, 1, 2]
