"""The joined path of two device trees extracted on the device
(gbp_tree_path_dev / gbp_tree_path_host, csrc/gbp_replan.hip) against the numpy
restatement of joinTreePaths in tests/shared_ref.py (itself pinned to
csrc/host/gbp_tree_path.cpp by test_shared_ref.py), bit for bit: states,
actions, length and the three counts.
"""
import ctypes

import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from global_body_planner_amd import engine
from tests import prune_ref as R
from tests import shared_ref as SR
from tests.helpers import bits
from tests.test_gpu_tree_prune import assert_same_tree, device_terrain

pytestmark = pytest.mark.gpu


def loaded(tree, capacity=None):
    dt = engine.DeviceTree(tree["v"][0], capacity=capacity or len(tree["parent"]))
    dt.load(tree["v"], tree["act"], tree["parent"])
    return dt


def assert_path(got, want, label):
    (s, a, info), (ws_, wa, wlen, na, nb) = got, want
    assert info["error"] == 0, (label, info)
    assert (info["n_states"], info["n_from_a"], info["n_from_b"]) == (len(ws_), na, nb), (label, info)
    assert s.shape == ws_.shape and np.array_equal(bits(s), bits(ws_)), label
    assert a.shape == wa.shape and np.array_equal(bits(a), bits(wa)), label
    assert bits(info["length"]) == bits(wlen), (label, info["length"], wlen)


def star_search(T, start, goal, batch, seed, halves, stream_a=101, stream_b=102):
    """RRT*-Connect on the device from the roots, in groups of two halves, halts
    resolved and resumed as the host planner does: (workspace, tree a, tree b)."""
    lib = L.load()
    ws = engine.PlanWorkspace(T, batch)
    ws.star_config(3.0, max(1 << 18, 8 * batch), 1 << 16)
    ws.reset()
    trees = [engine.DeviceTree(s, capacity=1 << 16) for s in (start, goal)]
    run_halves(T, ws, trees, 0, halves, batch, seed, stream_a, stream_b)
    return ws, trees[0], trees[1]


def run_halves(T, ws, trees, first, halves, batch, seed, stream_a=101, stream_b=102, group=20):
    lib = L.load()
    ta, tb = trees
    st = None
    for half in range(first, first + halves, group):
        g = min(group, first + halves - half)
        ws.halves(T, ta, tb, half, g, batch, seed=seed, stream_a=stream_a, stream_b=stream_b)
        st = ws.status()
        while st["halt"]:
            assert not st["halt"] & L.PLAN_HALT_STAR_PAIRS
            h0 = st["halt_half"]
            k = h0 & 1
            resume, nres = ctypes.c_int(-1), ctypes.c_int64(0)
            L.check(lib.gbp_plan_resolve_host(T._h, ws._h, trees[k]._h, trees[k ^ 1]._h,
                                              L.FORWARD if k == 0 else L.REVERSE, batch, 0,
                                              ctypes.byref(resume), ctypes.byref(nres), None),
                    "plan_resolve")
            assert resume.value >= 0
            ws.halves(T, ta, tb, h0, half + g - h0, batch, seed=seed, stream_a=stream_a,
                      stream_b=stream_b, first_stage=resume.value)
            st = ws.status()
        assert not st["error"], st["error"]
    return st


# ---- 1: the oracle's RRT*-Connect trees, every kept connection ---------------------------------
def test_every_kept_connection_of_the_oracle_search(gpu):
    """Set S of tests/prune_ref.py grown on the device (trees equal to the
    oracle's bit for bit): the path of every listed connection, and the ranked
    best with no index given."""
    r = R.search("S")
    T = device_terrain(None)
    start, goal = R.start_goal()
    ws, ta, tb = star_search(T, start, goal, **{k: R.SETS["S"][k] for k in ("batch", "seed")},
                             halves=R.SETS["S"]["max_halves"])
    for dt, name in ((ta, "a"), (tb, "b")):
        s, a, p, g = dt.read()
        assert_same_tree(dict(v=s, act=a, parent=p, g=g), r[name], name)
    pairs, ba, bb, bc = ws.shared_read()
    assert len(pairs) == r["solutions"] >= 3
    assert (ba, bb) == (r["best_a"], r["best_b"]) and bits(bc) == bits(r["best_cost"])
    assert (ba, bb) == SR.rank(pairs, r["a"]["g"], r["b"]["g"])[:2]
    depths = []
    for ia, ib in pairs:
        want = SR.join(r["a"], ia, r["b"], ib)
        assert_path(engine.tree_path(ta, tb, ia, ib), want, (ia, ib))
        depths.append(len(want[0]))
    # -1 / -1 with the workspace: the ranked best, read on the device
    got = ws.tree_path(ta, tb)
    assert_path(got, SR.join(r["a"], ba, r["b"], bb), "best")
    assert np.array_equal(bits(got[0][0]), bits(start)) and np.array_equal(bits(got[0][-1]), bits(goal))
    print(f"{len(pairs)} connections, paths of {min(depths)} .. {max(depths)} states")


# ---- 2: one-sided paths ------------------------------------------------------------------------
def test_roots(gpu):
    A, B = SR.small_tree(11), SR.small_tree(12)
    ta, tb = loaded(A), loaded(B)
    leaf_a, leaf_b = 299, 298
    for ia, ib in ((0, leaf_b), (leaf_a, 0), (0, 0), (leaf_a, leaf_b), (17, 170)):
        want = SR.join(A, ia, B, ib)
        assert_path(engine.tree_path(ta, tb, ia, ib), want, (ia, ib))
    assert SR.join(A, 0, B, 0)[0].shape == (1, 8)          # a's root alone, no action
    assert SR.join(A, 0, B, leaf_b)[3] == 1 and SR.join(A, leaf_a, B, 0)[4] == 0


# ---- 3: depth ------------------------------------------------------------------------------------
def test_chain_of_4097_against_the_index_order(gpu):
    """Vertex 1 of the chain is 4,096 edges deep and every parent has the
    larger index: the walk is 4,097 dependent loads on each side."""
    A, B = SR.chain_against_the_index_order(4097), SR.chain_against_the_index_order(4098)
    ta, tb = loaded(A), loaded(B)
    for t, dt in ((A, ta), (B, tb)):
        t["g"] = dt.read()[3]   # the device's own sums (4,096 terms)
    want = SR.join(A, 1, B, 1)
    assert want[3] == 4097 and want[4] == 4097
    assert_path(engine.tree_path(ta, tb, 1, 1, max_states=8194), want, "chain")
    # the first guess too small: reported, then repeated with the length asked for
    assert_path(engine.tree_path(ta, tb, 1, 1, max_states=16), want, "chain, grown")


# ---- 4: a buffer one row too small ---------------------------------------------------------------
def test_max_states_one_too_small_writes_nothing(gpu):
    import torch
    lib = L.load()
    A, B = SR.small_tree(11), SR.small_tree(12)
    ta, tb = loaded(A), loaded(B)
    ia, ib = 299, 298
    want = SR.join(A, ia, B, ib)
    m = len(want[0])
    assert m >= 4
    guard = 8 * 6    # six rows of guard words behind each buffer
    for cap in (m - 1, m):
        s = torch.full((8 * cap + guard,), -7.0, dtype=torch.float64, device="cuda")
        a = torch.full((10 * cap + guard,), -7.0, dtype=torch.float64, device="cuda")
        info = torch.zeros(3, dtype=torch.int64, device="cuda")
        L.check(lib.gbp_tree_path_dev(ta._h, ia, tb._h, ib, None, cap, s.data_ptr(), a.data_ptr(),
                                      info.data_ptr(), engine._stream(0)), "tree_path_dev")
        n, na, nb, err = info.cpu().numpy().view(np.int32)[:4]
        assert (n, na, nb) == (m, want[3], want[4])
        s, a = s.cpu().numpy(), a.cpu().numpy()
        if cap < m:
            assert err == L.PATH_E_SHORT
            assert np.all(s == -7.0) and np.all(a == -7.0)            # nothing written at all
        else:
            assert err == 0
            assert np.array_equal(bits(s[:8 * m]), bits(want[0].ravel()))
            assert np.array_equal(bits(a[:10 * (m - 1)]), bits(want[1].ravel()))
            assert np.all(s[8 * m:] == -7.0) and np.all(a[10 * (m - 1):] == -7.0)
    # the host entry with the short buffer: the length needed, no row
    s, a, info = engine.tree_path(ta, tb, ia, ib, max_states=m - 1, grow=False)
    assert info["error"] == L.PATH_E_SHORT and info["n_states"] == m and len(s) == 0


# ---- 5: the ranked best ---------------------------------------------------------------------------
def test_best_of_a_loaded_list_and_none(gpu):
    T = device_terrain(None)
    A, B = SR.small_tree(11), SR.small_tree(12)
    ta, tb = loaded(A), loaded(B)
    ws = engine.PlanWorkspace(T, 64)
    ws.star_config(3.0, 1 << 12, 1 << 12)
    ws.reset()
    s, a, info = ws.tree_path(ta, tb)          # no connection yet
    assert info == dict(n_states=0, n_from_a=0, n_from_b=0, error=0, length=np.inf) and len(s) == 0
    pairs = SR.random_pairs(np.random.default_rng(21), 500, 300, 300)
    ws.shared_load(ta, tb, pairs)              # ranks the list
    ba, bb, bc = SR.rank(pairs, A["g"], B["g"])
    got = ws.tree_path(ta, tb)
    assert_path(got, SR.join(A, ba, B, bb), "best of the list")
    assert got[2]["length"] == bc
    ws.shared_load(ta, tb, np.empty((0, 2), np.int32))
    assert ws.tree_path(ta, tb)[2]["n_states"] == 0


# ---- 6: what is refused -----------------------------------------------------------------------------
def test_bad_indices(gpu):
    A, B = SR.small_tree(11), SR.small_tree(12)
    ta, tb = loaded(A), loaded(B)
    for ia, ib in ((300, 0), (0, 300)):        # past the count: reported by the kernel
        s, a, info = engine.tree_path(ta, tb, ia, ib)
        assert info["error"] == L.PATH_E_CHAIN and info["n_states"] == 0 and len(s) == 0
    with pytest.raises(L.GbpError) as e:       # -1 / -1 means the best, which needs a workspace
        engine.tree_path(ta, tb, -1, -1)
    assert e.value.status == L.E_INVALID_ARG
    with pytest.raises(L.GbpError) as e:
        engine.tree_path(ta, ta, 1, 1)
    assert e.value.status == L.E_INVALID_ARG
