"""RRT*'s kept connections read, loaded and carried through a remap on the
device (gbp_plan_shared_read_host / _load_host / _remap_dev,
csrc/gbp_replan.hip) against the numpy restatement in tests/shared_ref.py, bit
for bit: the list in order, its length, the four counters and the ranked best.

The trees are shared_ref's small ones (300 vertices, every g a multiple of
1 / 4, so equal costs are exact), loaded with DeviceTree.load; their g is read
back once and must be the restatement's.
"""
import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from global_body_planner_amd import engine
from tests import shared_ref as SR
from tests.helpers import bits
from tests.test_gpu_tree_prune import device_terrain

pytestmark = pytest.mark.gpu

MAX_SHARED = 4096
_state = {}


def setup():
    """(workspace, tree a, tree b, their dicts): RRT* configured with room for
    MAX_SHARED connections; the trees as loaded (g checked once)."""
    if not _state:
        T = device_terrain(None)
        ws = engine.PlanWorkspace(T, 256)
        ws.star_config(3.0, 1 << 12, MAX_SHARED)
        ws.reset()
        _state.update(ws=ws, T=T)
    ws = _state["ws"]
    trees = []
    for seed in (11, 12):
        t = SR.small_tree(seed)
        dt = engine.DeviceTree(t["v"][0], capacity=len(t["parent"]))
        dt.load(t["v"], t["act"], t["parent"])
        g = dt.read()[3]
        assert np.array_equal(bits(g), bits(t["g"]))
        assert np.all(g * 4 == np.round(g * 4))   # exact quarters
        trees.append(dt)
    return ws, trees[0], trees[1], SR.small_tree(11), SR.small_tree(12)


def assert_state(ws, pairs, best, label):
    got, ba, bb, bc = ws.shared_read()
    assert got.shape == np.asarray(pairs).reshape(-1, 2).shape, (label, got.shape)
    assert np.array_equal(got, pairs), (label, np.flatnonzero((got != pairs).any(axis=1))[:10])
    st = ws.status()
    assert st["n_shared"] == len(got), label
    assert (st["best_a"], st["best_b"]) == (ba, bb) and bits(st["best_cost"]) == bits(bc), label
    assert (ba, bb) == best[:2], (label, (ba, bb, bc), best)
    assert bits(bc) == bits(best[2]), (label, bc, best[2])


# ---- 1: wave and tile edges ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_lengths_at_wave_and_tile_edges(gpu, n):
    ws, ta, tb, A, B = setup()
    rng = np.random.default_rng(1000 + n)
    na, nb = len(A["parent"]), len(B["parent"])
    pairs = SR.random_pairs(rng, n, na, nb)
    ws.shared_load(ta, tb, pairs)
    assert_state(ws, pairs, SR.rank(pairs, A["g"], B["g"]), ("loaded", n))
    ra, rb = SR.random_remap(rng, na), SR.random_remap(rng, nb)
    want, wstats = SR.remap_pairs(pairs, ra, rb)
    # the trees after the change: the kept vertices in order (a random remap is
    # no prune of the tree's own edges, so they hang under the root)
    ta2, tb2 = _tree_with_g(A, ra >= 0), _tree_with_g(B, rb >= 0)
    stats = ws.shared_remap(ta2[0], tb2[0], ra, rb)
    assert {k: stats[k] for k in SR.STATS} == {k: wstats[k] for k in SR.STATS}, (n, stats, wstats)
    assert stats["error"] == 0
    if n >= 63:
        assert 0 < wstats["n_kept"] < n and wstats["n_dropped_a"] and wstats["n_dropped_b"]
    assert_state(ws, want, SR.rank(want, ta2[1], tb2[1]), ("remapped", n))


def _tree_with_g(tree, keep):
    """The kept vertices as a tree of their own, every one hung under the root
    at its old x (so its g is |x - x0|, exact): (DeviceTree, g)."""
    v, act = tree["v"][keep].copy(), tree["act"][keep].copy()
    parent = np.zeros(len(v), np.int32)
    parent[0] = -1
    dt = engine.DeviceTree(v[0], capacity=len(v))
    dt.load(v, act, parent)
    g = dt.read()[3]
    assert np.array_equal(bits(g), bits(np.abs(v[:, 0] - v[0, 0])))
    return dt, g


# ---- 1b: more tiles than one pass of the tile scan ----------------------------------------------
def test_more_than_1024_tiles(gpu):
    """1,024 x 1,024 + 1 pairs are 1,025 tiles: the one workgroup that scans
    the tiles' counts takes a second pass, with one tile in it, and the tiles
    after the first 1,024 get offsets that carry the first pass's total.  Two
    trees of 64 vertices, the pairs drawn with repeats; each remap drops a few
    vertices.  A workspace of its own with room for the list (max_shared
    1 << 22)."""
    n = 1024 * 1024 + 1
    T = device_terrain(None)
    ws = engine.PlanWorkspace(T, 256)
    ws.star_config(3.0, 1 << 12)
    ws.reset()
    A, B = SR.small_tree(21, 64), SR.small_tree(22, 64)
    trees = []
    for t in (A, B):
        dt = engine.DeviceTree(t["v"][0], capacity=64)
        dt.load(t["v"], t["act"], t["parent"])
        assert np.array_equal(bits(dt.read()[3]), bits(t["g"]))
        trees.append(dt)
    ta, tb = trees
    rng = np.random.default_rng(1000 + n)
    pairs = SR.random_pairs(rng, n, 64, 64)
    ws.shared_load(ta, tb, pairs)
    assert_state(ws, pairs, SR.rank(pairs, A["g"], B["g"]), ("loaded", n))
    ra, rb = SR.random_remap(rng, 64, keep=0.9), SR.random_remap(rng, 64, keep=0.9)
    assert 0 < (ra < 0).sum() < 16 and 0 < (rb < 0).sum() < 16
    want, wstats = SR.remap_pairs(pairs, ra, rb)
    ta2, tb2 = _tree_with_g(A, ra >= 0), _tree_with_g(B, rb >= 0)
    stats = ws.shared_remap(ta2[0], tb2[0], ra, rb)
    assert {k: stats[k] for k in SR.STATS} == {k: wstats[k] for k in SR.STATS}, (stats, wstats)
    assert stats["error"] == 0
    assert 0 < wstats["n_kept"] < n and wstats["n_dropped_a"] and wstats["n_dropped_b"]
    assert wstats["n_kept"] > 1024 * 1024 // 2   # kept pairs on both sides of the passes' boundary
    assert_state(ws, want, SR.rank(want, ta2[1], tb2[1]), ("remapped", n))


# ---- 2: the identity ----------------------------------------------------------------------------
def test_both_remaps_null_is_the_identity(gpu):
    ws, ta, tb, A, B = setup()
    pairs = SR.random_pairs(np.random.default_rng(5), 1500, 300, 300)
    ws.shared_load(ta, tb, pairs)
    before = ws.shared_read()
    stats = ws.shared_remap(ta, tb, None, None)
    assert stats == dict(n_before=1500, n_kept=1500, n_dropped_a=0, n_dropped_b=0, error=0)
    after = ws.shared_read()
    assert np.array_equal(before[0], after[0]) and before[1:3] == after[1:3]
    assert bits(before[3]) == bits(after[3])
    assert_state(ws, pairs, SR.rank(pairs, A["g"], B["g"]), "identity")


@pytest.mark.parametrize("side", "ab")
def test_one_null_remap_and_one_real(gpu, side):
    ws, ta, tb, A, B = setup()
    rng = np.random.default_rng(6)
    pairs = SR.random_pairs(rng, 1100, 300, 300)
    ws.shared_load(ta, tb, pairs)
    r = SR.random_remap(rng, 300)
    keep = r >= 0
    if side == "a":
        (ta, ga), gb = _tree_with_g(A, keep), B["g"]
        want, wstats = SR.remap_pairs(pairs, r, None)
        stats = ws.shared_remap(ta, tb, r, None)
        assert wstats["n_dropped_b"] == 0 < wstats["n_dropped_a"]
    else:
        ga, (tb, gb) = A["g"], _tree_with_g(B, keep)
        want, wstats = SR.remap_pairs(pairs, None, r)
        stats = ws.shared_remap(ta, tb, None, r)
        assert wstats["n_dropped_a"] == 0 < wstats["n_dropped_b"]
    assert stats == wstats
    assert_state(ws, want, SR.rank(want, ga, gb), side)


# ---- 3: nothing survives ------------------------------------------------------------------------
def test_everything_dropped(gpu):
    ws, ta, tb, A, B = setup()
    pairs = SR.random_pairs(np.random.default_rng(7), 700, 300, 300)
    pairs[:, 0] = np.maximum(pairs[:, 0], 1)   # no pair at a's root, which every remap keeps
    ws.shared_load(ta, tb, pairs)
    assert ws.status()["best_a"] >= 0
    root_only = np.r_[0, np.full(299, -1)].astype(np.int32)
    ta2, _ = _tree_with_g(A, root_only >= 0)
    stats = ws.shared_remap(ta2, tb, root_only, None)
    assert stats == dict(n_before=700, n_kept=0, n_dropped_a=700, n_dropped_b=0, error=0)
    assert_state(ws, np.empty((0, 2), np.int32), (-1, -1, np.inf), "all dropped")
    s, a, info = ws.tree_path(ta2, tb)   # the ranked best: there is none
    assert info["n_states"] == 0 and info["error"] == 0 and len(s) == 0 and info["length"] == np.inf


# ---- 4: ties ------------------------------------------------------------------------------------
def test_duplicates_and_equal_costs_go_to_the_earliest(gpu):
    ws, ta, tb, A, B = setup()
    ga, gb = A["g"], B["g"]
    cost = ga[:, None] + gb[None, :]
    # two different pairs of exactly equal cost, cheaper than everything else listed
    a1, b1 = 1, 1
    same = np.argwhere((cost == cost[a1, b1]))
    other = next((int(a), int(b)) for a, b in same if (a, b) != (a1, b1) and a != a1)
    dearer = np.argwhere(cost > cost[a1, b1])[:40].astype(np.int32)
    for first, second in (((a1, b1), other), (other, (a1, b1))):
        pairs = np.r_[dearer[:20], [first], dearer[20:], [second], [first], [second]].astype(np.int32)
        ws.shared_load(ta, tb, pairs)
        want = SR.rank(pairs, ga, gb)
        assert want[:2] == first and want[2] == cost[a1, b1]
        assert_state(ws, pairs, want, ("tie", first))
        # through the identity on one side and a real remap that keeps everything in order
        stats = ws.shared_remap(ta, tb, np.arange(300, dtype=np.int32), None)
        assert stats["n_kept"] == len(pairs)
        assert_state(ws, pairs, want, ("tie, remapped", first))


# ---- 5: the best is reset, not only lowered ----------------------------------------------------
def test_dropped_best_is_not_kept(gpu):
    ws, ta, tb, A, B = setup()
    ga, gb = A["g"], B["g"]
    rng = np.random.default_rng(9)
    pairs = SR.random_pairs(rng, 900, 300, 300)
    pairs = pairs[(pairs[:, 0] > 0) & (pairs[:, 1] > 0)]
    ba, bb, bc = SR.rank(pairs, ga, gb)
    # one cheapest pair only, in the middle of the list
    dearer = pairs[ga[pairs[:, 0]] + gb[pairs[:, 1]] > bc]
    pairs = np.r_[dearer[:400], [(ba, bb)], dearer[400:]].astype(np.int32)
    ws.shared_load(ta, tb, pairs)
    assert_state(ws, pairs, (ba, bb, bc), "before")
    # a's vertex of the best pair pruned with its subtree: the survivors keep their g
    keep = np.ones(300, bool)
    todo = [ba]
    while todo:
        u = todo.pop()
        keep[u] = False
        todo += [int(c) for c in np.flatnonzero(A["parent"] == u)]
    r = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    pruned = dict(v=A["v"][keep], act=A["act"][keep],
                  parent=np.where(A["parent"][keep] >= 0, r[A["parent"][keep]], -1).astype(np.int32))
    ta2 = engine.DeviceTree(pruned["v"][0], capacity=int(keep.sum()))
    ta2.load(pruned["v"], pruned["act"], pruned["parent"])
    ga2 = ta2.read()[3]
    assert np.array_equal(bits(ga2), bits(ga[keep]))
    want, wstats = SR.remap_pairs(pairs, r, None)
    best2 = SR.rank(want, ga2, gb)
    assert best2[0] >= 0 and best2[2] > bc   # a best_cost only ever lowered would keep the stale value
    stats = ws.shared_remap(ta2, tb, r, None)
    assert stats == wstats and wstats["n_dropped_a"] >= 1
    assert_state(ws, want, best2, "after")


# ---- 6: g derived again by a real re-root -------------------------------------------------------
def test_survivors_g_changes_under_a_reroot(gpu):
    import torch
    ws, ta, tb, A, B = setup()
    lib = L.load()
    kids = np.bincount(A["parent"][1:], minlength=300)
    # a vertex under the root that heads a large subtree
    k = max((i for i in range(1, 300) if A["parent"][i] == 0), key=lambda i: _below(A["parent"], i))
    assert kids[k] > 0
    pairs = SR.random_pairs(np.random.default_rng(10), 1300, 300, 300)
    ws.shared_load(ta, tb, pairs)
    remap = torch.empty(300, dtype=torch.int32, device="cuda")
    stats = torch.zeros(6, dtype=torch.int64, device="cuda")
    L.check(lib.gbp_tree_reroot_dev(ta._h, 300, int(k), None, remap.data_ptr(), stats.data_ptr(),
                                    engine._stream(0)), "reroot_dev")
    r = remap.cpu().numpy()
    ga2 = ta.read()[3]
    old = np.flatnonzero(r > 0)
    assert len(old) > 20 and np.any(ga2[r[old]] != A["g"][old])   # g below the new root changed
    want, wstats = SR.remap_pairs(pairs, r, None)
    assert 0 < wstats["n_kept"] < len(pairs)
    got = ws.shared_remap(ta, tb, remap, None)     # the device array the re-root wrote
    assert got == wstats
    assert_state(ws, want, SR.rank(want, ga2, B["g"]), "rerooted")


def _below(parent, k):
    n, todo = 0, [k]
    kids = {}
    for i, p in enumerate(parent):
        kids.setdefault(int(p), []).append(i)
    while todo:
        u = todo.pop()
        n += 1
        todo += kids.get(u, [])
    return n


# ---- 7: what is refused -------------------------------------------------------------------------
def test_load_validation_leaves_the_list(gpu):
    ws, ta, tb, A, B = setup()
    pairs = SR.random_pairs(np.random.default_rng(11), 130, 300, 300)
    ws.shared_load(ta, tb, pairs)
    best = SR.rank(pairs, A["g"], B["g"])
    for bad in ([[300, 0]], [[0, 300]], [[-1, 0]], [[5, 5]] * 70 + [[0, 300]]):
        with pytest.raises(L.GbpError) as e:
            ws.shared_load(ta, tb, np.array(bad, np.int32))
        assert e.value.status == L.E_INVALID_ARG
        assert_state(ws, pairs, best, bad[-1])
    with pytest.raises(L.GbpError) as e:
        ws.shared_load(ta, tb, np.zeros((MAX_SHARED + 1, 2), np.int32))
    assert e.value.status == L.E_INVALID_ARG
    assert_state(ws, pairs, best, "n > max_shared")
    # exactly max_shared pairs fit
    full = SR.random_pairs(np.random.default_rng(12), MAX_SHARED, 300, 300)
    ws.shared_load(ta, tb, full)
    assert_state(ws, full, SR.rank(full, A["g"], B["g"]), "full")


def test_remap_reports_an_index_outside_the_remap(gpu):
    ws, ta, tb, A, B = setup()
    pairs = SR.random_pairs(np.random.default_rng(13), 1200, 300, 300)
    pairs[1100] = (299, 7)
    ws.shared_load(ta, tb, pairs)
    best = SR.rank(pairs, A["g"], B["g"])
    short = SR.random_remap(np.random.default_rng(14), 299)   # a remap one vertex short
    stats = ws.shared_remap(ta, tb, short, None)
    assert stats["error"] == 1
    assert_state(ws, pairs, best, "index outside the remap")


def test_rrt_star_must_be_configured(gpu):
    T = device_terrain(None)
    ws = engine.PlanWorkspace(T, 64)
    _, ta, tb, _, _ = setup()
    for call in (lambda: ws.shared_read(), lambda: ws.shared_load(ta, tb, [[0, 0]]),
                 lambda: ws.shared_remap(ta, tb, None, None)):
        with pytest.raises(L.GbpError) as e:
            call()
        assert e.value.status == L.E_UNSUPPORTED
