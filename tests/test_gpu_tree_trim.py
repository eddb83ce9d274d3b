"""Device trees trimmed by cost (gbp_tree_trim_flags_dev / gbp_tree_trim_host,
csrc/gbp_tree_trim.hip, then gbp_tree_prune_dev) against the numpy restatement
in tests/trim_ref.py, bit for bit: keep, f, cut, the counters, the remap, and
v / a / parent / g and the successor lists of the trimmed tree.

The trees are the oracle's (tests/prune_ref.py's set S and its 64 copies,
6,017 vertices with 64-way ties in f), loaded with DeviceTree.load, so no case
depends on a device search.
"""
import ctypes

import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from global_body_planner_amd import engine
from tests import prune_ref as R
from tests import shared_ref as SR
from tests import trim_ref as TR
from tests.helpers import bits, same_f64
from tests.test_gpu_tree_prune import assert_lists_hold_the_children, assert_same_tree

pytestmark = pytest.mark.gpu

INF = float("inf")


def load(tree, capacity=None):
    dt = engine.DeviceTree(tree["v"][0], capacity=capacity or len(tree["parent"]))
    if len(tree["parent"]) > 1:
        dt.load(tree["v"], tree["act"], tree["parent"])
    assert len(dt) == len(tree["parent"])
    return dt


def root_tree(root):
    return engine.DeviceTree(root, capacity=4)


def check_flags(dt, other, tree, other_root, bound, max_keep, protect, label):
    """Stage A alone: keep, f, the record."""
    keep, f, st = dt.trim_flags(other, bound, max_keep, protect)
    rk, rf, rs = TR.flags(tree, other_root, bound, max_keep, protect)
    assert np.array_equal(bits(f.cpu().numpy()), bits(rf)), (label, "f")
    assert np.array_equal(keep.cpu().numpy(), rk), (label, "keep")
    st = st.cpu().numpy()
    assert list(st[:7]) == [rs["n_before"], 0, rs["n_over_bound"], rs["n_over_budget"],
                            rs["n_protected"], 0, 0], (label, st, rs)
    assert st[7:].view(np.uint64)[0] == bits(rs["cut"]), (label, "cut", st[7:].view(np.float64), rs["cut"])
    return keep, rs


def check_trim(tree, other_root, bound=INF, max_keep=0, protect=-1, label=None, flags=True):
    """Both stages on a fresh device tree -> (the device tree, the restatement's result)."""
    label = label or (len(tree["parent"]), bound, max_keep, protect)
    dt, other = load(tree), root_tree(other_root)
    if flags:
        check_flags(dt, other, tree, other_root, bound, max_keep, protect, label)
    remap, stats = dt.trim(other, bound, max_keep, protect)
    ref = TR.trim(tree, other_root, bound, max_keep, protect)
    assert np.array_equal(remap, ref[1]), (label, np.flatnonzero(remap != ref[1])[:10])
    for k in TR.STATS:
        assert stats[k] == ref[2][k], (label, k, stats, ref[2])
    assert stats["error"] == 0 and bits(stats["cut"]) == bits(ref[2]["cut"]), (label, stats)
    assert len(dt) == ref[2]["n_kept"]
    s, a, p, g = dt.read()
    assert_same_tree(dict(v=s, act=a, parent=p, g=g), ref[0], label)
    assert_lists_hold_the_children(dt, p)
    return dt, ref


def prefix(n):
    """The first n vertices of the 6,017-vertex tree as a tree of their own (a
    parent past the end becomes the root), g derived as a load derives it."""
    t = TR.big()[0]
    parent = np.where(t["parent"][:n] < n, t["parent"][:n], 0).astype(np.int32)
    v = t["v"][:n].copy()
    return dict(v=v, act=t["act"][:n].copy(), parent=parent, g=SR.pose_g(v, parent))


def deepest(tree):
    depth = [len(SR.chain(tree["parent"], i)) for i in range(len(tree["parent"]))]
    return int(np.argmax(depth))


# ---- 1: a vertex, a wave and a tile with the root's offset --------------------------------
@pytest.mark.parametrize("n", [1, 2, 65, 1025])
def test_small_trees(gpu, n):
    tree, rb = prefix(n), TR.big()[1]
    f = TR.f_values(tree, rb)
    mid = float(np.median(f[1:])) if n > 1 else 1.0
    leaf = deepest(tree)
    check_trim(tree, rb, bound=mid)
    check_trim(tree, rb, max_keep=n // 2 + 1)
    check_trim(tree, rb, max_keep=1)
    check_trim(tree, rb, bound=mid, max_keep=n // 3 + 1, protect=leaf)
    if n > 1:
        ref = check_trim(tree, rb, bound=0.0, protect=leaf)[1]     # every vertex fails the bound
        assert ref[2]["n_kept"] == len(SR.chain(tree["parent"], leaf)) == ref[2]["n_protected"] + 1


# ---- 2: 6,017 vertices, 64-way ties, every budget ------------------------------------------
@pytest.mark.parametrize("permute", [False, True])
def test_many_tiles_every_budget(gpu, permute):
    tree, rb, cost = TR.big(permute)
    dt, other = load(tree), root_tree(rb)
    for max_keep, kept in TR.BUDGETS + ((1, 1),):
        keep, rs = check_flags(dt, other, tree, rb, INF, max_keep, -1, ("budget", permute, max_keep))
        assert int(keep.sum()) == kept     # (f never falls from parent to child: flags = kept)
    check_flags(dt, other, tree, rb, cost, 0, -1, ("bound", permute))
    check_flags(dt, other, tree, rb, cost, 1025, 66, ("both", permute))
    assert len(dt) == 6017                  # stage A changes nothing
    for max_keep in (1024, 3000):
        ref = check_trim(tree, rb, max_keep=max_keep, flags=False)[1]
        assert ref[2]["n_kept"] == dict(TR.BUDGETS)[max_keep]
    ref = check_trim(tree, rb, bound=cost, flags=False)[1]
    assert ref[2]["n_kept"] == 1473
    # budget and bound together, a protected chain on top
    protect = deepest(tree)
    ref = check_trim(tree, rb, bound=cost, max_keep=1025, protect=protect)[1]
    assert ref[2]["n_over_bound"] > 0 and ref[2]["n_over_budget"] > 0
    assert ref[2]["n_kept"] <= 1025 + len(SR.chain(tree["parent"], protect))


# ---- 3: what cuts nothing ------------------------------------------------------------------
def test_identity(gpu):
    tree, rb, cost = TR.big()
    n = len(tree["parent"])
    for kw in (dict(bound=INF), dict(bound=float("nan")), dict(max_keep=n), dict(max_keep=n + 1),
               dict(bound=float("nan"), max_keep=0, protect=66)):
        dt, ref = check_trim(tree, rb, flags=False, **kw)
        assert np.array_equal(ref[1], np.arange(n)) and ref[2]["n_kept"] == n and ref[2]["cut"] == INF


# ---- 4: the protected chain ------------------------------------------------------------------
def test_protection_keeps_the_best_chain_of_set_S(gpu):
    """Set S, tree a: the best connection's own vertex 66 lies 1.3e-15 above
    the best cost."""
    s = R.search("S")
    ta, rb, cost = s["a"], s["b"]["v"][0], s["best_cost"]
    plain = check_trim(ta, rb, bound=cost)[1]
    assert plain[1][66] < 0
    prot = check_trim(ta, rb, bound=cost, protect=66)[1]
    assert np.all(prot[1][SR.chain(ta["parent"], 66)] >= 0) and prot[2]["n_protected"] >= 1
    check_trim(s["b"], ta["v"][0], bound=cost, protect=38)


def test_protect_at_the_leaf_of_a_deep_chain(gpu):
    """2,000 vertices in one chain against the index order: vertex 1 is 1,999
    edges deep.  Every vertex fails the bound and the whole chain is protected;
    protected from the middle, the lower half goes."""
    n = 2000
    tree = SR.chain_against_the_index_order(n)
    rb = np.zeros(8)
    ref = check_trim(tree, rb, bound=-1.0, protect=1)[1]
    assert ref[2]["n_kept"] == n and ref[2]["n_protected"] == n - 1
    ref = check_trim(tree, rb, bound=-1.0, protect=1000)[1]
    assert ref[2]["n_kept"] == n - 1000 + 1
    ref = check_trim(tree, rb, max_keep=500, protect=1)[1]
    assert ref[2]["n_kept"] == n


# ---- 5: what the entries refuse ----------------------------------------------------------------
def test_errors_leave_the_tree_unchanged(gpu):
    import torch
    from global_body_planner_amd.engine import _ptr, _stream
    lib = L.load()
    s = R.search("S")
    tree, rb = s["a"], s["b"]["v"][0]
    n = len(tree["parent"])
    dt, other = load(tree, capacity=128), root_tree(rb)
    st = L.TrimStats()
    for protect in (n, n + 5, -2):
        assert lib.gbp_tree_trim_host(dt._h, other._h, 1.0, 0, protect, None, ctypes.byref(st), None) == -1
    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(8, dtype=torch.int64, device="cuda")
    remap = torch.empty(n, dtype=torch.int32, device="cuda")
    pst = torch.zeros(4, dtype=torch.int64, device="cuda")
    sm = _stream(0)
    args = (1.0, 0, -1, _ptr(keep), None, _ptr(dst), sm)
    assert lib.gbp_tree_trim_flags_dev(dt._h, other._h, 129, *args) == -5      # > capacity
    assert lib.gbp_tree_trim_flags_dev(dt._h, other._h, 0, *args) == -1
    assert lib.gbp_tree_trim_flags_dev(dt._h, other._h, n, 1.0, 0, n, _ptr(keep), None, _ptr(dst), sm) == -1
    assert lib.gbp_tree_trim_flags_dev(dt._h, None, n, *args) == -2
    # a size that is not the device's count: reported in keep[0] and the record, refused by the prune
    assert lib.gbp_tree_trim_flags_dev(dt._h, other._h, n - 1, *args) == 0
    assert int(keep[0]) == 0 and int(dst[6]) == 1
    assert lib.gbp_tree_prune_dev(dt._h, n - 1, _ptr(keep), _ptr(remap), _ptr(pst), sm) == -5
    assert len(dt) == n
    sv, sa, sp, sg = dt.read()
    assert_same_tree(dict(v=sv, act=sa, parent=sp, g=sg), tree, "unchanged")
    assert_lists_hold_the_children(dt, sp)
    # a protected chain that does not reach the root: a vertex appended with no parent
    dt.append(tree["v"][5], tree["act"][5], [-1])
    assert len(dt) == n + 1
    keep = torch.full((n + 1,), 7, dtype=torch.uint8, device="cuda")
    assert lib.gbp_tree_trim_flags_dev(dt._h, other._h, n + 1, 1.0, 0, n, _ptr(keep), None, _ptr(dst),
                                       sm) == 0
    assert int(keep[0]) == 0 and int(dst[6]) == 2
    assert lib.gbp_tree_trim_host(dt._h, other._h, 1.0, 0, n, None, ctypes.byref(st), None) == -1
    assert lib.gbp_tree_trim_host(dt._h, other._h, 1.0, 40, n, None, ctypes.byref(st), None) == -1
    sv, sa, sp, sg = dt.read()
    assert len(sp) == n + 1 and sp[n] == -1
    assert_same_tree(dict(v=sv[:n], act=sa[:n], parent=sp[:n], g=sg[:n]), tree, "unchanged after a bad chain")


# ---- 6: the two stages on the caller's arrays -----------------------------------------------------
def test_dev_entry_then_the_prune(gpu):
    import torch
    from global_body_planner_amd.engine import _ptr, _stream
    lib = L.load()
    tree, rb, cost = TR.big(True)
    n = len(tree["parent"])
    dt, other = load(tree), root_tree(rb)
    ref = TR.trim(tree, rb, cost, 1500, 66)
    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    f = torch.zeros(n, dtype=torch.float64, device="cuda")
    dst = torch.zeros(8, dtype=torch.int64, device="cuda")
    remap = torch.empty(n, dtype=torch.int32, device="cuda")
    pst = torch.zeros(4, dtype=torch.int64, device="cuda")
    sm = _stream(0)
    assert lib.gbp_tree_trim_flags_dev(dt._h, other._h, n, cost, 1500, 66, _ptr(keep), _ptr(f), _ptr(dst),
                                       sm) == 0
    assert lib.gbp_tree_prune_dev(dt._h, n, _ptr(keep), _ptr(remap), _ptr(pst), sm) == 0
    assert np.array_equal(keep.cpu().numpy(), ref[3]) and np.array_equal(bits(f.cpu().numpy()), bits(ref[4]))
    assert np.array_equal(remap.cpu().numpy(), ref[1])
    flagged = ref[2]["n_over_bound"] + ref[2]["n_over_budget"] - ref[2]["n_protected"]
    assert pst.cpu().tolist() == [n, ref[2]["n_kept"], flagged, ref[2]["n_inherited"]]
    sv, sa, sp, sg = dt.read()
    assert_same_tree(dict(v=sv, act=sa, parent=sp, g=sg), ref[0], "dev entries")
    assert_lists_hold_the_children(dt, sp)


# ---- 7: the search reads the trimmed tree --------------------------------------------------------
def test_nearest_on_the_trimmed_device_tree(gpu):
    """gbp_tree_nearest_dev on the trimmed DeviceTree itself against the fp64
    scan over the restatement's survivors: a root with 5,000 leaves of distinct
    random states, trimmed to half by the budget; among the dropped are the
    rows of the largest magnitude, which set the search bounds before."""
    import torch
    T = engine.Terrain.from_data(R.terrain(None)[0])
    n = 5001
    root = R.start_goal()[0]
    leaves = T.sample_states(n - 1, seed=41, stream_id=1)[0].cpu().numpy()
    q = T.sample_states(4096, seed=42, stream_id=2)[0]
    v = np.vstack([root[None], leaves])
    v[[7, 900, 4100], 0] = 100.0
    parent = np.r_[-1, np.zeros(n - 1)].astype(np.int32)
    act = np.tile(R.search("C")["a"]["act"][1], (n, 1))
    act[0] = 0.0
    tree = dict(v=v, act=act, parent=parent, g=SR.pose_g(v, parent))
    rb = R.start_goal()[1]
    dt, ref = check_trim(tree, rb, max_keep=2501)
    assert ref[2]["n_kept"] == 2501 and np.abs(ref[0]["v"]).max() < 50.0
    survivors = torch.from_numpy(np.ascontiguousarray(ref[0]["v"])).cuda()
    assert np.all(same_f64(dt.read()[0], ref[0]["v"]))
    ws = engine.PlanWorkspace(T, 4096)
    for nqs in (4096, 33, 1):
        qt = q[:nqs].contiguous()
        got = ws.nearest(dt, qt).cpu().numpy()
        want = engine.nearest(qt, survivors)[0].cpu().numpy()
        miss = np.flatnonzero(got != want)
        assert miss.size == 0, (nqs, miss[:5], got[miss[:5]], want[miss[:5]])
