"""Tree upkeep at the sizes the planner reaches, and the trim's radix select on
every byte of its keys: prune, re-root, graft and trim on the 70,031-vertex
trees of tests/scale_cases.py (k_prune_gather, k_prune_move_rows and
k_trim_hist take more than one turn of their capped grids there), and the trim
on the key-range tree (f = +0, 2e-150 .. 2e150, values that part in their low
bytes alone, +inf, NaN), against the numpy restatements, bit for bit, with the
assertions of test_gpu_tree_prune.py, _reroot, _graft and _trim.

A tree load runs on one lane (about the time of everything else in a case), so
what changes no tree (stage A of the trim, the edge decisions) shares one loaded
tree per module; an operation that rewrites the tree in place loads its own.
"""
import time

import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from global_body_planner_amd import engine
from tests import graft_ref as G
from tests import prune_ref as R
from tests import reroot_ref as RR
from tests import scale_cases as X
from tests import trim_ref as TR
from tests.helpers import bits, same_f64
from tests.test_gpu_tree_graft import assert_graft_equals
from tests.test_gpu_tree_prune import (assert_lists_hold_the_children, assert_prune_equals,
                                       assert_same_tree, device_terrain)
from tests.test_gpu_tree_reroot import assert_reroot_equals
from tests.test_gpu_tree_trim import check_flags, root_tree

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
LOADS = []          # seconds of each 70,031-vertex load
_shared = {}


def load(tree):
    n = len(tree["parent"])
    dt = engine.DeviceTree(tree["v"][0], capacity=n)
    t0 = time.perf_counter()
    dt.load(tree["v"], tree["act"], tree["parent"])
    if n == X.N_BIG:
        LOADS.append(time.perf_counter() - t0)
        print(f"load of {n} vertices: {LOADS[-1]:.3f} s")
    assert len(dt) == n
    return dt


def shared(name, tree):
    """The module's one loaded copy of a tree, for what leaves it as it is."""
    if name not in _shared:
        _shared[name] = load(tree)
    assert len(_shared[name]) == len(tree["parent"])
    return _shared[name]


def read_back(dt):
    s, a, p, g = dt.read()
    assert_lists_hold_the_children(dt, p)
    return dict(v=s, act=a, parent=p, g=g)


_search = {}


def assert_nearest(dt, survivors, label):
    """gbp_tree_nearest_dev on the device tree against the fp64 scan over the
    restatement's vertices, 256 queries."""
    import torch
    T = device_terrain(None)
    if not _search:
        _search["q"] = T.sample_states(256, seed=46, stream_id=2)[0].contiguous()
        _search["ws"] = engine.PlanWorkspace(T, 256)
    q = _search["q"]
    got = _search["ws"].nearest(dt, q).cpu().numpy()
    want = engine.nearest(q, torch.from_numpy(np.ascontiguousarray(survivors)).cuda())[0].cpu().numpy()
    miss = np.flatnonzero(got != want)
    assert miss.size == 0, (label, miss[:5], got[miss[:5]], want[miss[:5]])


# ---- 1: the prune ---------------------------------------------------------------------------
@pytest.mark.parametrize("permute", [False, True])
def test_revalidate_on_box_1(gpu, permute):
    """k_prune_gather over 70,030 x 9 pieces and k_prune_move_rows over
    70,031 x 9: both past one turn of their grids (58,254 vertices)."""
    import torch
    from global_body_planner_amd.engine import _ptr, _stream
    lib = L.load()
    tree = X.big_tree(permute)[0]
    ok = X.big_edge_valid(permute)
    n = X.N_BIG
    T = device_terrain("box1")
    ref = R.prune(tree, ok)
    # stage A on the caller's arrays: the edge decisions and their flags
    dt = shared(("big", permute), tree)
    dev = T.torch_device
    ev = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    fl = torch.full((n,), -1, dtype=torch.int32, device=dev)
    assert lib.gbp_tree_revalidate_dev(T._h, dt._h, n, L.FORWARD, 0, _ptr(ev), _ptr(fl), _stream(T.device)) == 0
    flags = fl.cpu().numpy().view(np.uint32)
    sure = (flags & L.F_FRAGILE) == 0
    assert sure[0] and flags[0] == 0 and (~sure).sum() <= n // 1000
    assert np.array_equal(ev.cpu().numpy()[sure], ok[sure])
    assert np.array_equal(((flags & L.F_VALID) != 0)[sure][1:], ok[sure][1:] != 0)
    assert len(dt) == n                                      # stage A changes nothing
    # both stages, FRAGILE edges re-decided: remap, stats, the pruned tree, the lists
    own = load(tree)
    remap, stats = own.revalidate(T, L.FORWARD)
    assert len(own) == stats["n_kept"]
    assert_prune_equals((read_back(own), remap, stats), ref, ("box1", permute))
    assert_nearest(own, ref[0]["v"], ("box1", permute))


# ---- 2: the re-root and the graft --------------------------------------------------------------
@pytest.mark.parametrize("edges", [False, True])
def test_reroot_under_a_large_subtree(gpu, edges):
    import torch
    from global_body_planner_amd.engine import _ptr, _stream
    lib = L.load()
    tree, k, ok, _, _, size = X.random_tree()
    n = X.N_BIG
    ref = RR.reroot(tree, k, ok if edges else None)
    assert ref[2]["n_before"] == n and (ref[2]["n_kept"] == size) == (not edges)
    dt = load(tree)
    if edges:       # the caller's edge decisions on the caller's arrays
        dev = torch.device("cuda", 0)
        ev = torch.from_numpy(ok).to(dev)
        remap = torch.full((n,), 7, dtype=torch.int32, device=dev)
        st = torch.full((6,), -1, dtype=torch.int64, device=dev)
        assert lib.gbp_tree_reroot_dev(dt._h, n, k, _ptr(ev), _ptr(remap), _ptr(st), _stream(0)) == 0
        remap, stats = remap.cpu().numpy(), dict(zip(RR.STATS, st.cpu().tolist()))
    else:
        remap, stats = dt.reroot(k)
    assert len(dt) == stats["n_kept"]
    assert_reroot_equals((read_back(dt), remap, stats), ref, ("re-root", edges))
    assert_nearest(dt, ref[0]["v"], ("re-root", edges))


def test_graft_with_the_callers_attach_flags(gpu):
    import torch
    tree, _, ok, attach, actions, _ = X.random_tree()
    ref = G.graft(tree, X.NEW_ROOT, attach, actions, ok)
    dt = load(tree)
    dev = torch.device("cuda", 0)
    remap, stats = dt.graft_apply(X.NEW_ROOT, torch.from_numpy(attach).to(dev),
                                  torch.from_numpy(actions).to(dev), torch.from_numpy(ok).to(dev))
    assert len(dt) == stats["n_kept"]
    assert_graft_equals((read_back(dt), remap, stats), ref, "graft")
    assert_nearest(dt, ref[0]["v"], "graft")


# ---- 3: the trim ---------------------------------------------------------------------------------
def big_trim_cases(tree, rb, cost):
    leaf = X.deepest(tree, TR.f_values(tree, rb))
    return [(cost, 0, -1)] + [(INF, mk, -1) for mk in X.BIG_BUDGETS] + [(X.big_bound(), 32769, leaf)]


@pytest.mark.parametrize("permute", [False, True])
def test_trim_flags_on_70031_vertices(gpu, permute):
    """k_trim_hist: three turns of its 128 workgroups, the last with lanes past
    n; its rows summed by k_trim_pick.  745-way ties at every cut."""
    tree, rb, cost = X.big_tree(permute)
    dt, other = shared(("big", permute), tree), root_tree(rb)
    for bound, max_keep, protect in big_trim_cases(tree, rb, cost):
        check_flags(dt, other, tree, rb, bound, max_keep, protect, ("flags", permute, bound, max_keep))
    assert len(dt) == X.N_BIG


@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("permute", [False, True])
def test_trim_on_70031_vertices(gpu, permute, case):
    tree, rb, cost = X.big_tree(permute)
    bound, max_keep, protect = big_trim_cases(tree, rb, cost)[case]
    label = ("trim", permute, bound, max_keep, protect)
    ref = TR.trim(tree, rb, bound, max_keep, protect)
    dt, other = load(tree), root_tree(rb)
    remap, stats = dt.trim(other, bound, max_keep, protect)
    assert np.array_equal(remap, ref[1]), (label, np.flatnonzero(remap != ref[1])[:10])
    for k in TR.STATS:
        assert stats[k] == ref[2][k], (label, k, stats, ref[2])
    assert stats["error"] == 0 and bits(stats["cut"]) == bits(ref[2]["cut"]), (label, stats)
    assert len(dt) == ref[2]["n_kept"]
    assert_same_tree(read_back(dt), ref[0], label)
    assert_nearest(dt, ref[0]["v"], label)
    if case == 5:
        assert ref[2]["n_over_bound"] > 0 and ref[2]["n_over_budget"] > 0 and ref[2]["n_protected"] > 0


# ---- 4: the select on every byte of its keys ---------------------------------------------------------
def nan_bits_equal(x, y):
    return bool(np.all(same_f64(np.atleast_1d(x), np.atleast_1d(y))))


def key_check_flags(dt, other, tree, root, bound, max_keep, protect, label):
    """check_flags of test_gpu_tree_trim.py with f and cut compared bit for bit
    where they are not NaN and by NaN-ness where they are (host and device may
    differ in the payload)."""
    keep, f, st = dt.trim_flags(other, bound, max_keep, protect)
    rk, rf, rs = X.quiet(TR.flags, tree, root, bound, max_keep, protect)
    assert nan_bits_equal(f.cpu().numpy(), rf), (label, "f")
    assert np.array_equal(keep.cpu().numpy(), rk), (label, "keep", np.flatnonzero(keep.cpu().numpy() != rk)[:10])
    st = st.cpu().numpy()
    assert list(st[:7]) == [rs["n_before"], 0, rs["n_over_bound"], rs["n_over_budget"],
                            rs["n_protected"], 0, 0], (label, st, rs)
    assert nan_bits_equal(st[7:].view(np.float64), rs["cut"]), (label, "cut", st[7:].view(np.float64), rs["cut"])


def key_check_trim(tree, root, bound, max_keep, protect, label):
    dt, other = load(tree), root_tree(root)
    key_check_flags(dt, other, tree, root, bound, max_keep, protect, label)
    remap, stats = dt.trim(other, bound, max_keep, protect)
    ref = X.quiet(TR.trim, tree, root, bound, max_keep, protect)
    assert np.array_equal(remap, ref[1]), (label, np.flatnonzero(remap != ref[1])[:10])
    for k in TR.STATS:
        assert stats[k] == ref[2][k], (label, k, stats, ref[2])
    assert stats["error"] == 0 and nan_bits_equal(stats["cut"], ref[2]["cut"]), (label, stats)
    assert len(dt) == ref[2]["n_kept"]
    got = read_back(dt)
    assert np.array_equal(got["parent"], ref[0]["parent"]), label
    for k in ("v", "act", "g"):
        assert nan_bits_equal(got[k], ref[0][k]), (label, k)
    return ref


@pytest.mark.parametrize("bound", ["inf", "nan", "mid", "zero"])
def test_key_range_budgets(gpu, bound):
    """Every budget of scale_cases.key_budgets (the cut on +0, in a tie run,
    inside the runs that part in their low bytes, on +inf, on NaN) under a
    bound of inf, NaN, the median finite f and 0, with and without a protected
    vertex: one whose f is NaN, so a NaN row survives and is moved.  f is +0,
    positive, +inf or NaN by construction (g + poseDistance); a negative f is
    not reachable through the entry and is not tested."""
    tree, root, x = X.key_tree()
    f = X.key_f()
    fin = f[np.isfinite(f)]
    b = dict(inf=INF, nan=NAN, mid=float(np.median(fin)), zero=0.0)[bound]
    protected = int(np.flatnonzero(np.isnan(f))[3])
    kept_nan = 0
    for name, max_keep in X.key_budgets().items():
        for protect in (-1, protected):
            ref = key_check_trim(tree, root, b, max_keep, protect, (bound, name, max_keep, protect))
            kept_nan += int(np.isnan(ref[0]["g"]).sum())
            if protect >= 0:
                assert ref[1][protect] >= 0
    assert kept_nan > 0


def test_key_range_flags_at_every_budget(gpu):
    """Stage A alone at every budget 1 .. n - 1 on one loaded tree: each of the
    eight rounds chooses among several bytes at hundreds of them."""
    tree, root, _ = X.key_tree()
    dt, other = shared("key", tree), root_tree(root)
    n = len(tree["parent"])
    for max_keep in range(1, n, 7):
        key_check_flags(dt, other, tree, root, INF, max_keep, -1, ("every", max_keep))
