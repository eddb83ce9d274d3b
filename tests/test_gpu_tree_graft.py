"""Device trees grafted onto a root state that is none of their vertices
(gbp_tree_graft_check_dev in csrc/gbp_tree_graft.hip, gbp_tree_graft_dev /
gbp_tree_graft_host in csrc/gbp_tree_maint.hip) against the numpy restatement
in tests/graft_ref.py, bit for bit: the remap, the nine counters, and v / a /
parent / g of the grafted tree; the successor lists are read back and must hold
exactly each vertex's children.

The trees are the oracle's (tests/prune_ref.py: set S, RRT*-Connect with
rewired parents) and synthetic ones, loaded with DeviceTree.load; the roots are
tests/graft_ref.py's; the searches that continue from a grafted tree are
compared with the oracle's continuation from the restatement's.
"""
import ctypes

import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from global_body_planner_amd import engine, planner
from tests import graft_ref as G
from tests import prune_ref as R
from tests import reroot_ref as RR
from tests.helpers import bits, same_f64
from tests.test_gpu_tree_prune import (assert_lists_hold_the_children, assert_same_tree,
                                       device_terrain)

pytestmark = pytest.mark.gpu


def loaded(tree, capacity=None):
    dt = engine.DeviceTree(tree["v"][0], capacity=capacity or len(tree["parent"]))
    dt.load(tree["v"], tree["act"], tree["parent"])
    assert len(dt) == len(tree["parent"])
    return dt


def read_back(dt, stats):
    assert len(dt) == stats["n_kept"]
    s, a, p, g = dt.read()
    assert_lists_hold_the_children(dt, p)
    return dict(v=s, act=a, parent=p, g=g)


def device_graft(tree, root, radius, T, direction, **kw):
    """tree dict -> (grafted tree dict, remap, stats) through DeviceTree.graft."""
    dt = loaded(tree)
    remap, stats = dt.graft(root, radius, T, direction, **kw)
    return read_back(dt, stats), remap, stats


def assert_graft_equals(dev, ref, label):
    (dtree, dremap, dstats), (rtree, rremap, rstats) = dev, ref[:3]
    assert np.array_equal(dremap, rremap), (label, np.flatnonzero(dremap != rremap)[:10])
    for k in G.STATS:
        assert dstats[k] == rstats[k], (label, k, dstats, rstats)
    assert_same_tree(dtree, rtree, label)
    assert not np.any(dtree["act"][0]) and not np.any(np.signbit(dtree["act"][0])), label
    assert dtree["parent"][0] == -1 and bits(dtree["g"][:1])[0] == 0, label


def case_inputs(case):
    name, direction, radius = G.CASES[case]
    return R.search("S")[name], G.case_root(case), radius, direction


# ---- 1: stage A alone ----------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("case", ["a-mid5-r3", "b-mid5-r3"])
def test_stage_a_equals_the_oracle(gpu, case, adaptive):
    tree, root, radius, direction = case_inputs(case)
    T = device_terrain(None)
    ref = G.expected(case, None, adaptive)
    cand, checked, attach, actions = ref[3]
    dt = loaded(tree)
    datt, dact, dfl = (x.cpu().numpy() for x in dt.graft_check(root, radius, T, direction, adaptive))
    dfl = dfl.view(np.uint32)
    assert np.array_equal((dfl & L.F_GRAFT_CANDIDATE) != 0, cand)
    assert np.array_equal((dfl & L.F_GRAFT_CHECKED) != 0, checked)
    fragile = (dfl & L.F_FRAGILE) != 0       # left to the caller: compared through the host entry below
    print(f"{case} adaptive {adaptive}: {int(attach.sum())} attached of {int(cand.sum())}, "
          f"{int(fragile.sum())} fragile")
    assert fragile.sum() <= 2
    assert np.array_equal(datt[~fragile], attach[~fragile])
    assert np.array_equal(((dfl & L.F_VALID) != 0)[~fragile], attach[~fragile] != 0)
    att = (attach != 0) & ~fragile
    assert np.all(same_f64(dact[att], actions[att]))
    assert not np.any(dact[~checked]) and len(dt) == len(tree["parent"])   # stage A changes no tree
    # both stages, FRAGILE checks re-decided: the restatement, whatever the margin
    for eps in (None, 1e-5):
        Te = device_terrain(None, fragile_eps=eps)
        dev = device_graft(tree, root, radius, Te, direction, adaptive=adaptive)
        assert_graft_equals(dev, ref, (case, adaptive, eps))
        if eps is not None:
            assert dev[2]["n_resolved"] > 0
            print(f"  eps {eps}: {dev[2]['n_resolved']} checks re-decided with glibc")


def test_radius_is_inclusive_and_unbounded(gpu):
    case = "a-mid5-r3"
    tree, root, _, direction = case_inputs(case)
    T = device_terrain(None)
    d = np.array([oracle.pose_distance(root, row) for row in tree["v"]])
    j = int(np.argsort(d)[len(d) // 2])
    for radius, inside in ((d[j], True), (np.nextafter(d[j], 0.0), False)):
        ref = G.expected(case, radius=float(radius))
        assert bool(ref[3][0][j]) == inside
        assert ref[2]["n_candidates"] == int((d <= radius).sum())
        assert_graft_equals(device_graft(tree, root, radius, T, direction), ref, ("radius", inside))
    ref = G.expected(case, radius=float("inf"))
    assert ref[2]["n_candidates"] == len(d)
    assert_graft_equals(device_graft(tree, root, np.inf, T, direction), ref, "inf")
    small = float(np.nextafter(d.min(), 0.0))
    ref = G.expected(case, radius=small)
    assert ref[2]["n_candidates"] == 0 and ref[2]["n_kept"] == 1
    dev = device_graft(tree, root, small, T, direction)
    assert_graft_equals(dev, ref, "nothing within the radius")
    assert np.array_equal(dev[0]["v"][0].view(np.uint64), root.view(np.uint64))


def test_root_alone_and_root_on_a_vertex(gpu):
    T = device_terrain(None)
    tree, root, radius, direction = case_inputs("b-goal-shift")
    ref = G.expected("b-goal-shift")
    assert ref[2]["n_kept"] == 1 and ref[2]["n_candidates"] == 62
    assert_graft_equals(device_graft(tree, root, radius, T, direction), ref, "root alone")
    # a root that equals vertex 5's state: a candidate, t_s = 0, not attached
    tree = R.search("S")["a"]
    _, O = R.terrain(None)
    ref = G.graft_on(O, tree, tree["v"][5], 3.0, L.FORWARD)
    cand, checked, attach, _ = ref[3]
    assert cand[5] and not checked[5] and not attach[5] and ref[2]["n_attached"] >= 5
    dev = device_graft(tree, tree["v"][5], 3.0, T, L.FORWARD)
    assert_graft_equals(dev, ref, "root on a vertex")


@pytest.mark.parametrize("case", ["a-mid5-r1", "a-start-shift", "b-v30-shift"])
def test_other_roots(gpu, case):
    tree, root, radius, direction = case_inputs(case)
    dev = device_graft(tree, root, radius, device_terrain(None), direction)
    assert_graft_equals(dev, G.expected(case), case)
    print(case, dev[2])


# ---- 2: stage B alone, synthetic decisions ------------------------------------------------------
ROOT = np.array([0.25, -0.5, 0.75, 0.1, -0.2, 0.3, 0.05, -0.05])


def stage_b(tree, attach, actions, ok=None, capacity=None, root=ROOT):
    import torch
    dt = loaded(tree, capacity)
    dev = torch.device("cuda", 0)
    t_att = torch.from_numpy(np.ascontiguousarray(attach, np.uint8)).to(dev)
    t_act = torch.from_numpy(np.ascontiguousarray(actions, np.float64)).to(dev)
    t_ok = None if ok is None else torch.from_numpy(np.ascontiguousarray(ok, np.uint8)).to(dev)
    remap, stats = dt.graft_apply(root, t_att, t_act, t_ok)
    return (read_back(dt, stats), remap, stats), dt


def synthetic_actions(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 10))


@pytest.mark.parametrize("permute", [False, True])
def test_stage_b_several_tiles(gpu, permute):
    """6,017 vertices of a random recursive tree (six compaction tiles), about
    one vertex in a hundred attached by a seeded draw."""
    tree = RR.random_recursive_tree()
    if permute:
        tree, _ = RR.permuted(tree, 1, 20261021)
        assert np.any(tree["parent"] > np.arange(len(tree["parent"])))
    n = len(tree["parent"])
    attach = (np.random.default_rng(20261103).random(n) < 0.01).astype(np.uint8)
    assert 40 <= attach.sum() <= 80
    actions = synthetic_actions(n, 20261104)
    ref = G.graft(tree, ROOT, attach, actions)
    assert 1 < ref[2]["n_kept"] < n and ref[2]["n_outside"] > 0 and ref[2]["depth"] > 2
    assert attached_under_attached(tree["parent"], attach) >= 1
    dev, _ = stage_b(tree, attach, actions)
    assert_graft_equals(dev, ref, ("tiles", permute))
    if not permute:   # parents preceded their children: they still do
        assert np.all(dev[0]["parent"][1:] < np.arange(1, ref[2]["n_kept"]))
    print(f"permuted {permute}: {dev[2]}")


def attached_under_attached(parent, attach):
    out = 0
    for i in np.flatnonzero(attach):
        p = int(parent[i])
        while p >= 0 and not attach[p]:
            p = int(parent[p])
        out += p >= 0
    return out


def test_stage_b_all_none_one_and_nested(gpu):
    tree = RR.random_recursive_tree()
    n = len(tree["parent"])
    actions = synthetic_actions(n, 20261105)
    # every vertex attached: n + 1 vertices, one more than the capacity, depth 1
    ref = G.graft(tree, ROOT, np.ones(n, np.uint8), actions)
    assert ref[2]["depth"] == 1 and ref[2]["n_kept"] == n + 1
    dev, dt = stage_b(tree, np.ones(n, np.uint8), actions)
    assert_graft_equals(dev, ref, "all")
    assert dt.capacity() >= n + 1
    # none: the root alone
    ref = G.graft(tree, ROOT, np.zeros(n, np.uint8), actions)
    assert ref[2]["n_kept"] == 1 and ref[2]["n_outside"] == n
    assert_graft_equals(stage_b(tree, np.zeros(n, np.uint8), actions)[0], ref, "none")
    # one: vertex 1 and the 3,279 below it
    one = (np.arange(n) == 1).astype(np.uint8)
    ref = G.graft(tree, ROOT, one, actions)
    assert ref[2]["n_kept"] == 1 + 3280 and ref[2]["n_attached"] == 1
    assert_graft_equals(stage_b(tree, one, actions)[0], ref, "one")
    # an ancestor and its descendant: both hang under the root
    child = int(np.flatnonzero(tree["parent"] == 1)[0])
    grand = int(np.flatnonzero(tree["parent"] == child)[0])
    two = np.isin(np.arange(n), (1, grand)).astype(np.uint8)
    ref = G.graft(tree, ROOT, two, actions)
    assert ref[2]["n_kept"] == 1 + 3280 and ref[0]["parent"][ref[1][grand]] == 0
    assert ref[0]["parent"][ref[1][child]] == ref[1][1]
    assert_graft_equals(stage_b(tree, two, actions)[0], ref, "nested")
    # the old root attached: its own entry in edge_valid and its parent -1 are ignored
    root_too = (np.arange(n) == 0).astype(np.uint8)
    ok = (np.arange(n) != 7).astype(np.uint8)
    ok[0] = 0
    ref = G.graft(tree, ROOT, root_too, actions, ok)
    assert ref[2]["n_kept"] > 1 and ref[1][0] == 1 and ref[1][7] == -1
    assert_graft_equals(stage_b(tree, root_too, actions, ok)[0], ref, "old root attached")


def test_stage_b_deep_chain(gpu):
    """Vertex i's parent is i + 1: one attach in the middle keeps vertices
    1 .. 2,048, 2,047 edges deep, each level one vertex wide."""
    n = 4097
    tree = RR.chain_against_the_index_order(n)
    attach = (np.arange(n) == 2048).astype(np.uint8)
    actions = synthetic_actions(n, 20261106)
    ref = G.graft(tree, ROOT, attach, actions)
    assert ref[2]["n_kept"] == 1 + 2048 and ref[2]["depth"] == 2048
    assert np.array_equal(np.flatnonzero(ref[1] >= 0), np.arange(1, 2049))
    assert_graft_equals(stage_b(tree, attach, actions)[0], ref, "chain")


def test_stage_b_full_tree_and_failed_edges(gpu):
    """count == capacity: the graft reserves; and edge decisions: a failed edge
    between an attached vertex and a descendant cuts what hangs below it, a
    failed edge of an attached vertex itself is ignored."""
    tree = RR.random_recursive_tree(2051, seed=20261022)
    n = 2051
    actions = synthetic_actions(n, 20261107)
    attach = np.isin(np.arange(n), (1, 2, 3)).astype(np.uint8)
    ok = (np.random.default_rng(20261108).random(n) >= 0.1).astype(np.uint8)
    ok[1] = 0
    ref = G.graft(tree, ROOT, attach, actions, ok)
    free = G.graft(tree, ROOT, attach, actions)
    assert ref[2]["n_edge_invalid"] > 0 and ref[2]["n_inherited"] > 0
    assert 4 <= ref[2]["n_kept"] < free[2]["n_kept"] and ref[1][1] == 1
    dev, dt = stage_b(tree, attach, actions, ok, capacity=n)
    assert_graft_equals(dev, ref, "edges")
    full = np.ones(n, np.uint8)
    dev, dt = stage_b(tree, full, actions, ok, capacity=n)
    assert_graft_equals(dev, G.graft(tree, ROOT, full, actions, ok), "full")
    assert dev[2]["n_kept"] == n + 1 and dt.capacity() >= n + 1


def test_stage_b_errors_leave_the_tree(gpu):
    import torch
    from global_body_planner_amd.engine import _np_ptr, _ptr, _stream
    lib = L.load()
    T = device_terrain(None)
    tree = R.search("S")["a"]
    n = len(tree["parent"])
    dt = loaded(tree, 128)
    dev = T.torch_device
    att = torch.ones(n + 1, dtype=torch.uint8, device=dev)
    act = torch.zeros((n + 1, 10), dtype=torch.float64, device=dev)
    fl = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    remap = torch.full((n + 1,), 7, dtype=torch.int32, device=dev)
    st = torch.zeros(9, dtype=torch.int64, device=dev)
    s = _stream(T.device)
    root = np.ascontiguousarray(G.case_root("a-mid5-r3"))
    nan_root = root.copy()
    nan_root[2] = np.nan
    hs, k = L.GraftStats(), ctypes.c_int64(0)

    def unchanged():
        sv, sa, sp, sg = dt.read()
        assert len(dt) == n
        assert_same_tree(dict(v=sv, act=sa, parent=sp, g=sg), tree, "refused")
        assert_lists_hold_the_children(dt, sp)

    for wrong in (n - 1, n + 1):
        assert lib.gbp_tree_graft_dev(dt._h, wrong, _np_ptr(root), _ptr(att), _ptr(act), None, _ptr(remap),
                                      _ptr(st), s) == L.E_SHAPE
        assert lib.gbp_tree_graft_check_dev(T._h, dt._h, wrong, _np_ptr(root), 3.0, 0, 0, _ptr(att),
                                            _ptr(act), _ptr(fl), s) == L.E_SHAPE
        unchanged()
    assert lib.gbp_tree_graft_dev(dt._h, 129, _np_ptr(root), _ptr(att), _ptr(act), None, _ptr(remap),
                                  _ptr(st), s) == L.E_SHAPE      # > capacity
    assert lib.gbp_tree_graft_dev(dt._h, n, _np_ptr(nan_root), _ptr(att), _ptr(act), None, _ptr(remap),
                                  _ptr(st), s) == L.E_INVALID_ARG
    assert lib.gbp_tree_graft_dev(dt._h, n, _np_ptr(root), None, _ptr(act), None, _ptr(remap), _ptr(st),
                                  s) == L.E_INVALID_ARG
    assert lib.gbp_tree_graft_dev(dt._h, n, _np_ptr(root), _ptr(att), _ptr(act), None, None, _ptr(st),
                                  s) == L.E_INVALID_ARG
    unchanged()
    for direction, r, radius in ((2, root, 3.0), (0, nan_root, 3.0), (0, root, -1.0), (0, root, np.nan)):
        assert lib.gbp_tree_graft_check_dev(T._h, dt._h, n, _np_ptr(r), radius, direction, 0, _ptr(att),
                                            _ptr(act), _ptr(fl), s) == L.E_INVALID_ARG
        assert lib.gbp_tree_graft_host(T._h, dt._h, _np_ptr(r), radius, direction, 0, 0, None,
                                       ctypes.byref(hs), ctypes.byref(k)) == L.E_INVALID_ARG
        unchanged()
    small = torch.zeros(n - 1, dtype=torch.int32, device=dev)   # a device remap too short
    assert lib.gbp_tree_graft_keep_host(T._h, dt._h, _np_ptr(root), 3.0, 0, 0, 0, None, _ptr(small),
                                        n - 1, ctypes.byref(hs), ctypes.byref(k)) == L.E_SHAPE
    unchanged()
    # and the keep form leaves the remap in the caller's device array
    buf = torch.full((n + 5,), 7, dtype=torch.int32, device=dev)
    remap_h, stats = dt.graft(root, 3.0, T, L.FORWARD, remap_dev=buf)
    ref = G.expected("a-mid5-r3")
    assert np.array_equal(remap_h, ref[1]) and np.array_equal(buf[:n].cpu().numpy(), ref[1])
    assert np.all(buf[n:].cpu().numpy() == 7)
    assert dt.capacity() == 128
    assert_graft_equals((read_back(dt, stats), remap_h, stats), ref, "keep form")


# ---- 3: the map changed and the robot is off the tree ------------------------------------------------
@pytest.mark.parametrize("case", ["b-mid5-r3", "a-mid5-r3"])
def test_both_stages_on_a_changed_map(gpu, case):
    tree, root, radius, direction = case_inputs(case)
    ref = G.expected(case, "box1")
    if case == "b-mid5-r3":
        assert (ref[2]["n_attached"], ref[2]["n_edge_invalid"], ref[2]["n_inherited"],
                ref[2]["n_kept"]) == (14, 6, 8, 35)
    else:   # box 1 stands where this root's connections ran: nothing is attached
        assert ref[2]["n_attached"] == 0 and ref[2]["n_checked"] == 77
    for eps in (None, 1e-5):
        T = device_terrain("box1", fragile_eps=eps)
        dev = device_graft(tree, root, radius, T, direction, test_edges=True)
        assert_graft_equals(dev, ref, (case, "box1", eps))
        if eps is not None:
            assert dev[2]["n_resolved"] > 0
    # through the public call
    data, _ = R.terrain("box1")
    pub = planner.graft_tree(tree, root, radius, data, direction, test_edges=True)
    assert_graft_equals(pub, ref, (case, "public"))


# ---- 4: search rows ------------------------------------------------------------------------------
def test_nearest_on_the_grafted_device_tree(gpu):
    """gbp_tree_nearest_dev on the grafted DeviceTree itself against the
    oracle's scan over the restatement's vertices: the fp16 rows and magnitude
    bounds are the ones the graft wrote from the kept rows and the new root.
    A root with two children and 2,500 leaves under each; child 1 is attached;
    among the dropped are the rows of the largest magnitude and, second case,
    one past the fp16 range."""
    T = device_terrain(None)
    m = 2500
    n = 3 + 2 * m
    leaves = T.sample_states(2 * m + 3, seed=43, stream_id=1)[0].cpu().numpy()
    import torch
    new_root = T.sample_states(1, seed=45, stream_id=3)[0]
    q = torch.cat((new_root, T.sample_states(4095, seed=44, stream_id=2)[0]))   # q[0]: the root itself
    new_root = new_root.cpu().numpy()[0]
    ws = engine.PlanWorkspace(T, 4096)
    rng = np.random.default_rng(23)
    side = rng.permutation(np.r_[np.zeros(m, int), np.ones(m, int)])
    parent = np.r_[-1, 0, 0, 1 + side].astype(np.int32)
    attach = (np.arange(n) == 1).astype(np.uint8)
    actions = synthetic_actions(n, 20261109)
    for far in (100.0, 3e16):
        tree = dict(v=leaves.copy(), act=rng.uniform(-1, 1, (n, 10)), parent=parent)
        gone = np.flatnonzero(parent == 2)
        tree["v"][gone[:5], 0] = far
        ref = G.graft(tree, new_root, attach, actions)
        assert ref[2]["n_kept"] == 2 + m and np.abs(ref[0]["v"]).max() < 50.0 < far
        dev, dt = stage_b(tree, attach, actions, root=new_root)
        assert_graft_equals(dev, ref, ("rows", far))
        for nqs in (4096, 33, 1):
            qt = q[:nqs].contiguous()
            got = ws.nearest(dt, qt).cpu().numpy()
            want = oracle.nearest_batch(qt.cpu().numpy(), ref[0]["v"], nthreads=16)[0]
            assert want[0] == 0   # the new root's own row answers the query that equals it
            miss = np.flatnonzero(got != want)
            assert miss.size == 0, (far, nqs, miss[:5], got[miss[:5]], want[miss[:5]])


# ---- 5: the search goes on, in place ------------------------------------------------------------------
@pytest.mark.parametrize("side", ["a", "b"])
def test_rrt_star_continues_on_the_grafted_device_tree(gpu, side):
    """One tree of set S grafted at its mid-edge root in HBM and the other as it
    is, then 100 RRT*-Connect halves from half 300 on the DeviceTree objects
    themselves (gbp_plan_halves_dev, halts resolved and resumed as the host
    planner does).  Trees, lists, rewires and the best connection equal the
    oracle's continuation from the restated tree."""
    from global_body_planner_amd.engine import _stream
    lib = L.load()
    r = R.search("S")
    T = device_terrain(None)
    batch, seed, first, halves = 1024, 3, 300, 100
    case = f"{side}-mid5-r3"
    ta, tb = loaded(r["a"], 1 << 16), loaded(r["b"], 1 << 16)
    trees = [ta, tb]
    k0 = "ab".index(side)
    remap, stats = trees[k0].graft(G.case_root(case), 3.0, T, G.CASES[case][1])
    assert_graft_equals((read_back(trees[k0], stats), remap, stats), G.expected(case), case)
    ws = engine.PlanWorkspace(T, batch)
    L.check(lib.gbp_plan_star_config(ws._h, 1, 3.0, max(1 << 18, 8 * batch), 1 << 22), "star_config")
    L.check(lib.gbp_plan_reset(ws._h, int(r["ext_counter"]), _stream(0)), "plan_reset")
    st = None
    for half in range(first, first + halves, 2):
        ws.halves(T, ta, tb, half, 2, batch, seed=seed, stream_a=401, stream_b=402)
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
            ws.halves(T, ta, tb, h0, half + 2 - h0, batch, seed=seed, stream_a=401, stream_b=402,
                      first_stage=resume.value)
            st = ws.status()
        assert not st["error"], st["error"]
    ref = G.oracle_continues(side)
    assert (len(ref["a"]["v"]), len(ref["b"]["v"]), ref["rewires"]) == G.CONTINUED[side]
    for dt, name in zip(trees, "ab"):
        s, a, p, g = dt.read()
        assert_same_tree(dict(v=s, act=a, parent=p, g=g), ref[name], ("in place", side, name))
        assert_lists_hold_the_children(dt, p)
    assert st["stat_rewires"] == ref["rewires"]
    assert st["stat_targets"] == ref["targets"] and st["ext_counter"] == ref["ext_counter"]
    assert (st["best_a"], st["best_b"]) == (ref["best_a"], ref["best_b"])
    assert st["best_cost"] == ref["best_cost"]
