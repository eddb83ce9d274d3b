"""Device trees pruned against a changed terrain (gbp_tree_revalidate_dev /
gbp_tree_prune_dev / gbp_tree_revalidate_host, csrc/gbp_tree_maint.hip) against
the numpy restatement in tests/prune_ref.py, bit for bit: the remap, the four
counters, and v / a / parent / g of the pruned tree.

The trees are the oracle's (tests/prune_ref.py: set S, RRT*-Connect with
rewired parents, and set C, RRT-Connect), loaded with DeviceTree.load, so no
case depends on a device search; the searches that continue from the pruned
trees are compared with the oracle's continuation from the restatement's.
"""
import ctypes
import subprocess

import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from global_body_planner_amd import engine, planner
from tests import prune_ref as R
from tests.helpers import bits, same_f64

pytestmark = pytest.mark.gpu

_terrains = {}


def device_terrain(box, fragile_eps=None):
    key = (box, fragile_eps)
    if key not in _terrains:
        T = engine.Terrain.from_data(R.terrain(box)[0])
        if fragile_eps is not None:
            T.set_option(L.OPT_FRAGILE_EPS, int(round(fragile_eps * 1e15)))
        _terrains[key] = T
    return _terrains[key]


def device_prune(T, tree, direction):
    """tree dict -> (pruned tree dict, remap, stats) through DeviceTree."""
    dt = engine.DeviceTree(tree["v"][0], capacity=len(tree["parent"]))
    dt.load(tree["v"], tree["act"], tree["parent"])
    assert len(dt) == len(tree["parent"])
    remap, stats = dt.revalidate(T, direction)
    assert len(dt) == stats["n_kept"]
    s, a, p, g = dt.read()
    assert_lists_hold_the_children(dt, p)
    return dict(v=s, act=a, parent=p, g=g), remap, stats


def assert_lists_hold_the_children(dt, parent):
    """The device tree's successor lists (child / sibling / prev, read as they
    are in HBM) hold exactly each vertex's children: every list walked from
    `child` along `sibling` is the set prune_ref.children gives for the tree's
    parents, `prev` is the walk backwards, and no vertex is in two lists."""
    child, sibling, prev = dt.read_links()
    n = len(parent)
    want = R.children(parent)
    seen = np.zeros(n, bool)
    for p in range(n):
        got, c, before = [], int(child[p]), -1
        while c >= 0:
            assert 0 <= c < n and not seen[c], (p, c)
            seen[c] = True
            assert prev[c] == before, (p, c, prev[c], before)
            got.append(c)
            before, c = c, int(sibling[c])
        assert sorted(got) == want.get(p, []), (p, got[:8], want.get(p, [])[:8])
    assert not seen[0] and seen[1:].all()
    assert sibling[0] == -1 and prev[0] == -1


def assert_same_tree(dev, ref, label):
    assert dev["parent"].shape == ref["parent"].shape, label
    assert np.array_equal(dev["parent"], ref["parent"]), (label, "parent")
    assert np.all(same_f64(dev["v"], ref["v"])), (label, "v")
    assert np.all(same_f64(dev["act"], ref["act"])), (label, "act")
    assert np.array_equal(bits(dev["g"]), bits(ref["g"])), (label, "g")


def assert_prune_equals(dev, ref, label):
    (dtree, dremap, dstats), (rtree, rremap, rstats) = dev, ref
    assert np.array_equal(dremap, rremap), (label, np.flatnonzero(dremap != rremap)[:10])
    for k, v in rstats.items():
        assert dstats[k] == v, (label, k, dstats, rstats)
    assert_same_tree(dtree, rtree, label)


# ---- 1: unchanged terrain ------------------------------------------------------------
@pytest.mark.parametrize("which", ["S", "C"])
def test_unchanged_terrain_keeps_the_tree(gpu, which):
    r = R.search(which)
    T = device_terrain(None)
    for name, direction in (("a", L.FORWARD), ("b", L.REVERSE)):
        tree = r[name]
        n = len(tree["parent"])
        dtree, remap, stats = device_prune(T, tree, direction)
        assert stats["n_kept"] == stats["n_before"] == n
        assert stats["n_edge_invalid"] == stats["n_inherited"] == 0
        assert np.array_equal(remap, np.arange(n))
        assert_same_tree(dtree, tree, (which, name))


# ---- 2: S and C on the three boxes --------------------------------------------------------
@pytest.mark.parametrize("which,box", [(w, b) for w in "SC" for b in ("box1", "box2", "box3")])
def test_changed_terrain_equals_restatement(gpu, which, box):
    r = R.search(which)
    T = device_terrain(box)
    exp = R.expected(which, box)
    for k, (name, direction) in enumerate((("a", L.FORWARD), ("b", L.REVERSE))):
        dev = device_prune(T, r[name], direction)
        assert_prune_equals(dev, exp[k][:3], (which, box, name))
        print(f"{which} {box} tree {name}: {dev[2]}")
    if which == "S" and box in ("box1", "box3"):
        # a rewired vertex (parent > index) survives (tree b on box 1, tree a on
        # box 3: asserted on the restatement), so its renumbered parent was compared
        assert any(np.any(e[0]["parent"] > np.arange(len(e[0]["parent"]))) for e in exp)
    if (which, box) == ("S", "box2"):
        assert exp[0][2]["n_kept"] == 1   # the root alone
    if (which, box) == ("S", "box3"):
        assert exp[1][2]["n_kept"] == 1


def test_dev_entries_on_caller_arrays_and_argument_checks(gpu):
    """gbp_tree_revalidate_dev / gbp_tree_prune_dev with the caller's device
    arrays on the caller's stream (C tree a on box 1: no FRAGILE edge at the
    default margin), and what they refuse: a bad direction, a size that is not
    the tree's."""
    import torch
    from global_body_planner_amd.engine import _ptr, _stream
    lib = L.load()
    T = device_terrain("box1")
    tree = R.search("C")["a"]
    ref_tree, ref_remap, ref_stats, ok = R.expected("C", "box1")[0]
    n = len(tree["parent"])
    dt = engine.DeviceTree(tree["v"][0], capacity=64)
    dt.load(tree["v"], tree["act"], tree["parent"])
    dev = T.torch_device
    ev = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    fl = torch.full((n,), -1, dtype=torch.int32, device=dev)
    remap = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    s = _stream(T.device)
    assert lib.gbp_tree_revalidate_dev(T._h, dt._h, n, 2, 0, _ptr(ev), _ptr(fl), s) == -1
    assert lib.gbp_tree_revalidate_dev(T._h, dt._h, 65, 0, 0, _ptr(ev), _ptr(fl), s) == -5  # > capacity
    assert lib.gbp_tree_revalidate_host(T._h, dt._h, 2, 0, None, ctypes.byref(L.PruneStats()),
                                        None) == -1
    # a size that is not the device's count: reported in edge_valid[0], refused by the prune
    assert lib.gbp_tree_revalidate_dev(T._h, dt._h, n - 1, 0, 0, _ptr(ev), _ptr(fl), s) == 0
    assert int(ev[0]) == 0
    assert lib.gbp_tree_prune_dev(dt._h, n - 1, _ptr(ev), _ptr(remap), _ptr(st), s) == -5
    assert len(dt) == n
    # the two stages
    assert lib.gbp_tree_revalidate_dev(T._h, dt._h, n, 0, 0, _ptr(ev), _ptr(fl), s) == 0
    flags = fl.cpu().numpy().view(np.uint32)
    assert int(ev[0]) == 1 and flags[0] == 0 and not np.any(flags & L.F_FRAGILE)
    assert np.array_equal(ev.cpu().numpy(), ok)
    assert np.array_equal((flags[1:] & L.F_VALID) != 0, ok[1:] != 0)
    assert lib.gbp_tree_prune_dev(dt._h, n, _ptr(ev), _ptr(remap), _ptr(st), s) == 0
    assert np.array_equal(remap.cpu().numpy(), ref_remap)
    assert st.cpu().tolist() == [ref_stats[k] for k in ("n_before", "n_kept", "n_edge_invalid",
                                                        "n_inherited")]
    sv, sa, sp, sg = dt.read()
    assert_same_tree(dict(v=sv, act=sa, parent=sp, g=sg), ref_tree, "dev entries")


def test_tree_of_the_root_alone(gpu):
    """Nothing to test, nothing to move: the tree stays its root."""
    root = R.search("C")["a"]["v"][0]
    dt = engine.DeviceTree(root, capacity=4)
    remap, stats = dt.revalidate(device_terrain("box1"), L.FORWARD)
    assert list(remap) == [0]
    assert stats == dict(n_before=1, n_kept=1, n_edge_invalid=0, n_inherited=0, n_resolved=0)
    s, a, p, g = dt.read()
    assert np.array_equal(bits(s[0]), bits(root)) and list(p) == [-1] and g[0] == 0.0


# ---- 3: many tiles --------------------------------------------------------------------
def _copies(tree, copies):
    """`copies` copies of the tree's non-root vertices under its root."""
    m = len(tree["parent"]) - 1
    out = {k: np.concatenate([tree[k][:1]] + [tree[k][1:]] * copies) for k in ("v", "act", "g")}
    par = [np.array([-1], np.int32)]
    for c in range(copies):
        p = tree["parent"][1:].astype(np.int64)
        par.append(np.where(p == 0, 0, p + c * m).astype(np.int32))
    out["parent"] = np.concatenate(par)
    return out


def _permuted(tree, seed):
    """The same tree with its non-root vertices renumbered at random: parents
    land after their children, as RRT*'s rewiring leaves them."""
    n = len(tree["parent"])
    new = np.r_[0, 1 + np.random.default_rng(seed).permutation(n - 1)]   # old index -> new index
    out = {k: np.empty_like(tree[k]) for k in ("v", "act", "g", "parent")}
    for k in ("v", "act", "g"):
        out[k][new] = tree[k]
    out["parent"][new] = np.where(tree["parent"] >= 0, new[tree["parent"]], -1)
    return out


@pytest.mark.parametrize("permute", [False, True])
def test_many_tiles(gpu, permute):
    """6,017 vertices: six tiles of the compaction, more than one workgroup in
    every kernel; expected values from the restatement on box 1."""
    big = _copies(R.search("S")["a"], 64)
    if permute:
        big = _permuted(big, 20251020)
        assert np.any(big["parent"] > np.arange(len(big["parent"])))
    assert len(big["parent"]) == 6017
    _, O = R.terrain("box1")
    ok = R.edge_valid(O, big, L.FORWARD)
    ref = R.prune(big, ok)
    share = ref[2]["n_kept"] / ref[2]["n_before"]
    assert 0.0 < share < 1.0
    pruned = np.flatnonzero(ref[1] < 0)
    assert np.any(np.diff(pruned) > 1)   # not one contiguous run
    dev = device_prune(device_terrain("box1"), big, L.FORWARD)
    assert_prune_equals(dev, ref, ("tiles", permute))


# ---- 4: depth -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4097, 4098])
def test_deep_chain_against_the_index_order(gpu, n):
    """A chain of n vertices whose parents have the larger index: vertex i's
    parent is i + 1, vertex n - 1 hangs under the root, so vertex 1 is n - 1
    edges from the root.  Every edge carries the state and action of a root
    edge of C (valid), the edge into vertex 2048 an action the oracle rejects:
    exactly vertices 1 .. 2048 go.  With 4,097 vertices (4,096 = 2^12 edges)
    12 rounds of pointer jumping reach the root from vertex 1; with 4,098 it
    takes the 13th, the last of ceil(log2 n): one round too few keeps vertex 1."""
    c = R.search("C")["a"]
    j = int(np.flatnonzero(c["parent"] == 0)[0])
    _, O = R.terrain(None)
    s0, a0 = c["v"][0], c["act"][j]
    a_bad = a0.copy()
    a_bad[2] = a_bad[5] = -30.0   # pulled into the ground
    v, _, _, _, _ = O.validate_pairs(np.stack([s0, s0]), np.stack([a0, a_bad]), L.FORWARD)
    assert list(v) == [1, 0]
    m = 2048
    tree = dict(v=np.tile(s0, (n, 1)), act=np.tile(a0, (n, 1)), g=np.zeros(n),
                parent=np.r_[-1, np.arange(2, n), 0].astype(np.int32))
    tree["act"][m] = a_bad
    ok = R.edge_valid(O, tree, L.FORWARD)
    assert np.array_equal(np.flatnonzero(ok == 0), [m])
    ref = R.prune(tree, ok)
    assert np.array_equal(np.flatnonzero(ref[1] < 0), np.arange(1, m + 1))
    assert ref[2]["n_edge_invalid"] == 1 and ref[2]["n_inherited"] == m - 1
    dev = device_prune(device_terrain(None), tree, L.FORWARD)
    assert_prune_equals(dev, ref, "chain")


# ---- 5: FRAGILE edges -------------------------------------------------------------------
def test_fragile_edges_are_redecided_on_the_host(gpu):
    """S on box 1 with the FRAGILE margin widened to 1e-5: flagged edges are
    re-decided with glibc before the prune; the result equals the
    restatement with no exclusion."""
    r = R.search("S")
    T = device_terrain("box1", fragile_eps=1e-5)
    exp = R.expected("S", "box1")
    resolved = 0
    for k, (name, direction) in enumerate((("a", L.FORWARD), ("b", L.REVERSE))):
        dev = device_prune(T, r[name], direction)
        assert_prune_equals(dev, exp[k][:3], ("fragile", name))
        resolved += dev[2]["n_resolved"]
    assert resolved > 0
    print(f"{resolved} edges re-decided with glibc")


# ---- 6: the search goes on ----------------------------------------------------------------
def _continue(which, box, algorithm, halves, first_half):
    from tests.test_gpu_oracle_loop import assert_counters_equal, assert_trees_equal
    r = R.search(which)
    data, O = R.terrain(box)
    start, goal = R.start_goal()
    old = tuple({k: r[t][k] for k in ("v", "act", "parent")} for t in "ab")
    pruned, remaps, stats = planner.revalidate_trees(data, old)
    exp = R.expected(which, box)
    for k in range(2):
        assert_prune_equals((pruned[k], remaps[k], stats[k]), exp[k][:3], (which, box, k))
    ref_init = tuple({k: e[0][k] for k in ("v", "act", "parent")} for e in exp)
    star = algorithm == 5
    cfg = R.SETS[which]
    kw = dict(batch=cfg["batch"], seed=cfg["seed"], max_halves=halves, first_half=first_half,
              extend_base=r["ext_counter"])
    dev = planner.plan_rrt_connect(data, start, goal, algorithm=algorithm, max_time=300.0, trees=True,
                                   init_trees=pruned, **kw)
    streams = dict(stream_a=401, stream_b=402) if star else {}   # the device RRT*'s target streams
    ref = O.plan(start, goal, init_trees=ref_init, star=star, nthreads=16, **streams, **kw)
    assert dev["halves"] == ref["halves"] == halves
    assert dev["found"] == ref["found"]
    assert_counters_equal(dev, ref)
    assert_trees_equal(dev, ref)
    if star:
        assert dev["rewires"] == ref["rewires"] and dev["solutions"] == ref["solutions"]
    print(f"{which} {box}: continued from {[s['n_kept'] for s in stats]} vertices for {halves} halves "
          f"to {len(ref['a']['v'])}+{len(ref['b']['v'])}, found {ref['found']}, "
          f"rewires {ref.get('rewires')}")
    if ref["found"] and star:
        assert (dev["meet_a"], dev["meet_b"]) == (ref["best_a"], ref["best_b"])
        assert dev["path_cost"] == ref["best_cost"]
    return ref


def test_search_continues_from_pruned_rrt_connect_trees(gpu):
    _continue("C", "box1", algorithm=3, halves=40, first_half=200)


def test_search_continues_from_pruned_rrt_star_trees(gpu):
    """The survivors planner.revalidate_trees returns, as a warm start of
    algorithm 5 (the planner loads them into trees of its own: what is checked
    is the returned v / act / parent, not the pruned device arrays; those are
    test_rrt_star_continues_on_the_pruned_device_trees')."""
    _continue("S", "box1", algorithm=5, halves=10, first_half=300)


def test_rrt_star_rewires_the_pruned_trees(gpu):
    """The 10 halves above insert vertices but rewire none; 100 halves do
    (5 rewires, and a path)."""
    ref = _continue("S", "box1", algorithm=5, halves=100, first_half=300)
    assert ref["rewires"] > 0 and ref["found"]


def test_rrt_star_continues_on_the_pruned_device_trees(gpu):
    """The device planner loop run on the pruned DeviceTree objects
    themselves, with no read-back and reload in between: S on box 1 pruned in
    HBM, then 100 RRT*-Connect halves from half 300 (gbp_plan_halves_dev with
    the star configuration, halts resolved and resumed as the host planner
    does).  The targets' nearest-vertex search reads the fp16 rows and bounds
    the prune wrote; every insertion links into the rebuilt successor lists;
    the rewires (5, one of them of a vertex of the pruned tree b) unlink
    through `prev` and update g down the lists.  Trees, rewires and the best
    connection equal the oracle's continuation from the restatement's trees."""
    from global_body_planner_amd.engine import _stream
    lib = L.load()
    r = R.search("S")
    _, O = R.terrain("box1")
    T = device_terrain("box1")
    exp = R.expected("S", "box1")
    start, goal = R.start_goal()
    batch, seed, first, halves = 1024, 3, 300, 100
    trees = []
    for name, direction in (("a", L.FORWARD), ("b", L.REVERSE)):
        dt = engine.DeviceTree(r[name]["v"][0], capacity=1 << 16)
        dt.load(r[name]["v"], r[name]["act"], r[name]["parent"])
        dt.revalidate(T, direction)
        trees.append(dt)
    ta, tb = trees
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
    ref_init = tuple({k: e[0][k] for k in ("v", "act", "parent")} for e in exp)
    ref = O.plan(start, goal, init_trees=ref_init, star=True, nthreads=16, stream_a=401, stream_b=402,
                 batch=batch, seed=seed, max_halves=halves, first_half=first,
                 extend_base=r["ext_counter"])
    assert ref["rewires"] > 0 and ref["found"]
    n0 = len(ref_init[1]["parent"])   # a vertex of the pruned tree b was rewired
    assert np.any(ref["b"]["parent"][:n0] != ref_init[1]["parent"])
    for dt, name in zip(trees, "ab"):
        s, a, p, g = dt.read()
        assert_same_tree(dict(v=s, act=a, parent=p, g=g), ref[name], ("in place", name))
        assert_lists_hold_the_children(dt, p)
    assert st["stat_rewires"] == ref["rewires"]
    assert st["stat_targets"] == ref["targets"] and st["ext_counter"] == ref["ext_counter"]
    assert (st["best_a"], st["best_b"]) == (ref["best_a"], ref["best_b"])
    assert st["best_cost"] == ref["best_cost"]
    print(f"in place: {halves} halves to {len(ref['a']['v'])}+{len(ref['b']['v'])} vertices, "
          f"{ref['rewires']} rewires, {st['stat_fragile_resolved']} re-decided, targets "
          f"{st['stat_targets']} / {ref['targets']}, extend counter {st['ext_counter']} / "
          f"{ref['ext_counter']}")


def test_nearest_on_the_pruned_device_tree(gpu):
    """gbp_tree_nearest_dev on the pruned DeviceTree itself against the fp64
    scan over the restatement's survivors: the fp16 rows and magnitude bounds
    the prune wrote are the ones the matrix-core search reads.  The tree is a
    root with 5,000 leaves of distinct random states (a leaf's own state is in
    no edge check, so it is free), about half of them under an action the
    oracle rejects, in runs, so the root's successor list is walked past runs
    of pruned siblings.  Among the pruned leaves are the rows of the largest
    magnitude (|x| = 100, which set the bounds before the prune) and, second
    case, one past the fp16 rows' range (3e16: before the prune the tree is
    searched in fp64, after it on the matrix cores)."""
    import torch
    c = R.search("C")["a"]
    j = int(np.flatnonzero(c["parent"] == 0)[0])
    _, O = R.terrain("box1")
    T = device_terrain("box1")
    a_bad = c["act"][j].copy()
    a_bad[2] = a_bad[5] = -30.0
    valid = O.validate_pairs(np.stack([c["v"][0]] * 2), np.stack([c["act"][j], a_bad]), L.FORWARD)[0]
    assert list(valid) == [1, 0]
    n = 5001
    rng = np.random.default_rng(17)
    bad = np.r_[False, rng.random(n - 1) < 0.5]
    leaves = T.sample_states(n - 1, seed=41, stream_id=1)[0].cpu().numpy()
    q = T.sample_states(4096, seed=42, stream_id=2)[0]
    ws = engine.PlanWorkspace(T, 4096)
    for far in (100.0, 3e16):
        tree = dict(v=np.vstack([c["v"][:1], leaves]), act=np.tile(c["act"][j], (n, 1)), g=np.zeros(n),
                    parent=np.r_[-1, np.zeros(n - 1)].astype(np.int32))
        tree["act"][bad] = a_bad
        gone = np.flatnonzero(bad)
        tree["v"][gone[:5], 0] = far
        ok = R.edge_valid(O, tree, L.FORWARD)
        assert np.array_equal(ok == 0, bad)
        ref = R.prune(tree, ok)
        assert np.abs(ref[0]["v"]).max() < 50.0 < far
        dt = engine.DeviceTree(tree["v"][0], capacity=n)
        dt.load(tree["v"], tree["act"], tree["parent"])
        remap, stats = dt.revalidate(T, L.FORWARD)
        assert np.array_equal(remap, ref[1])
        assert_lists_hold_the_children(dt, dt.read()[2])
        survivors = torch.from_numpy(np.ascontiguousarray(ref[0]["v"])).cuda()
        assert np.all(same_f64(dt.read()[0], ref[0]["v"]))
        for nqs in (4096, 33, 1):
            qt = q[:nqs].contiguous()
            got = ws.nearest(dt, qt).cpu().numpy()
            want = engine.nearest(qt, survivors)[0].cpu().numpy()
            miss = np.flatnonzero(got != want)
            assert miss.size == 0, (far, nqs, miss[:5], got[miss[:5]], want[miss[:5]])


# ---- 7: RRTConnectClass::revalidateTrees -------------------------------------------------
def test_revalidate_trees_class_call(gpu, tmp_path):
    """tests/integration/revalidate_trees_node.cpp: the oracle's C trees and the
    box-1 map through FastTerrainMap::loadDataFlat and
    RRTConnectClass::revalidateTrees; the printed PruneStats and the
    survivors' parents equal the restatement's."""
    from tests.test_abi import build_node_callsite
    exe = build_node_callsite(tmp_path / "revalidate_trees_node", src="revalidate_trees_node.cpp")
    data, _ = R.terrain("box1")
    r = R.search("C")
    nx, ny = data.z.shape
    path = tmp_path / "input.bin"
    with open(path, "wb") as f:
        f.write(np.array([nx, ny], np.int32).tobytes())
        layers = [data.x, data.y, data.z,
                  np.zeros((nx, ny)) if data.dx is None else data.dx,
                  np.zeros((nx, ny)) if data.dy is None else data.dy,
                  np.ones((nx, ny)) if data.dz is None else data.dz]
        for arr in layers:
            f.write(np.ascontiguousarray(arr, np.float64).tobytes())
        for t in "ab":
            f.write(np.array([len(r[t]["parent"])], np.int32).tobytes())
            for k in ("v", "act", "g"):
                f.write(np.ascontiguousarray(r[t][k], np.float64).tobytes())
            f.write(np.ascontiguousarray(r[t]["parent"], np.int32).tobytes())
    out = subprocess.run(["timeout", "-k", "10", "120", exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == 4
    for k, e in enumerate(R.expected("C", "box1")):
        st = e[2]
        got = [int(x) for x in lines[2 * k].split()]
        assert got[:4] == [st["n_before"], st["n_kept"], st["n_edge_invalid"], st["n_inherited"]]
        assert [int(x) for x in lines[2 * k + 1].split()] == list(e[0]["parent"])
