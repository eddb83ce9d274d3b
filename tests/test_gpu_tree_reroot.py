"""Device trees re-rooted at one of their vertices (gbp_tree_reroot_dev /
gbp_tree_reroot_host, csrc/gbp_tree_maint.hip) against the numpy restatement in
tests/reroot_ref.py, bit for bit: the remap, the six counters, and v / a /
parent / g of the re-rooted tree; the successor lists are read back and must
hold exactly each vertex's children.

The trees are the oracle's (tests/prune_ref.py: set S, RRT*-Connect with
rewired parents, and set C, RRT-Connect) and synthetic ones, loaded with
DeviceTree.load; the searches that continue from a re-rooted tree are compared
with the oracle's continuation from the restatement's.
"""
import ctypes
import subprocess

import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from global_body_planner_amd import engine, planner
from tests import prune_ref as R
from tests import reroot_ref as RR
from tests.helpers import bits, same_f64
from tests.test_gpu_tree_prune import (assert_lists_hold_the_children, assert_prune_equals,
                                       assert_same_tree, device_terrain)

pytestmark = pytest.mark.gpu


def loaded(tree, capacity=None):
    dt = engine.DeviceTree(tree["v"][0], capacity=capacity or len(tree["parent"]))
    dt.load(tree["v"], tree["act"], tree["parent"])
    assert len(dt) == len(tree["parent"])
    return dt


def device_reroot(tree, k, T=None, direction=L.FORWARD):
    """tree dict -> (re-rooted tree dict, remap, stats) through DeviceTree."""
    dt = loaded(tree)
    remap, stats = dt.reroot(k, T, direction)
    assert len(dt) == stats["n_kept"]
    s, a, p, g = dt.read()
    assert_lists_hold_the_children(dt, p)
    return dict(v=s, act=a, parent=p, g=g), remap, stats


def assert_reroot_equals(dev, ref, label):
    (dtree, dremap, dstats), (rtree, rremap, rstats) = dev, ref
    assert np.array_equal(dremap, rremap), (label, np.flatnonzero(dremap != rremap)[:10])
    for k in RR.STATS:
        assert dstats[k] == rstats[k], (label, k, dstats, rstats)
    assert_same_tree(dtree, rtree, label)
    assert not np.any(dtree["act"][0]) and not np.any(np.signbit(dtree["act"][0])), label
    assert dtree["parent"][0] == -1 and bits(dtree["g"][:1])[0] == 0, label


# ---- 1: identity -------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["S", "C"])
def test_root_zero_is_the_identity(gpu, which):
    r = R.search(which)
    for name in "ab":
        tree = r[name]
        n = len(tree["parent"])
        dtree, remap, stats = device_reroot(tree, 0)
        assert np.array_equal(remap, np.arange(n))
        assert stats["n_kept"] == stats["n_before"] == n
        assert stats["n_outside"] == stats["n_edge_invalid"] == stats["n_inherited"] == 0
        assert stats["depth"] == RR.reroot(tree, 0)[2]["depth"]
        assert_same_tree(dtree, tree, (which, name))   # g included: the oracle's own bits


# ---- 2: the oracle's trees ---------------------------------------------------------------
def _leaf(tree):
    return int(np.setdiff1d(np.arange(len(tree["parent"])), tree["parent"]).max())


@pytest.mark.parametrize("which,name,k", [("S", "a", 1), ("S", "a", 5), ("S", "a", 36),
                                          ("S", "a", "leaf"), ("S", "b", 30), ("S", "b", 57),
                                          ("C", "a", 1), ("C", "a", 3)])
def test_oracle_trees_equal_restatement(gpu, which, name, k):
    tree = R.search(which)[name]
    if k == "leaf":
        k = _leaf(tree)
    ref = RR.reroot(tree, k)
    if k == _leaf(tree):
        assert ref[2]["n_kept"] == 1 and ref[2]["depth"] == 0   # the root alone
    if (which, name, k) in (("S", "a", 36), ("S", "b", 57)):
        # a descendant with a smaller index: the new root really leaves the order
        assert np.flatnonzero(ref[1] >= 0).min() < k
    dev = device_reroot(tree, k)
    assert_reroot_equals(dev, ref, (which, name, k))
    if which == "C":
        p = dev[0]["parent"]
        assert np.all(p[1:] < np.arange(1, len(p)))   # every parent precedes its child
    print(f"{which} {name} at {k}: {dev[2]}")


# ---- 3: with the map changed ----------------------------------------------------------------
@pytest.mark.parametrize("eps", [None, 1e-5])
def test_map_changed_and_robot_moved(gpu, eps):
    tree = R.search("S")["a"]
    T = device_terrain("box1", fragile_eps=eps)
    dt = loaded(tree)
    _, pst = dt.revalidate(T, L.FORWARD)   # the prune's count of re-decided edges
    resolved = []
    for k, kept, under in ((1, 4, 62), (36, 35, 35), (5, 1, 55)):
        ref = RR.expected("S", "a", k, "box1")
        assert ref[2]["n_kept"] == kept and ref[2]["n_before"] - ref[2]["n_outside"] == under
        dev = device_reroot(tree, k, T, L.FORWARD)
        assert_reroot_equals(dev, ref, ("box1", k, eps))
        resolved.append(dev[2]["n_resolved"])
    assert resolved == [pst["n_resolved"]] * 3
    if eps is not None:
        assert resolved[0] > 0
    print(f"eps {eps}: {resolved[0]} edges re-decided with glibc")


# ---- 4: several tiles -----------------------------------------------------------------------
@pytest.mark.parametrize("permute", [False, True])
def test_several_tiles(gpu, permute):
    """6,017 vertices of a random recursive tree: six compaction tiles, wide
    levels (a launch each) and narrow ones; vertex 1 heads 3,280 of them."""
    tree, k = RR.random_recursive_tree(), 1
    assert RR.reroot(tree, 0)[2]["depth"] == 18
    if permute:
        tree, k = RR.permuted(tree, k, 20261021)
        assert np.any(tree["parent"] > np.arange(len(tree["parent"])))
    ref = RR.reroot(tree, k)
    assert ref[2]["n_kept"] == 3280 and ref[2]["n_before"] == 6017
    dev = device_reroot(tree, k)
    assert_reroot_equals(dev, ref, ("tiles", permute))
    # the whole tree too: every level, the widest ones included
    assert_reroot_equals(device_reroot(tree, 0), RR.reroot(tree, 0), ("tiles, whole", permute))


# ---- 4b: the prune is a re-root at the root -------------------------------------------------
def test_prune_equals_a_reroot_at_the_root(gpu):
    """gbp_tree_prune_dev and gbp_tree_reroot_dev(new_root = 0) are one
    pipeline: on the same tree and the same edge decisions they write the same
    remap, tree and counters.  2,051 vertices (two full compaction tiles and a
    tile of 3) of a random recursive tree, renumbered so that parents follow
    their children; about one edge in ten fails, drawn at random."""
    import torch
    from global_body_planner_amd.engine import _ptr, _stream
    lib = L.load()
    n = 2051
    tree, k = RR.permuted(RR.random_recursive_tree(n, seed=20261022), 0, 20261023)
    assert k == 0 and np.any(tree["parent"] > np.arange(n))
    ok = (np.random.default_rng(20261024).random(n) >= 0.1).astype(np.uint8)
    assert 0.05 < 1.0 - ok.mean() < 0.15
    ref_p = R.prune(dict(tree, g=RR.derive_g(tree["v"], tree["parent"])), ok)
    ref_r = RR.reroot(tree, 0, ok)
    share = ref_p[2]["n_kept"] / n
    assert 0.0 < share < 1.0
    assert np.any(np.diff(np.flatnonzero(ref_p[1] < 0)) > 1)   # not one contiguous run
    T = device_terrain(None)
    dev = T.torch_device
    s = _stream(T.device)
    ev = torch.from_numpy(ok).to(dev)
    got = []
    for reroot in (False, True):
        dt = loaded(tree)
        remap = torch.full((n,), 7, dtype=torch.int32, device=dev)
        st = torch.full((6 if reroot else 4,), -1, dtype=torch.int64, device=dev)
        if reroot:
            rc = lib.gbp_tree_reroot_dev(dt._h, n, 0, _ptr(ev), _ptr(remap), _ptr(st), s)
        else:
            rc = lib.gbp_tree_prune_dev(dt._h, n, _ptr(ev), _ptr(remap), _ptr(st), s)
        assert rc == 0
        sv, sa, sp, sg = dt.read()
        assert_lists_hold_the_children(dt, sp)
        names = RR.STATS if reroot else ("n_before", "n_kept", "n_edge_invalid", "n_inherited")
        got.append((dict(v=sv, act=sa, parent=sp, g=sg), remap.cpu().numpy(),
                    dict(zip(names, st.cpu().tolist()))))
    (ptree, premap, pstats), (rtree, rremap, rstats) = got
    assert np.array_equal(premap, rremap), np.flatnonzero(premap != rremap)[:10]
    assert_same_tree(ptree, rtree, "prune against re-root at 0")
    for name in ("n_before", "n_kept", "n_edge_invalid", "n_inherited"):
        assert pstats[name] == rstats[name], (name, pstats, rstats)
    assert rstats["n_outside"] == 0
    assert rstats["depth"] == ref_r[2]["depth"]
    assert_prune_equals(got[0], ref_p, "prune")
    assert_reroot_equals(got[1], ref_r, "re-root at 0")
    print(f"prune = re-root at 0: {pstats}, depth {rstats['depth']}")


# ---- 5: depth -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(4098, 4097), (4099, 4098), (4098, 2048)])
def test_deep_chain_against_the_index_order(gpu, n, k):
    """Vertex i's parent is i + 1 and vertex n - 1 hangs under the root.  From
    k = n - 1 vertex 1 is n - 2 edges below the new root: 4,096 = 2^12 and
    4,097, so one jumping round too few drops it, and g runs over that many
    levels, each one vertex wide.  k = 2,048 keeps vertices 1 .. 2,048."""
    tree = RR.chain_against_the_index_order(n)
    ref = RR.reroot(tree, k)
    if k == n - 1:
        assert ref[2]["depth"] == n - 2 and ref[2]["n_kept"] == n - 1 and ref[1][1] == 1
    else:
        assert ref[2]["n_kept"] == 2048 and ref[1][2048] == 0 and ref[2]["depth"] == 2047
        assert np.array_equal(np.flatnonzero(ref[1] >= 0), np.arange(1, 2049))
    assert_reroot_equals(device_reroot(tree, k), ref, ("chain", n, k))


# ---- 6: search rows --------------------------------------------------------------------------
def test_nearest_on_the_rerooted_device_tree(gpu):
    """gbp_tree_nearest_dev on the re-rooted DeviceTree itself against the fp64
    scan over the restatement's survivors: the fp16 rows and magnitude bounds
    are the ones the re-root wrote from the kept rows.  A root with two
    children and 2,500 distinct leaves under each; among the dropped are the
    rows of the largest magnitude and, second case, one past the fp16 range."""
    import torch
    T = device_terrain(None)
    m = 2500
    n = 3 + 2 * m
    leaves = T.sample_states(2 * m + 3, seed=43, stream_id=1)[0].cpu().numpy()
    q = T.sample_states(4096, seed=44, stream_id=2)[0]
    ws = engine.PlanWorkspace(T, 4096)
    rng = np.random.default_rng(23)
    side = rng.permutation(np.r_[np.zeros(m, int), np.ones(m, int)])   # the two subtrees interleaved
    parent = np.r_[-1, 0, 0, 1 + side].astype(np.int32)
    for far in (100.0, 3e16):
        tree = dict(v=leaves.copy(), act=rng.uniform(-1, 1, (n, 10)), parent=parent)
        gone = np.flatnonzero(parent == 2)
        tree["v"][gone[:5], 0] = far
        ref = RR.reroot(tree, 1)
        assert ref[2]["n_kept"] == 1 + m
        assert np.abs(ref[0]["v"]).max() < 50.0 < far
        dt = loaded(tree)
        remap, stats = dt.reroot(1)
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


# ---- 7: the search goes on, in place -----------------------------------------------------------
def test_rrt_star_continues_on_the_rerooted_device_tree(gpu):
    """S a re-rooted at 5 in HBM (a vertex of the best path's chain
    0-1-5-36-39-71-66) and S b as it is, then 100 RRT*-Connect halves from half
    300 on the DeviceTree objects themselves (gbp_plan_halves_dev, halts
    resolved and resumed as the host planner does).  Trees, lists, rewires and
    the best connection equal the oracle's continuation from the restated
    tree; a vertex of the re-rooted tree is among the rewired."""
    from global_body_planner_amd.engine import _stream
    lib = L.load()
    r = R.search("S")
    _, O = R.terrain(None)
    T = device_terrain(None)
    _, goal = R.start_goal()
    batch, seed, first, halves = 1024, 3, 300, 100
    ref_a = RR.reroot(r["a"], 5)[0]
    ta, tb = loaded(r["a"], 1 << 16), loaded(r["b"], 1 << 16)
    ta.reroot(5)
    trees = [ta, tb]
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
    ref_init = tuple({k: t[k] for k in ("v", "act", "parent")} for t in (ref_a, r["b"]))
    ref = O.plan(ref_a["v"][0], goal, init_trees=ref_init, star=True, nthreads=16, stream_a=401,
                 stream_b=402, batch=batch, seed=seed, max_halves=halves, first_half=first,
                 extend_base=r["ext_counter"])
    assert ref["rewires"] == 18 and ref["found"]
    assert (len(ref["a"]["v"]), len(ref["b"]["v"])) == (93, 100)
    n0 = len(ref_a["parent"])   # a vertex of the re-rooted tree was rewired
    assert np.any(ref["a"]["parent"][:n0] != ref_a["parent"])
    for dt, name in zip(trees, "ab"):
        s, a, p, g = dt.read()
        assert_same_tree(dict(v=s, act=a, parent=p, g=g), ref[name], ("in place", name))
        assert_lists_hold_the_children(dt, p)
    assert st["stat_rewires"] == ref["rewires"]
    assert st["stat_targets"] == ref["targets"] and st["ext_counter"] == ref["ext_counter"]
    assert (st["best_a"], st["best_b"]) == (ref["best_a"], ref["best_b"])
    assert st["best_cost"] == ref["best_cost"]


# ---- 8: the search goes on, through the public calls ---------------------------------------------
def _continue(which, k, box, algorithm, halves, first_half):
    from tests.test_gpu_oracle_loop import assert_counters_equal, assert_trees_equal
    r = R.search(which)
    data, O = R.terrain(box)
    _, goal = R.start_goal()
    old = tuple({key: r[t][key] for key in ("v", "act", "parent")} for t in "ab")
    new_a, remap, stats = planner.reroot_tree(old[0], k, data=data if box else None)
    exp = RR.expected(which, "a", k, box)
    assert_reroot_equals((new_a, remap, stats), exp, (which, k, box))
    if box:
        new_b = planner.revalidate_trees(data, old)[0][1]
        assert_same_tree(new_b, R.expected(which, box)[1][0], (which, box, "b"))
        ref_b = R.expected(which, box)[1][0]
    else:
        new_b = ref_b = old[1]
    init = tuple({key: t[key] for key in ("v", "act", "parent")} for t in (new_a, new_b))
    ref_init = tuple({key: t[key] for key in ("v", "act", "parent")} for t in (exp[0], ref_b))
    star = algorithm == 5
    cfg = R.SETS[which]
    kw = dict(batch=cfg["batch"], seed=cfg["seed"], max_halves=halves, first_half=first_half,
              extend_base=r["ext_counter"])
    start = new_a["v"][0]
    dev = planner.plan_rrt_connect(data, start, goal, algorithm=algorithm, max_time=300.0, trees=True,
                                   init_trees=init, **kw)
    streams = dict(stream_a=401, stream_b=402) if star else {}
    ref = O.plan(exp[0]["v"][0], goal, init_trees=ref_init, star=star, nthreads=16, **streams, **kw)
    assert dev["halves"] == ref["halves"]
    assert dev["found"] == ref["found"]
    if star or not ref["found"]:   # RRT-Connect stops at its first solution, RRT* goes on
        assert ref["halves"] == halves
    assert_counters_equal(dev, ref)
    assert_trees_equal(dev, ref)
    if star:
        assert dev["rewires"] == ref["rewires"] and dev["solutions"] == ref["solutions"]
    if ref["found"] and star:
        assert (dev["meet_a"], dev["meet_b"]) == (ref["best_a"], ref["best_b"])
        assert dev["path_cost"] == ref["best_cost"]
    print(f"{which} at {k} {box}: {halves} halves to {len(ref['a']['v'])}+{len(ref['b']['v'])}, "
          f"found {ref['found']}, rewires {ref.get('rewires')}")
    return ref


def test_public_calls_rrt_star_ten_halves(gpu):
    ref = _continue("S", 5, None, algorithm=5, halves=10, first_half=300)
    assert ref["rewires"] == 1


def test_public_calls_rrt_connect(gpu):
    ref = _continue("C", 3, None, algorithm=3, halves=40, first_half=200)
    assert ref["found"] and (len(ref["a"]["v"]), len(ref["b"]["v"])) == (12, 23)


def test_public_calls_robot_moved_and_map_changed(gpu):
    ref = _continue("S", 36, "box1", algorithm=5, halves=100, first_half=300)
    assert ref["found"] and ref["rewires"] == 6
    assert (len(ref["a"]["v"]), len(ref["b"]["v"])) == (81, 97)


# ---- 9: arguments -------------------------------------------------------------------------------
def test_dev_entry_on_caller_arrays_and_argument_checks(gpu):
    import torch
    from global_body_planner_amd.engine import _ptr, _stream
    lib = L.load()
    T = device_terrain(None)
    tree = R.search("C")["a"]
    n = len(tree["parent"])
    dt = loaded(tree, 64)
    dev = T.torch_device
    remap = torch.full((n,), 7, dtype=torch.int32, device=dev)
    st = torch.zeros(6, dtype=torch.int64, device=dev)
    s = _stream(T.device)

    def unchanged():
        sv, sa, sp, sg = dt.read()
        assert len(dt) == n
        assert_same_tree(dict(v=sv, act=sa, parent=sp, g=sg), tree, "refused")
        assert_lists_hold_the_children(dt, sp)

    hs = L.RerootStats()
    for bad in (-1, n):
        assert lib.gbp_tree_reroot_dev(dt._h, n, bad, None, _ptr(remap), _ptr(st), s) == -1
        assert lib.gbp_tree_reroot_host(None, dt._h, bad, 0, 0, None, ctypes.byref(hs), None) == -1
        unchanged()
    assert lib.gbp_tree_reroot_host(T._h, dt._h, 1, 2, 0, None, ctypes.byref(hs), None) == -1
    unchanged()
    for wrong in (n - 1, n + 1):
        assert lib.gbp_tree_reroot_dev(dt._h, wrong, 1, None, _ptr(remap), _ptr(st), s) == -5
        unchanged()
    assert lib.gbp_tree_reroot_dev(dt._h, 65, 1, None, _ptr(remap), _ptr(st), s) == -5   # > capacity
    assert lib.gbp_tree_reroot_dev(dt._h, n, 1, None, None, _ptr(st), s) == -1
    unchanged()
    # the caller's edge decisions on the caller's stream: vertex 3's own edge fails
    ok = np.ones(n, np.uint8)
    ok[3] = 0
    ok[1] = 0   # the new root's own entry is ignored
    ref = RR.reroot(tree, 1, ok)
    assert ref[2]["n_edge_invalid"] == 1 and ref[2]["n_kept"] < RR.reroot(tree, 1)[2]["n_kept"]
    ev = torch.from_numpy(ok).to(dev)
    assert lib.gbp_tree_reroot_dev(dt._h, n, 1, _ptr(ev), _ptr(remap), _ptr(st), s) == 0
    assert np.array_equal(remap.cpu().numpy(), ref[1])
    assert st.cpu().tolist() == [ref[2][k] for k in RR.STATS]
    sv, sa, sp, sg = dt.read()
    assert_same_tree(dict(v=sv, act=sa, parent=sp, g=sg), ref[0], "dev entry")
    assert_lists_hold_the_children(dt, sp)
    cap = ctypes.c_int64(0)
    assert lib.gbp_tree_capacity(dt._h, ctypes.byref(cap)) == 0 and cap.value == 64


# ---- 10: RRTConnectClass::rerootStartTree ---------------------------------------------------------
def test_reroot_start_tree_class_call(gpu, tmp_path):
    """tests/integration/reroot_node.cpp: a search through the class, then
    rerootStartTree at the path's second state and the next search from there
    with warm_*.  The node checks the sequence itself (the kept tree is the
    subtree, g derived, the warm search starts from the kept vertices and
    finds a path from the new start) and prints the re-root's counters; the
    re-rooted tree equals the restatement of the dumped one."""
    from tests.test_abi import build_node_callsite
    exe = build_node_callsite(tmp_path / "reroot_node", src="reroot_node.cpp")
    data, _ = R.terrain(None)
    nx, ny = data.z.shape
    path, dump = tmp_path / "input.bin", tmp_path / "trees.bin"
    with open(path, "wb") as f:
        f.write(np.array([nx, ny], np.int32).tobytes())
        layers = [data.x, data.y, data.z,
                  np.zeros((nx, ny)) if data.dx is None else data.dx,
                  np.zeros((nx, ny)) if data.dy is None else data.dy,
                  np.ones((nx, ny)) if data.dz is None else data.dz]
        for arr in layers + list(R.start_goal()):
            f.write(np.ascontiguousarray(arr, np.float64).tobytes())
    out = subprocess.run(["timeout", "-k", "10", "120", exe, str(path), str(dump)], capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(dump, np.uint8)

    def take(at, dtype, count):
        nb = np.dtype(dtype).itemsize * count
        return raw[at:at + nb].view(dtype).copy(), at + nb

    at, trees = 0, []
    (k,), at = take(at, np.int32, 1)
    for _ in range(2):   # tree a before and after
        (n,), at = take(at, np.int32, 1)
        v, at = take(at, np.float64, 8 * n)
        a, at = take(at, np.float64, 10 * n)
        g, at = take(at, np.float64, n)
        p, at = take(at, np.int32, n)
        trees.append(dict(v=v.reshape(n, 8), act=a.reshape(n, 10), g=g, parent=p))
    (n,), at = take(at, np.int32, 1)
    remap, at = take(at, np.int32, n)
    stats, at = take(at, np.int64, 6)
    assert at == raw.size
    ref = RR.reroot(trees[0], int(k))
    assert np.array_equal(remap, ref[1])
    assert list(stats) == [ref[2][key] for key in RR.STATS]
    assert_same_tree(trees[1], ref[0], "class call")
    print(out.stdout.strip())
