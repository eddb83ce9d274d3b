"""Python binding of the batched RRT-Connect planner (lib/libgbp_planner.so).

The planner itself is C++ (csrc/host/gbp_planner.cpp, declared in
include/gbp_planner.h): a host mirror of the reference's FastTerrainMap /
planning_utils / PlannerClass / RRTConnectClass whose every validity check,
terrain query, nearest-neighbour scan and candidate draw runs on the HIP engine.
This module only marshals `gbp_plan_rrt_connect` (the flat C entry) — the call
the reference's GlobalBodyPlanner::callPlanner makes
(global_body_planner.cpp:89-131 -> RRTConnectClass::buildRRTConnect).
"""
import ctypes
import os

import numpy as np

from . import _lib

PLANNER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libgbp_planner.so")

_D = ctypes.c_double
_P = ctypes.c_void_p


class PlanParams(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("nx", ctypes.c_int), ("ny", ctypes.c_int),
                ("x", _P), ("y", _P), ("z", _P), ("dx", _P), ("dy", _P), ("dz", _P),
                ("start", _D * 8), ("goal", _D * 8), ("batch", ctypes.c_int),
                ("max_time", _D), ("seed", ctypes.c_uint64), ("post_process", ctypes.c_int),
                ("algorithm", ctypes.c_int), ("max_time_opt", _D),
                ("sampling", _lib.Sampling), ("fragile_eps_fm", ctypes.c_int64),
                ("adaptive", ctypes.c_int), ("nn_stats", ctypes.c_int),
                ("max_halves", ctypes.c_int64),
                ("tree_capacity", ctypes.c_int64), ("tree_v", _P * 2), ("tree_a", _P * 2),
                ("tree_parent", _P * 2), ("tree_g", _P * 2), ("stop_poll", _P),
                ("stop_ctx", _P), ("init_n", ctypes.c_int64 * 2), ("init_v", _P * 2),
                ("init_a", _P * 2), ("init_parent", _P * 2), ("first_half", ctypes.c_int64),
                ("extend_base", ctypes.c_int64), ("stage_timing", ctypes.c_int)]

# int (*stop_poll)(void *ctx, int local_stop, int found)
StopPoll = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int)


class PlanResult(ctypes.Structure):
    _fields_ = [("found", ctypes.c_int), ("time_to_first", _D), ("total_time", _D),
                ("iterations", ctypes.c_int64), ("targets", ctypes.c_int64),
                ("extends", ctypes.c_int64), ("attempts_checked", ctypes.c_int64),
                ("connects", ctypes.c_int64), ("vertices_a", ctypes.c_int64),
                ("vertices_b", ctypes.c_int64), ("n_states", ctypes.c_int),
                ("path_length", _D), ("path_cost", _D), ("path_duration", _D),
                ("rewires", ctypes.c_int64), ("solutions", ctypes.c_int64),
                ("extent_a", _D * 4), ("extent_b", _D * 4),
                ("fragile_resolved", ctypes.c_int64), ("depth_capped", ctypes.c_int64),
                ("status_reads", ctypes.c_int64), ("halts", ctypes.c_int64 * 4),
                ("nn_rechecks", ctypes.c_int64), ("nn_scans", ctypes.c_int64),
                ("reported_length", _D), ("reported_yaw", _D), ("meet_a", ctypes.c_int32),
                ("meet_b", ctypes.c_int32), ("halves", ctypes.c_int64),
                ("polls", ctypes.c_int64), ("stopped_by_peer", ctypes.c_int32),
                ("stage_us", _D * 7), ("stage_halves", ctypes.c_int64)]


_planner = None


def load():
    """Load libgbp_planner.so (raises if it is not built: no fallback)."""
    global _planner
    if _planner is None:
        _lib.load()   # libgbp.so first (the planner links it by rpath)
        if not os.path.exists(PLANNER_PATH):
            raise FileNotFoundError(f"{PLANNER_PATH} is missing: run __graft_entry__.build()")
        L = ctypes.CDLL(PLANNER_PATH)
        L.gbp_plan_rrt_connect.restype = ctypes.c_int
        L.gbp_plan_rrt_connect.argtypes = [ctypes.POINTER(PlanParams), ctypes.POINTER(PlanResult),
                                           _P, _P, ctypes.c_int]
        L.gbp_terrain_arrays_from_csv.restype = ctypes.c_int
        L.gbp_terrain_arrays_from_csv.argtypes = [ctypes.c_char_p, _P, _P, _P, _P, _P, _P, _P, _P,
                                                  ctypes.c_int64]
        L.gbp_attempt_connect_batch.restype = ctypes.c_int
        L.gbp_attempt_connect_batch.argtypes = [_P, ctypes.c_int64, _P, _P, _P, ctypes.c_int,
                                                ctypes.c_int, _P, _P, _P]
        _planner = L
    return _planner


def terrain_from_csv(directory):
    """The C++ ingest (gbp_terrain_arrays_from_csv: TerrainMapPublisher::loadCSV
    + loadMapFromCSV's grid_map geometry + FastTerrainMap::loadDataFromGridMap)
    of the reference CSVs in `directory` -> terrain_data.TerrainData."""
    from .terrain_data import TerrainData
    L = load()
    d = os.fsencode(str(directory))
    nx, ny = ctypes.c_int(0), ctypes.c_int(0)
    rc = L.gbp_terrain_arrays_from_csv(d, ctypes.byref(nx), ctypes.byref(ny), None, None, None,
                                       None, None, None, 0)
    if rc != 0:
        raise _lib.GbpError(rc, f"gbp_terrain_arrays_from_csv({directory})")
    x, y = np.empty(nx.value), np.empty(ny.value)
    z, dx, dy, dz = (np.empty((nx.value, ny.value)) for _ in range(4))
    rc = L.gbp_terrain_arrays_from_csv(d, ctypes.byref(nx), ctypes.byref(ny), x.ctypes.data,
                                       y.ctypes.data, z.ctypes.data, dx.ctypes.data, dy.ctypes.data,
                                       dz.ctypes.data, z.size)
    if rc != 0:
        raise _lib.GbpError(rc, f"gbp_terrain_arrays_from_csv({directory})")
    return TerrainData(x, y, z, dx, dy, dz, name=os.path.basename(str(directory)) + "-cpp-csv")


def start_goal_state(height, x, y):
    """GlobalBodyPlanner::setStartAndGoalStates (global_body_planner.cpp:219-264):
    z = 0.375 + ground height, v = (1, 0, 0), pitch and pitch rate 0."""
    return np.array([x, y, 0.375 + height, 1.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float64)


def plan_rrt_connect(data, start, goal, *, batch=64, max_time=5.0, seed=20251018,
                     post_process=False, device=0, capacity=4096, algorithm=0, max_time_opt=0.0,
                     sampling=None, fragile_eps=None, adaptive=False, nn_stats=False,
                     max_halves=0, trees=False,
                     tree_capacity=1 << 18, stop_poll=None, init_trees=None, first_half=0,
                     extend_base=0, stage_timing=False):
    """Plan start -> goal on terrain `data` (terrain_data.TerrainData).

    algorithm 0: batch-synchronous RRT-Connect, stops at the first solution;
    algorithm 1: batch-synchronous RRT*-Connect, anytime until max_time;
    algorithm 3: as 0, with the search resident on the device (trees in HBM,
      one stream-ordered kernel sequence per half-iteration; same trees and
      path as algorithm 0 for the same seed and batch);
    algorithm 4: as 2, each restart's search resident on the device (what
      buildRRTConnect does by default, RRTConnectClass::set_engine_batch);
    algorithm 5: as 1, the search resident on the device (buildRRTStarConnectDevice:
      same trees, counters and best connection as algorithm 1);
    algorithm 2: RRTConnectClass::buildRRTConnect's anytime restarts
      (rrt_connect.cpp:323-467) on batch-synchronous trees: restart on the
      growing horizon, post-process every solution, keep the cheapest, stop
      once a solution exists and `max_time_opt` seconds have passed.
    Returns a dict with the C result fields plus `states` [n][8] and
    `actions` [n-1][10] (the found path; empty if none).
    sampling: a _lib.Sampling (direction-biased draws, params.yaml:21-27);
    fragile_eps: a wider FRAGILE margin (forces host re-decisions: tests);
    adaptive: the adaptive-step pair checks (params.yaml:16);
    nn_stats: count the matrix-core search's fp64 re-checks (diagnostics);
    max_halves: algorithms 0, 1, 3 stop after this many half-iterations (a
      replayable run; 0 = no limit);
    trees: also return the final trees (out["a"], out["b"]: v, act, parent, g;
      algorithms 0, 1, 3), at most tree_capacity rows each;
    stop_poll: algorithm 3 — f(local_stop, found) -> bool called after every
      group of half-iterations; True stops the search (sharding.stop_together:
      config 4's ranks stop at the first solution of any of them);
    init_trees, first_half, extend_base: algorithms 3 and 5 — a warm start,
      the continuation of a search: init_trees = (a, b) dicts of v [n][8], act
      [n][10], parent [n] (root first, -1; algorithm 3: parents before
      children; algorithm 5: any tree rooted at 0, since rewiring gives
      vertices later parents), the first half-iteration (its targets are the
      draws a search from the roots makes there; even for algorithm 5) and the
      candidate stream's first extend index; max_halves then counts the
      continuation's halves.
    stage_timing: algorithms 3 / 5 — time every half-iteration's stage groups
      with hipEvents (diagnostics): out["stage_us"] = summed microseconds of
      [the half, stages 0-3, 6, 7 (its own stream), 4-5] over
      out["stage_halves"] halves."""
    L = load()
    x = np.ascontiguousarray(data.x, dtype=np.float64)
    y = np.ascontiguousarray(data.y, dtype=np.float64)
    z = np.ascontiguousarray(data.z, dtype=np.float64)
    slopes = [None if getattr(data, k, None) is None else
              np.ascontiguousarray(getattr(data, k), dtype=np.float64) for k in ("dx", "dy", "dz")]
    p = PlanParams()
    p.device, p.nx, p.ny = device, x.size, y.size
    p.x, p.y, p.z = x.ctypes.data, y.ctypes.data, z.ctypes.data
    p.dx, p.dy, p.dz = [None if s is None else s.ctypes.data for s in slopes]
    p.start[:] = [float(v) for v in start]
    p.goal[:] = [float(v) for v in goal]
    p.batch, p.max_time, p.seed, p.post_process = int(batch), float(max_time), int(seed), int(post_process)
    p.algorithm = int(algorithm)
    p.max_time_opt = float(max_time_opt)
    if sampling is not None:
        p.sampling = sampling
    p.fragile_eps_fm = 0 if fragile_eps is None else int(round(fragile_eps * 1e15))
    p.adaptive = int(bool(adaptive))
    p.nn_stats = int(bool(nn_stats))
    p.stage_timing = int(bool(stage_timing))
    p.max_halves = int(max_halves)
    p.first_half, p.extend_base = int(first_half), int(extend_base)
    warm = []
    if init_trees is not None:
        for k, t in enumerate(init_trees):
            arrs = (np.ascontiguousarray(t["v"], np.float64).reshape(-1, 8),
                    np.ascontiguousarray(t["act"], np.float64).reshape(-1, 10),
                    np.ascontiguousarray(t["parent"], np.int32).reshape(-1))
            warm.append(arrs)
            p.init_n[k] = arrs[0].shape[0]
            p.init_v[k], p.init_a[k], p.init_parent[k] = (x.ctypes.data for x in arrs)
    poll_cb = None
    if stop_poll is not None:
        def _poll(ctx, local, found):
            # fail safe: an exception cannot cross ctypes (it would read as 0 =
            # continue), so a poll that raises answers "stop"
            try:
                return 1 if stop_poll(bool(local), bool(found)) else 0
            except BaseException:  # noqa: BLE001 - reported as stop
                return 1
        poll_cb = StopPoll(_poll)
        p.stop_poll = ctypes.cast(poll_cb, _P)
    tb = []
    if trees:
        p.tree_capacity = int(tree_capacity)
        for k in range(2):
            arrs = dict(v=np.zeros((tree_capacity, 8)), act=np.zeros((tree_capacity, 10)),
                        parent=np.zeros(tree_capacity, np.int32), g=np.zeros(tree_capacity))
            tb.append(arrs)
            p.tree_v[k], p.tree_a[k] = arrs["v"].ctypes.data, arrs["act"].ctypes.data
            p.tree_parent[k], p.tree_g[k] = arrs["parent"].ctypes.data, arrs["g"].ctypes.data
    r = PlanResult()
    states = np.zeros((capacity, 8))
    actions = np.zeros((capacity, 10))
    rc = L.gbp_plan_rrt_connect(ctypes.byref(p), ctypes.byref(r), states.ctypes.data,
                                actions.ctypes.data, capacity)
    del poll_cb, warm
    if rc != 0:
        raise _lib.GbpError(rc, "gbp_plan_rrt_connect")
    out = {k: getattr(r, k) for k, _ in PlanResult._fields_}
    out["extent_a"], out["extent_b"] = list(r.extent_a), list(r.extent_b)
    out["halts"] = list(r.halts)
    out["stage_us"] = list(r.stage_us)
    for name, arrs, nv in zip("ab", tb, (r.vertices_a, r.vertices_b)):
        m = min(int(nv), tree_capacity)
        out[name] = {k: v[:m].copy() for k, v in arrs.items()}
    n = r.n_states
    out["states"] = states[:n].copy()
    out["actions"] = actions[:max(n - 1, 0)].copy()
    return out


def plan_rrt_connect_device(data, start, goal, **kw):
    """buildRRTConnectBatched with the search resident on the device (algorithm 3)."""
    return plan_rrt_connect(data, start, goal, algorithm=3, **kw)


def plan_rrt_star_connect(data, start, goal, device_loop=False, init_shared=None, **kw):
    """RRTStarConnectClass::buildRRTStarConnect, batch-synchronous (algorithm 1;
    algorithm 5 with device_loop: the search resident on the device, the
    insertions' choose-parent / rewire replayed in HBM).

    init_shared ([n][2], with device_loop and init_trees): the warm start also
    takes the earlier run's kept connections (pairs of a vertex of tree a and
    one of tree b, in list order), so the continuation goes on with that list
    and its best instead of starting a new ranking.  The flat C entry's
    parameter record has no room for a list, so this form runs the same device
    search through ReplanSession (the engine's own entries) and returns the
    fields that search produces: found, halves, solutions (carried + new),
    rewires, meet_a / meet_b and path_cost (the best pair and its cost),
    vertices_a / vertices_b, a, b (the trees), shared (the final list), states,
    actions, reported_length, reported_yaw, path_duration.  It takes batch,
    seed, max_time, max_halves, init_trees, first_half, extend_base, adaptive
    and device."""
    if init_shared is None:
        return plan_rrt_connect(data, start, goal, algorithm=5 if device_loop else 1, **kw)
    if not device_loop or kw.get("init_trees") is None:
        raise ValueError("init_shared continues a device search: device_loop=True and init_trees")
    known = {"batch", "seed", "max_time", "max_halves", "init_trees", "first_half", "extend_base",
             "adaptive", "device", "trees"}
    if set(kw) - known:
        raise ValueError(f"not taken with init_shared: {sorted(set(kw) - known)}")
    from . import engine
    own = not isinstance(data, engine.Terrain)
    T = engine.Terrain.from_data(data, device=kw.get("device", 0)) if own else data
    try:
        s = ReplanSession(T, adaptive=kw.get("adaptive", False))
        s.begin(start, goal, batch=kw.get("batch", 64), seed=kw.get("seed", 20251018),
                init_trees=kw["init_trees"], first_half=kw.get("first_half", 0),
                extend_base=kw.get("extend_base", 0), init_shared=init_shared)
        h0 = s.half
        found = s.search(kw.get("max_time", 5.0), kw.get("max_halves", 0))
        st = s.status
        pairs, best, cost = s.shared_connections()
        path = s.best_path()
        a, b = s.dump()
        out = dict(found=int(found), halves=s.half - h0, solutions=len(pairs),
                   rewires=st["stat_rewires"], meet_a=best[0], meet_b=best[1],
                   path_cost=cost if found else 0.0, vertices_a=len(a["parent"]),
                   vertices_b=len(b["parent"]), a=a, b=b, shared=pairs,
                   ext_counter=st["ext_counter"],
                   states=path["states"] if path else np.zeros((0, 8)),
                   actions=path["actions"] if path else np.zeros((0, 10)),
                   reported_length=path["length"] if path else 0.0,
                   reported_yaw=path["yaw"] if path else 0.0,
                   path_duration=path["duration"] if path else 0.0)
        s.end()
        return out
    finally:
        if own:
            T.close()


def plan_rrt_connect_anytime(data, start, goal, max_time_opt=1.0, device_loop=False, **kw):
    """RRTConnectClass::buildRRTConnect's anytime restarts, batch-synchronous
    (algorithm 2; algorithm 4 with device_loop: every restart's search resident
    on the device); `cost_history` is not returned, `solutions` counts the
    restarts that reached the goal."""
    return plan_rrt_connect(data, start, goal, algorithm=4 if device_loop else 2,
                            max_time_opt=max_time_opt, **kw)


def shortcut_paths(terrain_or_data, paths, actions, adaptive=False, cost_add_yaw=False,
                   length_weight=1.0, yaw_weight=1.0, device=0):
    """RRTConnectClass::postProcessPath (rrt_connect.cpp:139-227) for several
    found paths in one call (gbp_shortcut_paths_host): every connect decision
    of every path in one launch, then each path's walk on the host.

    terrain_or_data: an engine.Terrain, or a terrain_data.TerrainData (a
    Terrain is made for the call on `device`); paths: a list of [n_p][8] state
    arrays (n_p >= 2); actions: their [n_p - 1][10] edge actions.
    Returns a dict: `states` / `actions` (lists, one array per path: what the
    walk keeps), `path_length`, `path_yaw`, `path_cost` (arrays [n_paths], the
    reference's path_length_ / path_yaw_ / path_cost_) and `n_resolved` (pairs
    re-decided on the host)."""
    from . import engine
    own = not isinstance(terrain_or_data, engine.Terrain)
    T = engine.Terrain.from_data(terrain_or_data, device=device) if own else terrain_or_data
    try:
        ps = [np.ascontiguousarray(p, np.float64).reshape(-1, 8) for p in paths]
        acs = [np.ascontiguousarray(a, np.float64).reshape(-1, 10) for a in actions]
        if len(ps) != len(acs) or any(a.shape[0] != p.shape[0] - 1 for p, a in zip(ps, acs)):
            raise ValueError("each path of n states takes n - 1 actions")
        n_paths = len(ps)
        off = np.zeros(n_paths + 1, np.int64)
        off[1:] = np.cumsum([p.shape[0] for p in ps])
        total = int(off[-1])
        st = np.concatenate(ps) if ps else np.zeros((0, 8))
        ac = np.concatenate(acs) if acs else np.zeros((0, 10))
        out_off = np.zeros(n_paths + 1, np.int64)
        os_, oa = np.zeros((max(total, 1), 8)), np.zeros((max(total - n_paths, 1), 10))
        ln, yw, co = np.zeros(max(n_paths, 1)), np.zeros(max(n_paths, 1)), np.zeros(max(n_paths, 1))
        nres = ctypes.c_int64(0)
        rc = T._lib.gbp_shortcut_paths_host(
            T._h, n_paths, off.ctypes.data, st.ctypes.data, ac.ctypes.data, int(bool(adaptive)),
            int(bool(cost_add_yaw)), float(length_weight), float(yaw_weight), out_off.ctypes.data,
            os_.ctypes.data, oa.ctypes.data, ln.ctypes.data, yw.ctypes.data, co.ctypes.data,
            ctypes.byref(nres))
        if rc != 0:
            raise _lib.GbpError(rc, "gbp_shortcut_paths_host")
    finally:
        if own:
            T.close()
    return {"states": [os_[out_off[p]:out_off[p + 1]].copy() for p in range(n_paths)],
            "actions": [oa[out_off[p] - p:out_off[p + 1] - p - 1].copy() for p in range(n_paths)],
            "path_length": ln[:n_paths].copy(), "path_yaw": yw[:n_paths].copy(),
            "path_cost": co[:n_paths].copy(), "n_resolved": nres.value}


def revalidate_trees(data, trees, adaptive=False, device=0):
    """The trees of an earlier search against a changed map: what of them a
    new search on `data` (terrain_data.TerrainData, or an engine.Terrain) may
    start from.

    trees: (a, b) dicts of v [n][8], act [n][10], parent [n] — what
    plan_rrt_connect(..., trees=True) returns and init_trees= takes; tree a
    was grown FORWARD, tree b REVERSE.  Each is loaded into HBM and pruned
    there (engine.DeviceTree.revalidate): a vertex stays when every edge
    between it and the root still passes its pair check on the new map.  The
    roots are kept untested.  Returns (pruned_trees, remaps, stats): the
    survivors as (a, b) dicts of v, act, parent, g; per tree the int32 map from
    an old index to the new one (-1: pruned), for callers that carry vertex
    indices of their own across the prune; per tree the stats dict."""
    from . import engine
    own = not isinstance(data, engine.Terrain)
    T = engine.Terrain.from_data(data, device=device) if own else data
    pruned, remaps, stats = [], [], []
    try:
        for direction, t in zip((_lib.FORWARD, _lib.REVERSE), trees):
            v = np.ascontiguousarray(t["v"], np.float64).reshape(-1, 8)
            tree = engine.DeviceTree(v[0], device=T.device, capacity=max(v.shape[0], 1))
            tree.load(v, t["act"], t["parent"])
            remap, st = tree.revalidate(T, direction, adaptive=adaptive)
            s, a, p, g = tree.read()
            pruned.append(dict(v=s, act=a, parent=p, g=g))
            remaps.append(remap)
            stats.append(st)
            del tree
    finally:
        if own:
            T.close()
    return tuple(pruned), tuple(remaps), tuple(stats)


def reroot_tree(tree, vertex, data=None, adaptive=False, device=0):
    """The start tree of an earlier search once the robot stands on one of its
    vertices: what of it the next search, from that state, may start from.

    tree: a dict of v [n][8], act [n][10], parent [n] (tree a of
    plan_rrt_connect(..., trees=True): grown FORWARD).  It is loaded into HBM
    and re-rooted there (engine.DeviceTree.reroot): `vertex` becomes vertex 0
    and the subtree below it follows in ascending old index; everything else
    is unreachable, because the dynamics are not reversible.  With `data`
    (terrain_data.TerrainData, or an engine.Terrain) the map has changed too:
    the edges are tested FORWARD on it and a vertex stays only when every edge
    between it and the new root holds.  Returns (tree, remap, stats): the
    survivors as a dict of v, act, parent and g (derived again from the new
    root), the int32 map from an old index to the new one (-1: dropped), the
    stats dict.  The next search is plan_rrt_connect(data, tree["v"][0], goal,
    init_trees=(tree, b))."""
    from . import engine
    own = data is not None and not isinstance(data, engine.Terrain)
    T = engine.Terrain.from_data(data, device=device) if own else data
    try:
        v = np.ascontiguousarray(tree["v"], np.float64).reshape(-1, 8)
        dt = engine.DeviceTree(v[0], device=device if T is None else T.device,
                               capacity=max(v.shape[0], 1))
        dt.load(v, tree["act"], tree["parent"])
        remap, stats = dt.reroot(vertex, T, _lib.FORWARD, adaptive=adaptive)
        s, a, p, g = dt.read()
        del dt
    finally:
        if own:
            T.close()
    return dict(v=s, act=a, parent=p, g=g), remap, stats


def graft_tree(tree, root, radius, data, direction=_lib.FORWARD, adaptive=False, test_edges=False,
               device=0):
    """A tree of an earlier search once its root has moved to a state that is
    none of its vertices (the robot part of the way through an action or off
    its plan: tree a, FORWARD; a goal that moved: tree b, REVERSE): what of it
    the next search, from `root`, may start from.

    tree: a dict of v [n][8], act [n][10], parent [n].  It is loaded into HBM
    and grafted there (engine.DeviceTree.graft) on `data`
    (terrain_data.TerrainData, or an engine.Terrain): every vertex within
    `radius` that `root` connects to directly becomes a child of `root` by that
    connect action, and a vertex stays when such a vertex lies on its parent
    chain; with test_edges the map has changed too and every edge up to the
    nearest attached vertex must hold on it.  `root` itself is not tested.
    Returns (tree, remap, stats): `root` as vertex 0 and the survivors as a
    dict of v, act, parent and g (derived again), the int32 map from an old
    index to the new one (-1: dropped), the stats dict."""
    from . import engine
    own = not isinstance(data, engine.Terrain)
    T = engine.Terrain.from_data(data, device=device) if own else data
    try:
        v = np.ascontiguousarray(tree["v"], np.float64).reshape(-1, 8)
        dt = engine.DeviceTree(v[0], device=T.device, capacity=v.shape[0] + 1)
        dt.load(v, tree["act"], tree["parent"])
        remap, stats = dt.graft(root, radius, T, direction, adaptive=adaptive, test_edges=test_edges)
        s, a, p, g = dt.read()
        del dt
    finally:
        if own:
            T.close()
    return dict(v=s, act=a, parent=p, g=g), remap, stats


def attempt_connect(terrain, s_existing, s, direction, t_s=None, adaptive=False, s_new=None,
                    a_new=None):
    """RRTConnectClass::attemptConnect (rrt_connect.cpp:20-91) for n pairs on an
    engine Terrain (engine.Terrain).  Returns (result[n], s_new[n][8], a_new[n][10]);
    s_new / a_new start as the given arrays (NaN if None) and are written only
    where the reference writes them."""
    L = load()
    se = np.ascontiguousarray(s_existing, np.float64).reshape(-1, 8)
    sq = np.ascontiguousarray(s, np.float64).reshape(-1, 8)
    n = se.shape[0]
    ts = None if t_s is None else np.ascontiguousarray(t_s, np.float64).reshape(n)
    sn = np.full((n, 8), np.nan) if s_new is None else np.array(s_new, np.float64).reshape(n, 8)
    an = np.full((n, 10), np.nan) if a_new is None else np.array(a_new, np.float64).reshape(n, 10)
    res = np.empty(n, np.int32)
    rc = L.gbp_attempt_connect_batch(terrain._h, n, se.ctypes.data, sq.ctypes.data,
                                     None if ts is None else ts.ctypes.data, int(direction),
                                     int(bool(adaptive)), res.ctypes.data, sn.ctypes.data,
                                     an.ctypes.data)
    if rc != 0:
        raise _lib.GbpError(rc, "gbp_attempt_connect_batch")
    return res, sn, an


# ---- the search kept on the device between plans ------------------------------------
def _yaw_distance(q1, q2):
    """planning_utils::stateYawDistance with glibc's atan2 (math.atan2)."""
    import math
    y1, y2 = math.atan2(q1[4], q1[3]), math.atan2(q2[4], q2[3])
    lo, hi = min(y1, y2), max(y1, y2)
    return min(hi - lo, lo + 2 * math.pi - hi)


class ReplanSession:
    """RRT*-Connect kept alive in HBM between plans: the Python form of the C++
    `ReplanSession` (include/gbp_planner.h), written over the engine's own
    entries (engine.PlanWorkspace / engine.DeviceTree), so it holds the same
    trees, list of kept connections and best as the C++ class and as
    plan_rrt_star_connect(device_loop=True) for the same arguments.

    terrain: an engine.Terrain, which the caller updates in place
    (Terrain.update) before map_changed.  The search is algorithm 5's: target
    streams 401 / 402, groups of half-iterations with one status read each,
    FRAGILE halts re-decided on the host and resumed."""

    def __init__(self, terrain, adaptive=False):
        self.T = terrain
        self.adaptive = bool(adaptive)
        self.ws = None
        self._tree_limit = (0, 0)
        self.trims_by_search = 0
        self._informed = False
        self._informed_set = False   # the session has written the handle's ellipse
        self._roots = None           # the trees' roots as _update_informed last read them

    # -- life cycle ---------------------------------------------------------------
    def begin(self, start, goal, batch=1024, delta=3.0, seed=20251018, init_trees=None,
              first_half=0, extend_base=0, init_shared=None):
        """Sets the search up as buildRRTStarConnectDevice does.  init_trees,
        first_half, extend_base: a warm start as plan_rrt_connect takes it;
        init_shared ([n][2]): the kept connections the continuation starts
        with, loaded and ranked on the device (BatchStats::warm_shared)."""
        from . import engine
        self.end()
        if first_half < 0 or first_half & 1 or extend_base < 0:
            raise ValueError("a warm start of RRT*-Connect begins at an even half")
        self.batch, self.delta, self.seed = int(batch), float(delta), int(seed)
        self.ws = engine.PlanWorkspace(self.T, self.batch)
        self.pairs_cap = max(1 << 18, 8 * self.batch)
        self.ws.star_config(self.delta, self.pairs_cap, 1 << 22)
        cap = max(1 << 16, 4 * self.batch)
        roots = (start, goal)
        self.trees = []
        for k in range(2):
            t = None if init_trees is None else init_trees[k]
            n = 0 if t is None else len(t["parent"])
            dt = engine.DeviceTree(roots[k] if n == 0 else np.asarray(t["v"])[0], device=self.T.device,
                                   capacity=max(cap, 2 * n))
            if n:
                dt.load(t["v"], t["act"], t["parent"])
            self.trees.append(dt)
        self.known = [len(t) for t in self.trees]
        warm = init_trees is not None or first_half > 0
        self.ws.reset(self.T.device, extend_counter=extend_base if warm else 0)
        if init_shared is not None and len(init_shared):
            self.ws.shared_load(self.trees[0], self.trees[1], init_shared, device=self.T.device)
        self.half = int(first_half)
        self.group = 2
        self.g_max = max(2, min(64, (1 << 21) // self.batch)) & ~1
        self.status = self.ws.status(self.T.device)
        self._remap = [None, None]
        self._saved_informed = self.T.get_informed()
        self._roots = None
        self._update_informed()
        return self

    def end(self):
        if self.ws is not None and self._informed_set:
            self.T.set_informed(self._saved_informed)
        self._informed_set = False
        self.ws = None
        self.trees = None

    # -- informed sampling ------------------------------------------------------------
    @property
    def informed(self):
        """Informed sampling, off by default; the object's, like
        the tree limit.  When on, the session keeps the ellipse of (tree a's
        root, tree b's root, the status's best cost, the map's bounds) on the
        terrain handle: computed once per group of halves after the group's
        status read and after map_changed, robot_at, robot_off, goal_at and
        trim; off while no connection is held.  end() puts back what the handle
        held at begin; turning the property off restores it at once."""
        return self._informed

    @informed.setter
    def informed(self, on):
        self._informed = bool(on)
        if self.ws is None:
            return
        if self._informed:
            self._update_informed()
        elif self._informed_set:
            self.T.set_informed(self._saved_informed)
            self._informed_set = False

    @property
    def informed_state(self):
        """The _lib.Informed in force on the terrain handle."""
        self._need()
        return self.T.get_informed()

    def _update_informed(self):
        if not self._informed or self.ws is None:
            return
        st = self.status
        e = _lib.Informed()
        if st["best_a"] >= 0 and st["best_b"] >= 0 and st["best_cost"] < float("inf"):
            if self._roots is None:   # the search never moves a root: read again after upkeep only
                self._roots = [t.read_state(0) for t in self.trees]
            e = _lib.informed_ellipse(self._roots[0], self._roots[1], st["best_cost"],
                                      self.T.info()["bounds"])
        self.T.set_informed(e)
        self._informed_set = True

    @property
    def active(self):
        return self.ws is not None

    def _need(self):
        if self.ws is None:
            raise _lib.GbpError(_lib.E_BAD_HANDLE, "ReplanSession: begin was not called")

    # -- the search ---------------------------------------------------------------
    def _run_group(self):
        T, ws, (ta, tb) = self.T, self.ws, self.trees
        for k, t in enumerate(self.trees):   # room for `group` halves of appends
            c, need = t.capacity(), self.known[k] + self.group * self.batch
            if need > c:
                t.reserve(max(2 * c, need))
        kw = dict(seed=self.seed, stream_a=401, stream_b=402, adaptive=self.adaptive, device=T.device)
        ws.halves(T, ta, tb, self.half, self.group, self.batch, **kw)
        st = ws.status(T.device)
        while st["halt"]:
            h0 = st["halt_half"]
            k = h0 & 1
            if st["halt"] & _lib.PLAN_HALT_STAR_PAIRS:   # a half's neighbour pairs outgrew the sets
                self.pairs_cap = max(2 * self.pairs_cap, st["star_pairs"] + st["star_pairs"] // 4)
                ws.star_config(self.delta, self.pairs_cap, 1 << 22)
            resume, _ = ws.resolve(T, self.trees[k], self.trees[k ^ 1],
                                   _lib.FORWARD if k == 0 else _lib.REVERSE, self.batch,
                                   self.adaptive, T.device)
            if resume < 0:
                raise _lib.GbpError(_lib.E_INVALID_ARG, "plan resolve: nothing halted")
            ws.halves(T, ta, tb, h0, self.half + self.group - h0, self.batch, first_stage=resume, **kw)
            st = ws.status(T.device)
        if st["error"]:
            raise _lib.GbpError(_lib.E_SHAPE, f"device planner loop: status.error {st['error']}")
        self.known = [len(t) for t in self.trees]
        self.half += self.group
        self.status = st

    def search(self, max_time, max_halves=0):
        """Pairs of half-iterations until max_time seconds or max_halves of this
        call; halves and the extend counter go on from the last call.  Returns
        whether a connection is held."""
        import time
        self._need()
        t0, h0 = time.perf_counter(), self.half
        while time.perf_counter() - t0 < max_time and (max_halves <= 0 or
                                                      self.half - h0 + 2 <= max_halves):
            if max_halves > 0:
                self.group = min(self.group, (max_halves - (self.half - h0)) & ~1)
            self._run_group()
            self.group = min(self.group * 2, self.g_max)
            limit, trim_to = self._tree_limit   # the tree limit, once per group
            if limit > 0 and max(self.known) > limit:
                self.trim(trim_to)
                self.trims_by_search += 1
            self._update_informed()   # the next group's targets: inside the best cost's ellipse
        return self.status["best_a"] >= 0

    # -- the trees bounded --------------------------------------------------------------
    @property
    def tree_limit(self):
        """(max_vertices, trim_to): once per group of halves, when either tree
        holds more than max_vertices, search calls trim(trim_to).  (0, 0), the
        default, is off.  Setting it requires 1 <= trim_to <= max_vertices; it
        is the object's and outlives begin and end."""
        return self._tree_limit

    @tree_limit.setter
    def tree_limit(self, value):
        max_vertices, trim_to = (0, 0) if not value else (int(value[0]), int(value[1]))
        if max_vertices < 0 or (max_vertices > 0 and not 1 <= trim_to <= max_vertices):
            raise ValueError("a tree limit needs 1 <= trim_to <= max_vertices")
        self._tree_limit = (max_vertices, trim_to if max_vertices > 0 else 0)

    def trim(self, max_vertices=0):
        """Bounds the trees (engine.DeviceTree.trim): both are
        trimmed in HBM, tree a toward b's root and tree b toward a's, with
        bound = the held best cost (inf when none is held), at most
        max_vertices vertices per tree (0: no budget) and the best
        connection's vertices protected; the list is carried through both
        device remaps and ranked again.  best_path() and the best cost are
        bit-identical before and after.  g falls when a later rewire finds a
        shorter way, so a trimmed vertex might have become useful: the usual
        anytime-RRT* trade, and opt-in.  Returns (trim stats of tree a and b,
        shared stats)."""
        self._need()
        if max_vertices < 0:
            raise ValueError("a negative vertex budget")
        before = list(self.known)
        st = self.status
        held = st["best_a"] >= 0 and st["best_b"] >= 0
        bound = st["best_cost"] if held else float("inf")
        protect = (st["best_a"], st["best_b"]) if held else (-1, -1)
        stats = []
        for k in range(2):
            buf = self._remap_buf(k, before[k])
            stats.append(self.trees[k].trim(self.trees[k ^ 1], bound, max_vertices, protect[k],
                                            remap_dev=buf)[1])
            self.known[k] = stats[k]["n_kept"]
        return tuple(stats), self._carry(self._remap[0], self._remap[1], before)

    # -- the map changed, the robot moved ----------------------------------------------
    def _remap_buf(self, k, n):
        import torch
        if self._remap[k] is None or self._remap[k].numel() < n:
            self._remap[k] = torch.empty(max(n, 1 << 12), dtype=torch.int32,
                                         device=self.T.torch_device)
        return self._remap[k]

    def _carry(self, ra, rb, before):
        st = self.ws.shared_remap(self.trees[0], self.trees[1], ra, rb, before[0], before[1],
                                  device=self.T.device)
        self.status = self.ws.status(self.T.device)
        if st["error"]:
            raise _lib.GbpError(_lib.E_INVALID_ARG, "kept connections: an index outside its tree")
        self._roots = None        # a re-root or a graft moves a root
        self._update_informed()   # ... and the best cost may have changed
        return st

    def map_changed(self):
        """The terrain was updated in place: both trees pruned where they are,
        the list carried through the prunes' device remaps and ranked again.
        Returns (prune stats of tree a and b, shared stats).

        A moved window (engine.Terrain.move) is such an update: the handle is
        the same one, so the session goes on,

            T.move(sx, sy, x_new, y_new, z_new)   # the map scrolled by whole cells
            session.map_changed()                 # prune what left the window
            session.search(...)

        A vertex whose edge now leaves the window reads GBP_F_OOD, is invalid
        and is pruned like any other; the roots are never tested, so keeping
        both inside the new window is the caller's."""
        self._need()
        before = list(self.known)
        stats = []
        for k, direction in enumerate((_lib.FORWARD, _lib.REVERSE)):
            buf = self._remap_buf(k, before[k])
            stats.append(self.trees[k].revalidate(self.T, direction, self.adaptive, remap_dev=buf)[1])
            self.known[k] = stats[k]["n_kept"]
        return tuple(stats), self._carry(self._remap[0], self._remap[1], before)

    def robot_at(self, where, test_edges=False):
        """The robot stands on start-tree vertex `where` (an int), or on a state
        of the current best path ([8] values, matched bit for bit among the
        path's start-tree states; the chain's vertex indices come from the
        parents alone, 4 bytes per vertex of tree a).  Returns (re-root stats,
        shared stats)."""
        self._need()
        if np.ndim(where) == 0:
            vertex = int(where)
        else:
            path = self.best_path()
            if path is None:
                raise _lib.GbpError(_lib.E_INVALID_ARG, "ReplanSession: no path to locate the robot on")
            parent = self.trees[0].read_parents()
            chain = [self.status["best_a"]]
            while chain[-1] != 0 and len(chain) <= len(parent):
                chain.append(int(parent[chain[-1]]))
            chain = chain[::-1]
            s = np.ascontiguousarray(where, np.float64).reshape(8)
            hit = [v for v, row in zip(chain, path["states"][:path["n_from_a"]])
                   if row.tobytes() == s.tobytes()]
            if not hit:
                raise _lib.GbpError(_lib.E_INVALID_ARG,
                                    "ReplanSession: the state is no start-tree vertex of the path")
            vertex = hit[0]
        before = list(self.known)
        buf = self._remap_buf(0, before[0])
        stats = self.trees[0].reroot(vertex, self.T if test_edges else None, _lib.FORWARD,
                                     self.adaptive, remap_dev=buf)[1]
        self.known[0] = stats["n_kept"]
        return stats, self._carry(buf, None, before)

    def _graft(self, k, s, radius, test_edges):
        s = np.ascontiguousarray(s, np.float64).reshape(8)
        # the new root is tested before anything changes: a start in STANCE, a
        # goal in STANCE or in FLIGHT (a goal root may be FLIGHT-valid only)
        phases = (_lib.STANCE,) if k == 0 else (_lib.STANCE, _lib.FLIGHT)
        if not any(self.T.valid_states_host(s[None], ph)[0][0] for ph in phases):
            return None
        before = list(self.known)
        buf = self._remap_buf(k, before[k])
        stats = self.trees[k].graft(s, radius, self.T, _lib.FORWARD if k == 0 else _lib.REVERSE,
                                    self.adaptive, test_edges=test_edges, remap_dev=buf)[1]
        self.known[k] = stats["n_kept"]
        return stats, self._carry(buf if k == 0 else None, buf if k == 1 else None, before)

    def robot_off(self, s, radius, test_edges=False):
        """The robot stands on state `s` ([8] values), which need not be a
        vertex: the start tree is grafted onto it (engine.DeviceTree.graft,
        FORWARD, the vertices within `radius` checked) and the list carried
        through that remap and ranked again.  `s` is tested first (STANCE):
        returns None, with nothing changed, when it fails; else (graft stats,
        shared stats).  With nothing attached the start tree is `s` alone and
        the list empty."""
        self._need()
        return self._graft(0, s, radius, test_edges)

    def goal_at(self, s, radius, test_edges=False):
        """The goal moved to state `s`: robot_off's operation on the goal tree
        (REVERSE); `s` may be valid in STANCE or in FLIGHT."""
        self._need()
        return self._graft(1, s, radius, test_edges)

    # -- what the search holds --------------------------------------------------------
    def best_path(self):
        """The joined path of the best kept connection, extracted on the device
        (neither tree is read): a dict of states, actions, length, yaw, cost,
        duration, n_from_a; None when no connection is held."""
        self._need()
        if self.status["best_a"] < 0 or self.status["best_b"] < 0:
            return None
        s, a, info = self.ws.tree_path(self.trees[0], self.trees[1], device=self.T.device)
        if info["error"]:
            raise _lib.GbpError(_lib.E_SHAPE, "ReplanSession: the trees' parents are no chains")
        if info["n_states"] < 1:
            return None
        na, n = info["n_from_a"], info["n_states"]
        s_ib = self.trees[1].read_state(self.status["best_b"])   # the goal chain's yaw sum ends there
        ya = yb = 0.0
        for i in range(1, na):
            ya = ya + _yaw_distance(s[i - 1], s[i])
        for i in range(n - 1, na, -1):
            yb = yb + _yaw_distance(s[i], s[i - 1])
        if n > na:
            yb = yb + _yaw_distance(s[na], s_ib)
        duration = 0.0
        for row in a:
            duration += row[6] + row[7]
        return dict(states=s, actions=a, length=info["length"], yaw=ya + yb, cost=info["length"],
                    duration=duration, n_from_a=na)

    def dump(self):
        """Both trees read back: (a, b) dicts of v, act, parent, g."""
        self._need()
        return tuple(dict(zip(("v", "act", "parent", "g"), t.read())) for t in self.trees)

    def shared_connections(self):
        """(pairs [n][2] in list order, (best_a, best_b), best_cost)."""
        self._need()
        pairs, ba, bb, bc = self.ws.shared_read(device=self.T.device)
        return pairs, (ba, bb), bc
