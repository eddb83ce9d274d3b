"""Grafting a tree onto a root state that is none of its vertices, restated in
numpy (the expected values of test_tree_graft_ref.py, test_gpu_tree_graft.py
and test_gpu_replan_graft.py).  Nothing here is the engine's: the candidates
are oracle.pose_distance against the radius, an attached vertex is one the
oracle's attemptConnect reaches from the root, the keep rule is a fixed-point
loop, the order is [root] + sorted(kept), g is reroot_ref.derive_g's walk and
the counters are counted."""
import functools

import numpy as np

import oracle
from tests import prune_ref as R
from tests import reroot_ref as RR

FORWARD, REVERSE = R.FORWARD, R.REVERSE
STATS = ("n_before", "n_kept", "n_candidates", "n_checked", "n_attached", "n_outside",
         "n_edge_invalid", "n_inherited", "depth")
V_NOM, KINEMATICS_RES = 0.75, 0.05   # planning_utils.h


def connect_action(s_start, s_goal, t_s):
    """rrt_connect.cpp:53-63, term by term."""
    a = np.zeros(10)
    for k, (q, dq) in enumerate(((0, 3), (1, 4), (2, 5), (6, 7))):
        td, to, dtd, dto = s_start[q], s_goal[q], s_start[dq], s_goal[dq]
        lo = -(2.0 * (3.0 * td - 3.0 * to + 2.0 * dtd * t_s + dto * t_s)) / (t_s * t_s)
        hi = (2.0 * (3.0 * td - 3.0 * to + dtd * t_s + 2.0 * dto * t_s)) / (t_s * t_s)
        if k < 3:
            a[k], a[3 + k] = lo, hi
        else:
            a[8], a[9] = lo, hi
    a[6] = t_s
    return a


def decisions(O, tree, root, radius, direction, adaptive=False):
    """Stage A restated: (candidate bool [n], checked bool [n], attach uint8
    [n], actions [n][10], rows of attached vertices alone) of `root` against
    the vertices of `tree` on O's terrain."""
    v = np.asarray(tree["v"])
    n = len(v)
    root = np.asarray(root, np.float64)
    cand, checked = np.zeros(n, bool), np.zeros(n, bool)
    attach, actions = np.zeros(n, np.uint8), np.zeros((n, 10))
    for j in range(n):
        if not oracle.pose_distance(root, v[j]) <= radius:
            continue
        cand[j] = True
        t_s = oracle.pose_distance(v[j], root) / V_NOM
        if not t_s > KINEMATICS_RES:
            continue
        s_start, s_goal = (root, v[j]) if direction == FORWARD else (v[j], root)
        checked[j] = oracle.is_valid_action(connect_action(s_start, s_goal, t_s))
        res, _, a_new = O.attempt_connect(root, v[j], direction, adaptive=adaptive)
        if res == oracle.REACHED:
            attach[j] = 1
            actions[j] = a_new
    return cand, checked, attach, actions


def under_attached(parent, attach):
    """under[i]: i's parent chain, i included, holds an attached vertex."""
    parent = np.asarray(parent)
    out = np.asarray(attach).astype(bool).copy()
    has = parent >= 0
    while True:
        nxt = out.copy()
        nxt[has] |= out[parent[has]]
        if np.array_equal(nxt, out):
            return out
        out = nxt


def keep_rule(parent, attach, ok=None):
    """keep[i]: i is under an attached vertex and every edge from i up to but
    excluding the nearest one has ok = 1 (an attached vertex's own edge is
    ignored)."""
    parent = np.asarray(parent)
    att = np.asarray(attach).astype(bool)
    keep = under_attached(parent, att)
    if ok is not None:
        keep &= att | np.asarray(ok).astype(bool)
    idx = np.flatnonzero(~att & (parent >= 0))
    while True:
        nxt = keep.copy()
        nxt[idx] &= keep[parent[idx]]
        if np.array_equal(nxt, keep):
            return keep
        keep = nxt


def graft(tree, root, attach, actions, ok=None, n_candidates=0, n_checked=0):
    """(grafted tree with g, remap, stats) of a tree dict (v, act, parent)
    under the decisions attach / actions and edge decisions ok (None: every
    edge holds)."""
    parent = np.asarray(tree["parent"])
    n = len(parent)
    att = np.asarray(attach).astype(bool)
    under = under_attached(parent, att)
    keep = keep_rule(parent, att, ok)
    order = np.array(sorted(int(i) for i in np.flatnonzero(keep)), np.int64)
    remap = np.full(n, -1, np.int32)
    remap[order] = 1 + np.arange(len(order), dtype=np.int32)
    m = 1 + len(order)
    v, act = np.zeros((m, 8)), np.zeros((m, 10))
    v[0] = root
    v[1:] = np.asarray(tree["v"])[order]
    act[1:] = np.where(att[order, None], np.asarray(actions)[order], np.asarray(tree["act"])[order])
    p = np.full(m, -1, np.int32)
    p[1:] = np.where(att[order], 0, remap[np.maximum(parent[order], 0)])
    out = dict(v=v, act=act, parent=p, g=RR.derive_g(v, p))
    depth = np.zeros(m, np.int64)
    while True:
        nxt = depth.copy()
        nxt[1:] = depth[p[1:]] + 1
        if np.array_equal(nxt, depth):
            break
        depth = nxt
    bad = np.zeros(n, bool) if ok is None else ~np.asarray(ok).astype(bool)
    bad &= under & ~att
    stats = dict(n_before=n, n_kept=m, n_candidates=int(n_candidates), n_checked=int(n_checked),
                 n_attached=int(att.sum()), n_outside=int((~under).sum()),
                 n_edge_invalid=int(bad.sum()), n_inherited=int((under & ~keep & ~bad).sum()),
                 depth=int(depth.max()))
    return out, remap, stats


def graft_on(O, tree, root, radius, direction, ok=None, adaptive=False):
    """Both stages restated on O's terrain: (tree, remap, stats, (cand, checked, attach, actions))."""
    oracle.set_scan_mode(1)
    dec = decisions(O, tree, root, radius, direction, adaptive)
    cand, checked, attach, actions = dec
    return graft(tree, root, attach, actions, ok, cand.sum(), checked.sum()) + (dec,)


# ---- the shared inputs: roots off the trees of prune_ref.search("S") -------------------------
def on_ground(O, s, dx, dy):
    """s shifted by (dx, dy), its height above the ground kept."""
    out = np.array(s, np.float64)
    h0, _ = O.ground_height(out[0], out[1])
    out[0] += dx
    out[1] += dy
    h1, _ = O.ground_height(out[0], out[1])
    out[2] += h1 - h0
    return out


def mid_edge(tree, i, direction):
    """The state half way along the stance of the edge into vertex i."""
    v, act, parent = tree["v"], tree["act"], tree["parent"]
    f = oracle.apply_stance if direction == FORWARD else oracle.apply_stance_reverse
    return f(v[parent[i]], act[i], act[i][6] / 2)


# name -> (tree, direction, radius)
CASES = {
    "a-mid5-r3": ("a", FORWARD, 3.0),
    "a-mid5-r1": ("a", FORWARD, 1.0),
    "a-start-shift": ("a", FORWARD, 3.0),
    "b-mid5-r3": ("b", REVERSE, 3.0),
    "b-v30-shift": ("b", REVERSE, 3.0),
    "b-goal-shift": ("b", REVERSE, 3.0),
}


@functools.lru_cache(maxsize=None)
def case_root(case):
    _, O = R.terrain(None)
    r = R.search("S")
    start, goal = R.start_goal()
    if case in ("a-mid5-r3", "a-mid5-r1"):
        return mid_edge(r["a"], 5, FORWARD)
    if case == "a-start-shift":
        return on_ground(O, start, 0.10, 0.05)
    if case == "b-mid5-r3":
        return mid_edge(r["b"], 5, REVERSE)
    if case == "b-v30-shift":
        return on_ground(O, r["b"]["v"][30], 0.05, -0.03)
    if case == "b-goal-shift":
        g = np.array(goal, np.float64)
        g[0] += 0.10
        g[1] += 0.05
        return g
    raise KeyError(case)


@functools.lru_cache(maxsize=None)
def expected(case, box=None, adaptive=False, radius=None):
    """(grafted tree, remap, stats, decisions) of a CASES entry on the terrain
    with `box` (None: unchanged, no edge tested; else the edges are tested on
    it as well)."""
    name, direction, r0 = CASES[case]
    tree = R.search("S")[name]
    _, O = R.terrain(box)
    oracle.set_scan_mode(1)
    ok = R.edge_valid(O, tree, direction, adaptive) if box is not None else None
    return graft_on(O, tree, case_root(case), r0 if radius is None else radius, direction, ok, adaptive)


# ---- the oracle's continuation from a grafted tree ------------------------------------------
# side -> (vertices of a, of b, rewires) after 100 halves from half 300
CONTINUED = {"a": (85, 96, 19), "b": (125, 78, 17)}


@functools.lru_cache(maxsize=None)
def oracle_continues(side, halves=100, first=300):
    """The oracle's RRT*-Connect from the restated graft of one tree of set S
    (side "a": tree a at its mid-edge root with b as it is; side "b": the
    mirror), streams 401 / 402."""
    r = R.search("S")
    _, O = R.terrain(None)
    cfg = R.SETS["S"]
    trees = {"a": r["a"], "b": r["b"]}
    trees[side] = expected(f"{side}-mid5-r3")[0]
    init = tuple({key: trees[t][key] for key in ("v", "act", "parent")} for t in "ab")
    oracle.set_scan_mode(1)
    return O.plan(init[0]["v"][0], init[1]["v"][0], init_trees=init, star=True, nthreads=16,
                  stream_a=401, stream_b=402, batch=cfg["batch"], seed=cfg["seed"], max_halves=halves,
                  first_half=first, extend_base=r["ext_counter"])
