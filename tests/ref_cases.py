"""Inputs of the reference-parity fixture (tests/golden/reference_vectors.npz).

Shared by tools/make_ref_golden.py (which runs the compiled reference on them),
tests/test_reference_parity.py (oracle and host statements against the
recorded results, on the CPU) and tests/test_gpu_reference_parity.py (device
kernels against the same records).  Wherever they exist the inputs are the ones
already in oracle_vectors.npz and shortcut_paths.npz, taken by index, so the
fixture stores only selections, the few inputs made here, and the reference's
recorded outputs.  Nothing in this module needs the reference.

Defined domain: a case whose oracle flags carry GBP_F_OOD or
GBP_F_LIMIT at any level, whose connect would consume an unassigned s_new /
t_new, or which reaches GBP_CONNECT_MAX_DEPTH has no defined reference result;
the generator screens it out with the oracle and never passes it to the
reference.  CAPS bounds the screened share per entry.
"""
import functools
import os

import numpy as np

import oracle
from global_body_planner_amd import _lib as L
from global_body_planner_amd import terrain_data as td
from tests import grid_cases, shortcut_cases
from tests.helpers import attempts_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_vectors.npz")
ORACLE_VECTORS = os.path.join(HERE, "golden", "oracle_vectors.npz")

GOLDEN_TERRAINS = ["slope-gridmap", "rough_terrain-gridmap", "synth-rough-256"]
GRID_PAIR = ("graded", "twostep", "ripple")      # non-uniform: the reference's linear scan
GRID_TERRAIN = "grid-" + grid_cases.terrain_id(GRID_PAIR)
TERRAINS = GOLDEN_TERRAINS + [GRID_TERRAIN]
TREE_TERRAIN = "synth-rough-256"

UNDEFINED = np.uint32(L.F_OOD | L.F_LIMIT)
# the probes' "never assigned" patterns (tests/native/closed_forms_probe.cpp)
S_UNSET = np.frombuffer(b"\x55" * 8, np.float64)[0]
T_UNSET = -7.0

N_LOOKUP, N_STATES, N_PAIRS, N_CONNECT, N_FORMS = 400, 400, 400, 160, 160
CAPS = {"lookups": 0.10, "valid_states": 0.15, "pairs": 0.03, "connects": 0.05,
        "replays": 0.0, "post_process": 0.0}
TREE_SIZES = [12, 13, 14, 128, 257, 600]
N_QUERIES, NBR_RADIUS, KNN_K = 32, 2.0, 8
YAW_WEIGHTS = (1.0, 0.5)
REHASH = [13, 29, 59, 127, 257, 541]       # sizes at which the vertex map rehashes
STAR_DELTA = 3.0
KINEMATICS_RES = 0.05
NAN_CELLS = [(20, 30), (70, 10), (5, 90), (100, 100), (33, 64), (64, 33)]


@functools.lru_cache(maxsize=None)
def oracle_vectors():
    with np.load(ORACLE_VECTORS) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def terrain(name):
    """(TerrainData, OracleTerrain)."""
    if name != GRID_TERRAIN:
        data = td.by_name(name)
    else:   # the grid case with NaN cells: single ones and a block
        base = grid_cases.terrain(*GRID_PAIR)
        z = base.z.copy()
        for ix, iy in NAN_CELLS:
            z[ix, iy] = np.nan
        z[40:43, 50:53] = np.nan
        data = td.TerrainData(base.x.copy(), base.y.copy(), z, base.dx, base.dy, base.dz,
                              name=GRID_TERRAIN)
    return data, oracle.OracleTerrain.from_data(data)


@functools.lru_cache(maxsize=None)
def base_inputs(name):
    """xy, states, pair_s / pair_a / pair_dir of a terrain: oracle_vectors.npz's
    own for the golden terrains (the first rows, and for xy the points on grid
    lines and the corners too), the oracle's samplers for the grid terrain."""
    data, O = terrain(name)
    if name != GRID_TERRAIN:
        g = oracle_vectors()
        xy = g[name + "/xy"]
        n = xy.shape[0]
        sel = np.r_[0:N_LOOKUP - 104, 2000:min(2100, n - 4), n - 4:n]
        return _with_pair_extras(O, dict(
            xy=xy[sel], xy_sel=sel, states=g[name + "/states"][:N_STATES], pool=g[name + "/states"],
            pair_s=g[name + "/pair_s"][:N_PAIRS], pair_a=g[name + "/pair_a"][:N_PAIRS],
            pair_dir=g[name + "/pair_dir"][:N_PAIRS]))
    xy = grid_cases.lookup_points(data, seed=1, n_random=N_LOOKUP - 100, n_lines=20)
    # the four cells around every NaN grid point, and points on its grid lines
    around = [((data.x[ix + i] + data.x[ix + i + 1]) / 2, (data.y[iy + j] + data.y[iy + j + 1]) / 2)
              for ix, iy in NAN_CELLS + [(41, 51)] for i in (-1, 0) for j in (-1, 0)]
    around += [(data.x[ix], (data.y[iy] + data.y[iy + 1]) / 2) for ix, iy in NAN_CELLS]
    xy = np.concatenate([np.array(around), xy])
    pool, _ = O.sample_states(1500, 77, 5, 0)
    s, a, d, _, _ = attempts_oracle(O, N_PAIRS, seed=grid_cases.pair_seed(GRID_PAIR), nthreads=4)
    return _with_pair_extras(O, dict(xy=xy[:N_LOOKUP + 200], xy_sel=None, states=pool[:N_STATES],
                                     pool=pool, pair_s=s, pair_a=a, pair_dir=d))


# flight times at which the adaptive loops' t (0.05, then + 0.10, + 0.15) lands
# exactly on t_f, and no flight phase at all
GRID_FLIGHT_TIMES = [0.0, 0.05, 0.05 + 0.1, 0.05 + 0.1 + 0.15]
N_PAIR_EXTRAS = 96


def _with_pair_extras(O, b):
    """Appends pairs the samplers never draw: the golden actions with t_f on
    the adaptive step's own grid or zero, from states the oracle finds
    STANCE-invalid (first half) and STANCE-valid (second half) with every
    lookup inside the map.  There `t < t_f` against `t <= t_f` decides whether
    the end state itself gets a FLIGHT check, and with it whether a failing
    reverse check assigns s_new."""
    v, f, _ = O.valid_states(b["pool"], L.STANCE)
    inside = (f & UNDEFINED) == 0
    half = N_PAIR_EXTRAS // 2
    rows = np.concatenate([np.flatnonzero(inside & (v == 0))[:half],
                           np.flatnonzero(inside & (v != 0))[:half]])
    k = np.arange(rows.size)
    a = b["pair_a"][:rows.size].copy()
    a[:, 7] = np.array(GRID_FLIGHT_TIMES)[(k // 2) % 4]
    b["pair_s"] = np.concatenate([b["pair_s"], b["pool"][rows]])
    b["pair_a"] = np.concatenate([b["pair_a"], a])
    b["pair_dir"] = np.concatenate([b["pair_dir"], (k % 2).astype(np.uint8)])
    return b


def lookup_screen(name):
    """True where the oracle reports an out-of-domain lookup."""
    _, O = terrain(name)
    xy = base_inputs(name)["xy"]
    _, _, ood = O.height_batch(xy)
    _, nood = O.normal_batch(xy)
    return (ood != 0) | (nood != 0)


def state_screen(name, phase):
    _, O = terrain(name)
    _, f, _ = O.valid_states(base_inputs(name)["states"], phase)
    return (f & UNDEFINED) != 0


def pair_screen(name, adaptive):
    _, O = terrain(name)
    b = base_inputs(name)
    _, _, _, f, _ = O.validate_pairs(b["pair_s"], b["pair_a"], b["pair_dir"], adaptive=adaptive)
    return (f & UNDEFINED) != 0


def connect_candidates(name):
    """(e_idx, s_idx) into the pool: end states the oracle finds STANCE-valid
    with every lookup inside the map, half of the pairs far apart (stride
    through the valid states), half the 1st..5th nearest valid state by pose, so
    short connects, one-level and many-level recursions all occur.  Row k runs
    direction k & 1, adaptive (k >> 1) & 1 (the closed-forms probe's rule)."""
    _, O = terrain(name)
    pool = base_inputs(name)["pool"]
    v, f, _ = O.valid_states(pool, L.STANCE)
    ok = np.flatnonzero((v != 0) & ((f & UNDEFINED) == 0))
    e = ok[:N_CONNECT]
    s = np.empty_like(e)
    P = pool[ok][:, :3]
    for k in range(e.size):
        if k % 2 == 0:
            s[k] = ok[(k * 7 + 11) % ok.size]
            if s[k] == e[k]:
                s[k] = ok[(k * 7 + 12) % ok.size]
        else:
            d = np.linalg.norm(P - P[k], axis=1)
            s[k] = ok[np.argsort(d, kind="stable")[1 + (k // 2) % 5]]
    return e, s


def connect_undefined(O, e, s, direction, adaptive, t_s=0.0):
    r, _, _, flags, undef, _ = O.attempt_connect_info(e, s, direction, t_s=t_s, adaptive=adaptive)
    return bool(np.uint32(flags) & UNDEFINED) or undef != 0


def ts_cases():
    """t_s of the three-argument overload around KINEMATICS_RES."""
    k = KINEMATICS_RES
    return np.array([k, np.nextafter(k, 1.0), np.nextafter(k, 0.0), k + 1e-9, 0.06, 0.1, 0.3, 1.0])


def form_inputs():
    """Closed-form rows: s, s2, a, t from synth-rough-256's golden pairs and
    states; t sweeps 0 .. the stance time and beyond; some s2 sit at, just
    inside and just outside GOAL_BOUNDS of s along x (binary-exact offsets)."""
    g = oracle_vectors()
    p = TREE_TERRAIN + "/"
    s = g[p + "pair_s"][1000:1000 + N_FORMS].copy()
    a = g[p + "pair_a"][1000:1000 + N_FORMS].copy()
    s2 = g[p + "states"][1000:1000 + N_FORMS].copy()
    t = a[:, 6] * (np.arange(N_FORMS) % 9) / 6.0
    for k, off in zip(range(0, 40, 4), [0.5, 0.25, 0.75, 0.5, 0.0, 0.5, 0.125, 1.0, 0.5, 0.375]):
        s[k, 0] = 1.0 + k / 64.0
        s2[k] = s[k]
        s2[k, k % 3] = s[k, k % 3] + off
    return s, s2, a, t


def tree_vertices():
    """600 STANCE-valid states of synth-rough-256's golden pool, vertex 0 the
    root; parents and edge actions are arbitrary but fixed (the neighbour
    searches and path walks do not test the edges)."""
    _, O = terrain(TREE_TERRAIN)
    g = oracle_vectors()
    pool = g[TREE_TERRAIN + "/states"]
    v, f, _ = O.valid_states(pool, L.STANCE)
    ok = np.flatnonzero((v != 0) & ((f & UNDEFINED) == 0))
    sel = ok[:max(TREE_SIZES)]
    n = sel.size
    parent = np.full(n, -1, np.int32)
    for i in range(1, n):
        parent[i] = (i * 2654435761 >> 7) % i if i % 3 else i - 1
    act = g[TREE_TERRAIN + "/pair_a"][:n].copy()
    act[0] = 0.0
    queries = pool[ok[-N_QUERIES:]]
    return pool[sel], parent, act, queries


ROOT_CONNECT_CONFIGS = [(0, 0), (1, 0), (0, 1), (1, 1)]     # (direction, adaptive)


@functools.lru_cache(maxsize=None)
def graft_vertices():
    """(root, vertices [600][8]) of the graft check on synth-rough-256: the
    states of its found and densified paths (a fair share of them connect
    directly), filled up with tree_vertices(); the root is the middle state of
    the longest found path, which is left out of the vertices."""
    found = [shortcut_cases.found_path(c, b, s, ad)[0] for c, b, s in shortcut_cases.FOUND
             if c == shortcut_cases.SYNTH for ad in (False, True)]
    c, b, s, k = shortcut_cases.DENSE[0]
    assert c == shortcut_cases.SYNTH
    long = max(found, key=len)
    root = long[len(long) // 2]
    v = np.concatenate(found + [shortcut_cases.dense_path(c, b, s, k)[0]])
    v = v[~(v == root).all(axis=1)]
    _, first = np.unique(v, axis=0, return_index=True)
    v = v[np.sort(first)]
    v = np.concatenate([v, tree_vertices()[0]])[:600]
    return root, v


def graft_screen(direction, adaptive):
    """True where attemptConnect(root, vertex) leaves the defined domain."""
    _, O = terrain(TREE_TERRAIN)
    root, verts = graft_vertices()
    return np.array([connect_undefined(O, root, v, direction, adaptive) for v in verts])


def no_exact_ties(verts, queries):
    """No query sees two vertices at the same fp64 state distance (H9: ties
    are the one documented deviation of the device searches) nor at the same
    yaw-weighted key."""
    for q in queries:
        d = np.array([oracle.state_distance(q, v) for v in verts])
        w = np.array([oracle.state_distance_yaw(q, v, *YAW_WEIGHTS) for v in verts])
        if np.unique(d).size != d.size or np.unique(w).size != w.size:
            return False
    return True


# slope seed 2's plain path has one pair (4, 25) whose connect meets an
# out-of-domain lookup two levels down: no defined reference result, so the
# path (and its densified form) is no input here
PATHS_OUTSIDE_DOMAIN = {(shortcut_cases.SLOPE, 256, 2, False)}


def path_cases():
    """(key, terrain name, states, actions, adaptive): every found path of
    shortcut_paths.npz, walked with the step rule it was found with and the
    other one; then the two densified paths (about 106 states, marker actions:
    their walk takes the fallback branch), plain."""
    out = []
    for case, batch, seed in shortcut_cases.FOUND:
        for found_adaptive in (False, True):
            if (case, batch, seed, found_adaptive) in PATHS_OUTSIDE_DOMAIN:
                continue
            S, A = shortcut_cases.found_path(case, batch, seed, found_adaptive)
            for adaptive in (False, True):
                key = shortcut_cases.path_key(case, batch, seed, found_adaptive) + f"_w{int(adaptive)}"
                out.append((key, case[0], S, A, adaptive))
    for case, batch, seed, k in shortcut_cases.DENSE:
        if (case, batch, seed, False) in PATHS_OUTSIDE_DOMAIN:
            continue
        S, A = shortcut_cases.dense_path(case, batch, seed, k)
        out.append((f"{case[0]}_dense{k}_w0", case[0], S, A, False))
    return out


REPLAY_INSERTIONS = 4
REPLAY_BOX = (1.0, 4.1)


@functools.lru_cache(maxsize=None)
def replay_vertices():
    """The replay trees' vertices: STANCE-valid golden states at least 1 m from
    the map's edge, where no connect between two of them meets an out-of-domain
    lookup (RRT*'s delta of 3 m makes nearly every vertex a neighbour, and one
    undefined connect would take the whole insertion out of the domain)."""
    _, O = terrain(TREE_TERRAIN)
    pool = oracle_vectors()[TREE_TERRAIN + "/states"]
    v, f, _ = O.valid_states(pool, L.STANCE)
    lo, hi = REPLAY_BOX
    inside = (pool[:, :2] > lo).all(axis=1) & (pool[:, :2] < hi).all(axis=1)
    return pool[(v != 0) & ((f & UNDEFINED) == 0) & inside]


def replay_parents(n0):
    """Every vertex under its nearest earlier vertex by pose."""
    verts = replay_vertices()
    parent = np.full(n0, -1, np.int32)
    for i in range(1, n0):
        parent[i] = int(np.argmin(np.linalg.norm(verts[:i, :3] - verts[i, :3], axis=1)))
    return parent


REPLAY_TARGETS = 400000


def interp_path_cases(fx):
    """(key, states, actions, dt) for getInterpPath: found paths as the search
    left them (stance and flight phases, t_f > 0), and what postProcessPath
    keeps of them as recorded in the fixture (connect actions, t_f == 0: the
    CONNECT_STANCE phase), at the reference's dt and at one that divides no
    stance time.  fx: the fixture (its pp/ records are inputs here)."""
    out = []
    for (case, batch, seed), ad, dt in [((shortcut_cases.SYNTH, 64, 11), False, 0.05),
                                        ((shortcut_cases.SYNTH, 64, 3), True, 0.03),
                                        ((shortcut_cases.SYNTH, 1, 11), True, 0.05)]:
        S, A = shortcut_cases.found_path(case, batch, seed, ad)
        key = shortcut_cases.path_key(case, batch, seed, ad)
        out.append((key + "_found", S, A, dt))
        p = "pp/" + key + "_w0/"
        out.append((key + "_kept", fx[p + "states"], fx[p + "actions"], 2 * dt))
    return out


def replay_trees():
    """(key, direction, adaptive, star, n0, target stream): a tree of the first
    n0 replay_vertices() is built, then extended toward replay_targets(stream)
    in turn until REPLAY_INSERTIONS calls have inserted a vertex (most calls
    are TRAPPED, as in the reference's own search).  The n0 sit two below each
    rehash size so the insertions cross it."""
    out = [(f"star{r}", i % 2, (i // 2) % 2, 1, r - 2, 900 + i) for i, r in enumerate(REHASH)]
    return out + [("rrt13", 0, 0, 0, 11, 950), ("rrt29", 1, 1, 0, 27, 951)]


def replay_targets(stream):
    """The generator's extend targets: the oracle's sampler, kept where the
    target lies half a metre further inside the map than the vertices."""
    _, O = terrain(TREE_TERRAIN)
    t = O.sample_states(REPLAY_TARGETS, 20251021, stream, 0, nthreads=4)[0]
    lo, hi = REPLAY_BOX
    return t[(t[:, :2] > lo + 0.5).all(axis=1) & (t[:, :2] < hi - 0.5).all(axis=1)]


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}
