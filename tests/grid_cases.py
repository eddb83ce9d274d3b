"""Non-uniform terrain grids: named coordinate vectors, the terrains built from
them, and numpy restatements of the engine's bracket search and of the host
analysis that picks the device code (gbp_terrain_create: one_step_exact,
affine_fit).  Shared by test_grid_cases.py (CPU) and test_gpu_grid_parity.py.

The engine brackets a coordinate v in an ascending vector d (first i with
d[i] <= v < d[i+1]) from a guess (int)((v - d[0]) * inv), inv = 1 / mean
spacing, clamped to [0, n-2], and then either
  * one correction step (exact when one_step_exact holds: uniform spacing up
    to rounding, grid_map geometry), or
  * the general search: walk down while v < d[i], then up while v >= d[i+1]
    (any ascending vector, repeated coordinates = empty cells included).
The restatements below use the same IEEE double operations in numpy.
"""
import functools

import numpy as np

from global_body_planner_amd import terrain_data as td

BR_LOW, BR_HIGH = -1, -2   # no bracket: NaN or v < d[0]; v >= d[n-1]


# ---- the named vectors ------------------------------------------------------------
def _uniform():
    return np.arange(128, dtype=np.float64) * 0.04


def _jitter():
    d = _uniform()
    d[1:-1] += np.random.default_rng(20251020).uniform(-0.015, 0.015, d.size - 2)
    return d


def _offset():
    return -1000.0 + np.arange(128, dtype=np.float64) * 0.04


def _graded():
    return np.concatenate([[0.0], np.cumsum(0.01 * 1.03 ** np.arange(127, dtype=np.float64))])


def _twostep():
    fine = np.arange(64, dtype=np.float64) * 0.02
    return np.concatenate([fine, fine[-1] + np.arange(1, 65, dtype=np.float64) * 0.06])


def _dups():
    d = _uniform()
    return np.sort(np.concatenate([d, [d[0], d[40], d[40], d[-1]]]))


def _two():
    return np.array([0.0, 5.08])


VECTORS = {"uniform": _uniform(), "jitter": _jitter(), "offset": _offset(), "graded": _graded(),
           "twostep": _twostep(), "dups": _dups(), "two": _two()}
for _v in VECTORS.values():
    _v.setflags(write=False)

# name -> (one-step correction exact, bit-for-bit affine): what the host analysis
# is expected to find (asserted against the restatements in test_grid_cases.py)
CLASSES = {"uniform": (1, True), "jitter": (1, False), "offset": (1, False), "graded": (0, False),
           "twostep": (0, False), "dups": (0, False), "two": (1, True)}

# (x vector, y vector[, "ripple"]): the tiny shapes (n - 2 == 0 clamps), then
# the rippled heights (see terrain())
TERRAINS = [("graded", "graded"), ("graded", "uniform"), ("uniform", "twostep"), ("dups", "jitter"),
            ("jitter", "jitter"), ("offset", "uniform"), ("graded", "twostep"), ("dups", "uniform"),
            ("uniform", "uniform"), ("two", "dups"), ("dups", "two"), ("two", "two"),
            ("graded", "twostep", "ripple"), ("twostep", "graded", "ripple"),
            ("dups", "jitter", "ripple")]


def terrain_id(pair):
    return f"{pair[0]}x{pair[1]}" + ("-ripple" if len(pair) > 2 and pair[2] else "")


# the validate-pairs batch of a terrain: helpers.attempts_oracle(O, N_PAIRS, pair_seed(pair)).
# A terrain whose batch has more near-line (FRAGILE) attempts than the bar
# N_PAIRS * 1e-3 gets another seed here (checked on the CPU, test_grid_cases.py)
N_PAIRS = 8192
_PAIR_SEEDS = {}


def pair_seed(pair):
    return _PAIR_SEEDS.get(tuple(pair), 500 + TERRAINS.index(tuple(pair)))


@functools.lru_cache(maxsize=None)
def terrain(xname, yname, ripple=None):
    """TerrainData on the named vectors; heights and slope layers are
    synth_rough(max(nx, ny))'s, cut to [nx, ny]: indexed by cell, whatever the
    spacing.  synth_rough is flat over blocks of 10 x 10 cells, so a bracket
    that is one cell off mostly finds the same heights and a state check
    decides the same; with `ripple` every height is moved by a seeded
    U(-3 cm, 3 cm) (float-rounded), so the neighbouring cell gives another
    height and, near a threshold, another decision."""
    x, y = VECTORS[xname], VECTORS[yname]
    base = td.synth_rough(max(x.size, y.size))
    cut = lambda a: np.ascontiguousarray(a[:x.size, :y.size])
    z = cut(base.z)
    if ripple:
        z = z + np.random.default_rng(7).uniform(-0.03, 0.03, z.shape)
        z = z.astype(np.float32).astype(np.float64)
    return td.TerrainData(x.copy(), y.copy(), z, cut(base.dx), cut(base.dy), cut(base.dz),
                          name=terrain_id((xname, yname, ripple)))


# ---- the bracket, restated ----------------------------------------------------------
def inv_spacing(d):
    """gbp_terrain_create's inv_hx / inv_hy."""
    return float(d.size - 1) / (d[-1] - d[0]) if d[-1] > d[0] else 0.0


def bracket_guess(d, v, inv=None):
    """(int)((v - d[0]) * inv) clamped to [0, n-2], for finite v in the domain."""
    inv = inv_spacing(d) if inv is None else inv
    i = np.trunc((np.asarray(v, np.float64) - d[0]) * inv)
    return np.clip(i, 0, d.size - 2).astype(np.int64)


def _codes(d, v):
    """(in domain, code for the others)"""
    inside = (v >= d[0]) & (v < d[-1])          # False for NaN
    return inside, np.where(v >= d[-1], BR_HIGH, BR_LOW)


def bracket_one_step(d, v):
    """The guess plus one correction step; BR_LOW / BR_HIGH outside."""
    v = np.asarray(v, np.float64)
    inside, out = _codes(d, v)
    vi = v[inside]
    i = bracket_guess(d, vi)
    i = i + (vi >= d[i + 1]).astype(np.int64) - (vi < d[i]).astype(np.int64)
    out[inside] = i
    return out


def bracket_general(d, v):
    """The guess, the walk down, then the walk up; BR_LOW / BR_HIGH outside."""
    v = np.asarray(v, np.float64)
    n = d.size
    inside, out = _codes(d, v)
    vi = v[inside]
    i = bracket_guess(d, vi)
    while True:
        m = (i > 0) & (vi < d[i])
        if not m.any():
            break
        i[m] -= 1
    while True:
        m = (i < n - 2) & (vi >= d[np.minimum(i + 1, n - 1)])
        if not m.any():
            break
        i[m] += 1
    out[inside] = i
    return out


def bracket_expected(d, v):
    """The reference's scan by definition: the last i with d[i] <= v, for
    d[0] <= v < d[n-1]."""
    v = np.asarray(v, np.float64)
    inside, out = _codes(d, v)
    out[inside] = np.searchsorted(d, v[inside], side="right") - 1
    return out


# ---- the host analysis, restated ------------------------------------------------------
def one_step_exact(d):
    """1 when the guess is within one cell of the bracket at both ends of every
    cell (the guess is monotone in v), 0 otherwise or with an empty cell."""
    n, inv = d.size, inv_spacing(d)
    if not (inv > 0 and np.isfinite(inv)):
        return 0
    if not np.all(d[:-1] < d[1:]):
        return 0
    i = np.arange(n - 1)
    lo = bracket_guess(d, d[:-1], inv)
    hi = bracket_guess(d, np.nextafter(d[1:], -np.inf), inv)
    return int(not (np.any(lo < i - 1) or np.any(hi > i + 1)))


def affine_fit(d):
    """Is d[i] == a + h * (i - base) bit for bit, base 0 or n-1, h within 4 ulps
    of the mean, first or last spacing?  -> (a, h, base) or None."""
    n = d.size
    if n < 2:
        return None
    cands = ((d[-1] - d[0]) / float(n - 1), d[1] - d[0], d[-1] - d[-2])
    for base in (0, n - 1):
        a = d[base]
        k = (np.arange(n) - base).astype(np.float64)
        for c in cands:
            if not (c > 0 and np.isfinite(c)):
                continue
            h = c
            for _ in range(4):
                h = np.nextafter(h, -np.inf)
            for _ in range(9):
                if np.array_equal((a + h * k).view(np.uint64), d.view(np.uint64)):
                    return float(a), float(h), base
                h = np.nextafter(h, np.inf)
    return None


def predicted(pair):
    """(one_x, one_y, affine on both axes) of a terrain, from the restatements."""
    x, y = VECTORS[pair[0]], VECTORS[pair[1]]
    return (one_step_exact(x), one_step_exact(y),
            affine_fit(x) is not None and affine_fit(y) is not None)


# ---- query points -----------------------------------------------------------------------
def axis_queries(d, seed=0, n_random=10000):
    """Every grid line, nextafter on both sides of it, seeded random points in
    the span, both ends, NaN."""
    rng = np.random.default_rng(seed)
    return np.concatenate([d, np.nextafter(d, -np.inf), np.nextafter(d, np.inf),
                           rng.uniform(d[0], d[-1], n_random), [d[0], d[-1]], [np.nan]])


def lookup_points(data, seed=1, n_random=20000, n_lines=500):
    """test_height_and_normal_parity's points on `data`: random with a 0.3 m
    margin outside the map, grid lines, +-1 ulp around them, the four corners;
    plus every point on and beside a repeated line of either axis."""
    rng = np.random.default_rng(seed)
    x0, xN, y0, yN = data.bounds
    xy = np.stack([rng.uniform(x0 - 0.3, xN + 0.3, n_random),
                   rng.uniform(y0 - 0.3, yN + 0.3, n_random)], 1)
    gx = data.x[rng.integers(0, data.x.size, n_lines)]
    gy = data.y[rng.integers(0, data.y.size, n_lines)]
    parts = [xy, np.stack([gx, gy], 1), np.stack([np.nextafter(gx, -np.inf), gy], 1),
             np.stack([np.nextafter(gx, np.inf), np.nextafter(gy, np.inf)], 1),
             np.array([[xN, y0], [x0, yN], [xN, yN], [x0, y0]])]

    def beside(d):
        r = np.unique(d[:-1][d[:-1] == d[1:]])
        return np.concatenate([r, np.nextafter(r, -np.inf), np.nextafter(r, np.inf)])

    rx, ry = beside(data.x), beside(data.y)
    if rx.size:
        oy = rng.uniform(y0, yN, rx.size)
        parts += [np.stack([rx, oy], 1), np.stack([rx, gy[:rx.size]], 1)]
    if ry.size:
        ox = rng.uniform(x0, xN, ry.size)
        parts += [np.stack([ox, ry], 1), np.stack([gx[:ry.size], ry], 1)]
    if rx.size and ry.size:
        parts.append(np.stack(np.meshgrid(rx, ry, indexing="ij"), -1).reshape(-1, 2))
    return np.concatenate(parts)
