"""The bracket search on non-uniform grids, on the CPU: the numpy restatements
in tests/grid_cases.py against the bracket's definition
(searchsorted(d, v, 'right') - 1), the class the host analysis is expected to
give every named vector, and the oracle's two scan modes on every terrain of
test_gpu_grid_parity.py.

What the `ONE` kernels rest on: where one_step_exact says 1, guess + one
correction is the bracket for EVERY v.  Where it says 0 the general search
(walk down, then up) must be, empty cells included.
"""
import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from tests import grid_cases as G
from tests.helpers import attempts_oracle, same_f64

NAMES = list(G.VECTORS)
IDS = [G.terrain_id(p) for p in G.TERRAINS]


@pytest.fixture(autouse=True)
def _linear_scan_after():
    yield
    oracle.set_scan_mode(0)


@pytest.mark.parametrize("name", NAMES)
def test_named_vector_lands_in_its_class(name):
    d = G.VECTORS[name]
    one, affine = G.CLASSES[name]
    assert np.all(d[:-1] <= d[1:])
    assert G.one_step_exact(d) == one
    assert (G.affine_fit(d) is not None) == affine
    if name != "two":
        assert d.size == (132 if name == "dups" else 128)
        assert 5.0 <= d[-1] - d[0] <= 14.0
    if name == "jitter":
        assert np.unique(np.diff(d)).size == 127
    if name == "dups":   # empty cells at both ends and inside (one of them two cells wide)
        empty = np.flatnonzero(d[:-1] == d[1:])
        assert list(empty) == [0, 41, 42, 130]


def test_affine_fit_reproduces_the_vector():
    for name in NAMES:
        d = G.VECTORS[name]
        fit = G.affine_fit(d)
        if fit is not None:
            a, h, base = fit
            assert np.array_equal(a + h * (np.arange(d.size) - base).astype(np.float64), d)
    # grid_map's reversed cell centres: affine from the last line
    rev = (5.0 + 0.02 * -np.arange(200, dtype=np.float64))[::-1].copy()
    assert G.affine_fit(rev) is not None and G.one_step_exact(rev) == 1


@pytest.mark.parametrize("name", NAMES)
def test_bracket_restatements_equal_the_definition(name):
    d = G.VECTORS[name]
    v = G.axis_queries(d, seed=NAMES.index(name))
    want = G.bracket_expected(d, v)
    assert want[-1] == G.BR_LOW and want[-2] == G.BR_HIGH and want[-3] == 0 + int(d[0] == d[1])
    inside = want >= 0
    assert np.all(d[want[inside]] <= v[inside]) and np.all(v[inside] < d[want[inside] + 1])
    # the general search is the bracket on any ascending vector
    got = G.bracket_general(d, v)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    if G.one_step_exact(d):
        got = G.bracket_one_step(d, v)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    elif name in ("graded", "twostep"):
        # and these vectors need it: one correction step is not enough
        assert not np.array_equal(G.bracket_one_step(d, v), want)


@pytest.mark.parametrize("pair", G.TERRAINS, ids=IDS)
def test_terrain_classes(pair):
    ox, oy, affine = G.predicted(pair)
    assert (ox, oy) == (G.CLASSES[pair[0]][0], G.CLASSES[pair[1]][0])
    assert affine == (G.CLASSES[pair[0]][1] and G.CLASSES[pair[1]][1])
    data = G.terrain(*pair)
    assert data.z.shape == (data.x.size, data.y.size) == data.dx.shape
    assert max(data.z.shape) <= 132
    assert np.array_equal(data.z.astype(np.float32).astype(np.float64), data.z)  # fp32 storage


@pytest.mark.parametrize("pair", G.TERRAINS, ids=IDS)
def test_oracle_scan_modes_agree(pair):
    """Linear scan (the reference's loop) and bisection give the same brackets:
    same heights, normals, NaN / out-of-domain marks, pair results and flags."""
    data = G.terrain(*pair)
    O = oracle.OracleTerrain.from_data(data)
    xy = G.lookup_points(data, n_random=5000)
    oracle.set_scan_mode(1)
    s, a, d, _, _ = attempts_oracle(O, 2048, seed=G.pair_seed(pair))
    st, _ = O.sample_states(4000, 11, 7, 0, -1, 1, nthreads=8)
    outs = []
    for mode in (0, 1):
        oracle.set_scan_mode(mode)
        h, nan, ood = O.height_batch(xy, nthreads=8)
        nrm, nood = O.normal_batch(xy, nthreads=8)
        pairs = O.validate_pairs(s, a, d, nthreads=8)
        states = O.valid_states(st, L.STANCE, nthreads=8)
        outs.append((h, nan, ood, nrm, nood) + tuple(pairs) + tuple(states))
    for p, q in zip(*outs):
        if p.dtype == np.float64:
            assert np.all(same_f64(p, q))
        else:
            assert np.array_equal(p, q)
    h, nan, ood = outs[0][:3]
    assert ood.sum() > 0 and (ood == 0).sum() > 0.5 * len(ood)
    # heights against the restated bracket + the bilinear blend in numpy
    ix, iy = G.bracket_expected(data.x, xy[:, 0]), G.bracket_expected(data.y, xy[:, 1])
    ok = (ix >= 0) & (iy >= 0)
    assert np.array_equal(ood == 0, ok)
    x, y, i, j = xy[ok, 0], xy[ok, 1], ix[ok], iy[ok]
    x1, x2, y1, y2 = data.x[i], data.x[i + 1], data.y[j], data.y[j + 1]
    z = data.z
    want = 1.0 / ((x2 - x1) * (y2 - y1)) * (
        z[i, j] * (x2 - x) * (y2 - y) + z[i + 1, j] * (x - x1) * (y2 - y) +
        z[i, j + 1] * (x2 - x) * (y - y1) + z[i + 1, j + 1] * (x - x1) * (y - y1))
    assert np.all(same_f64(h[ok], want))


@pytest.mark.parametrize("pair", G.TERRAINS, ids=IDS)
def test_pair_batches_exercise_the_terrain(pair):
    """The batch test_gpu_grid_parity.py validates on this terrain: some valid
    pairs, and the oracle's own near-line (FRAGILE) count under the bar of
    n * 1e-3 the GPU test holds the engine to."""
    data = G.terrain(*pair)
    O = oracle.OracleTerrain.from_data(data)
    oracle.set_scan_mode(1)
    s, a, d, _, tries = attempts_oracle(O, G.N_PAIRS, seed=G.pair_seed(pair))
    for adaptive in (False, True):
        v, _, _, f, _ = O.validate_pairs(s, a, d, adaptive=adaptive, nthreads=8)
        nfrag = int(((f & L.F_FRAGILE) != 0).sum())
        print(f"{data.name} ad{int(adaptive)}: {int(v.sum())} valid, {int(((f & L.F_OOD) != 0).sum())} "
              f"OOD, {nfrag} near a line, tries <= {int(tries.max())}, {int((tries < 0).sum())} unplaced")
        assert v.sum() > 0
        assert nfrag <= G.N_PAIRS * 1e-3
