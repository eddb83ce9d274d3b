"""The state check without its NaN tests and centre lookup, for maps the host
has verified to hold no NaN height (is_valid_state's NF, GBP_OPT_NAN_FREE /
GBP_OPT_NAN_TESTS), and how updates keep that fact.

Map: 64 x 64, uniform 0.1 m grid, fp32 heights, coordinates staged in LDS
(mode 1) or computed (mode 2): the two forms compiled without the NaN tests.
Attempts: 4,096 from the oracle's sampler, directions alternating; 320 of them
get a start position outside the domain, exactly on or just beyond the last
grid line (where heightIsNan's read is out of bounds), next to it (centre
inside, legs beyond), or NaN.  The kernel without the ring runs this batch as
it is.  The ring's kernel needs a slice of more than 64 attempts per wave, so
it runs the same attempts repeated to 65 per wave of the full grid, and its
outputs are compared with the same rows repeated.

Bar: on the NaN-free map the outputs with and without the NaN tests are byte
for byte the same arrays, and equal the oracle's (FRAGILE attempts re-decided
on the host, as the product does).  With a NaN cell at create, and through
host and device updates of a living handle, the option reads 1 exactly while
the host knows the map to be NaN-free, and the outputs equal the oracle's on
the map the device holds at that moment.
"""
import ctypes

import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from global_body_planner_amd import planner
from global_body_planner_amd import terrain_data as td
from tests.helpers import assert_pairs_equal, attempts_oracle, resolver

torch = pytest.importorskip("torch")

N = 4096
NX = NY = 64
SPACING = 0.1
NAN_CELL = (31, 30)
N_EDGE = 320
SEED = 20261020
_cache = {}


def map_data():
    return td.synth_rough(NX, spacing=SPACING)


def edge_positions(x, y, k):
    """The k-th special start position: (x, y), None = keep the sampled value."""
    x0, xN, y0, yN = x[0], x[-1], y[0], y[-1]
    nan, inf = float("nan"), float("inf")
    table = [
        (xN, None), (None, yN), (xN, yN),                            # on the last grid line
        (np.nextafter(xN, inf), None), (None, yN + 1e-9), (xN + 0.37, None), (inf, None),
        (x0 - 0.2, None), (None, np.nextafter(y0, -inf)),            # below the first
        (nan, None), (None, nan), (nan, nan),
        (xN - 0.05, None), (None, yN - 0.03),                        # centre inside, legs beyond
        (np.nextafter(xN, -inf), None), (x0, None),                  # the last and first values inside
    ]
    return table[k % len(table)]


def inputs():
    """(data, s, a, d, z with the NaN cell, oracle results on both maps), made once on the CPU."""
    if "in" not in _cache:
        data = map_data()
        assert data.z.shape == (NX, NY) and not np.isnan(data.z).any()
        O = oracle.OracleTerrain.from_data(data)
        s, a, d, _, _ = attempts_oracle(O, N, SEED)
        s = s.copy()
        rows = np.random.default_rng(SEED).choice(N, N_EDGE, replace=False)
        for k, r in enumerate(rows):
            px, py = edge_positions(data.x, data.y, k)
            if px is not None:
                s[r, 0] = px
            if py is not None:
                s[r, 1] = py
        out = (s[:, 0] < data.x[0]) | (s[:, 0] >= data.x[-1]) | (s[:, 1] < data.y[0]) | \
            (s[:, 1] >= data.y[-1])
        assert 0.03 * N <= out.sum() <= 0.07 * N, out.sum()        # about 5 %
        assert np.isnan(s[:, :2]).any(axis=1).sum() >= 40
        assert 0 < d.sum() < N                                       # both directions
        z_nan = data.z.copy()
        z_nan[NAN_CELL] = np.nan
        oracle.set_scan_mode(1)   # same brackets as the linear scan, faster
        try:
            ref = O.validate_pairs(s, a, d, nthreads=8)
            ref_nan = oracle.OracleTerrain(data.x, data.y, z_nan, data.dx, data.dy,
                                           data.dz).validate_pairs(s, a, d, nthreads=8)
        finally:
            oracle.set_scan_mode(0)
        # the oracle alone shows that the NaN cell is met and nothing else is NaN
        assert not (ref[3] & L.F_NAN).any()
        assert (ref_nan[3] & L.F_NAN).sum() >= 1
        assert (ref[3] & L.F_OOD).sum() >= 1
        _cache["in"] = (data, s, a, d, z_nan, ref, ref_nan)
    return _cache["in"]


def oracle_on(z):
    data, s, a, d = inputs()[:4]
    oracle.set_scan_mode(1)
    try:
        return oracle.OracleTerrain(data.x, data.y, z, data.dx, data.dy, data.dz).validate_pairs(
            s, a, d, nthreads=8)
    finally:
        oracle.set_scan_mode(0)


def handle(z=None, lds=1):
    import global_body_planner_amd as gbp
    data = inputs()[0]
    T = gbp.Terrain(data.x, data.y, data.z if z is None else z, data.dx, data.dy, data.dz)
    assert T.info()["storage"] == L.STORAGE_F32
    T.set_option(L.OPT_LDS_COORDS, lds)
    assert T.get_option(L.OPT_COORD_MODE) == (1 if lds else 2)
    return T


def ring_index(T):
    """Row numbers that repeat the N attempts to 65 per wave of the full grid."""
    from tests.test_gpu_block_rule import waves_of
    full = waves_of(T, 1 << 30)
    n = 65 * full
    assert waves_of(T, n) == full and n > 64 * full   # launch_validate_w takes the ring's kernel
    return np.arange(n) % N


def launch(T, idx=None, nan_tests=0):
    """One persistent launch of the attempts (rows idx): numpy (valid, s_new, t_new, flags, counts)."""
    from tests.test_gpu_refill_window import run
    _, s, a, d = inputs()[:4]
    if idx is not None:
        s, a, d = s[idx], a[idx], d[idx]
    dev = T.torch_device
    T.set_option(L.OPT_NAN_TESTS, nan_tests)
    try:
        return run(T, L.KERNEL_PERSISTENT, torch.from_numpy(s).to(dev), torch.from_numpy(a).to(dev),
                   torch.from_numpy(np.ascontiguousarray(d, np.uint8)).to(dev))
    finally:
        T.set_option(L.OPT_NAN_TESTS, 0)


def assert_bytes(got, ref, label):
    for name, g, r in zip(("valid", "s_new", "t_new", "flags", "counts"), got, ref):
        assert g.shape == r.shape and g.tobytes() == r.tobytes(), f"{label}: {name} differs"


def assert_oracle(T, got, ref, label, idx=None):
    _, s, a, d = inputs()[:4]
    if idx is not None:
        s, a, d = s[idx], a[idx], d[idx]
        ref = tuple(r[idx] for r in ref)
    return assert_pairs_equal(got, ref, label, resolve=resolver(T, s, a, d))


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [1, 0])
def test_nan_free_map(gpu, lds):
    """The option reads 1; with and without the NaN tests the outputs are the
    same bytes, and the oracle's; with and without the ring."""
    ref = inputs()[5]
    T = handle(lds=lds)
    assert T.get_option(L.OPT_NAN_FREE) == 1 and T.get_option(L.OPT_NAN_TESTS) == 0
    for name, idx in (("plain", None), ("ring", ring_index(T))):
        fast, general = launch(T, idx), launch(T, idx, nan_tests=1)
        assert_bytes(fast, general, f"lds {lds}/{name}")
        nres = assert_oracle(T, fast, ref, f"lds {lds}/{name}/oracle", idx)
        assert not (fast[3] & L.F_NAN).any()
        print(f"lds {lds} {name}: {len(fast[0])} attempts, {int(fast[0].sum())} valid, "
              f"{int(((fast[3] & L.F_OOD) != 0).sum())} OOD, {nres} re-decided")
    assert T.get_option(L.OPT_NAN_FREE) == 1


@pytest.mark.gpu
def test_one_nan_cell_at_create(gpu):
    """The option reads 0 and the outputs equal the oracle's, GBP_F_NAN among them."""
    z_nan, _, ref_nan = inputs()[4:]
    T = handle(z_nan)
    assert T.get_option(L.OPT_NAN_FREE) == 0
    for name, idx in (("plain", None), ("ring", ring_index(T))):
        got = launch(T, idx)
        assert (got[3] & L.F_NAN).sum() >= 1
        assert_oracle(T, got, ref_nan, f"nan cell/{name}", idx)
        assert_bytes(got, launch(T, idx, nan_tests=1), f"nan cell/{name}/forced")


@pytest.mark.gpu
def test_host_update_writes_and_removes_the_nan(gpu):
    data, _, _, _, z_nan, ref, ref_nan = inputs()
    T = handle()
    first = launch(T)
    assert_oracle(T, first, ref, "before")
    T.update(np.array([[np.nan]]), *NAN_CELL)
    assert T.get_option(L.OPT_NAN_FREE) == 0
    got = launch(T)
    assert (got[3] & L.F_NAN).sum() >= 1
    assert_oracle(T, got, ref_nan, "nan written")
    T.update(np.array([[data.z[NAN_CELL]]]), *NAN_CELL)
    assert T.get_option(L.OPT_NAN_FREE) == 1
    assert_bytes(launch(T), first, "nan removed")
    # a finite patch keeps the fact; a NaN elsewhere with the first restored clears it
    T.update(data.z[5:9, 7:20], 5, 7)
    assert T.get_option(L.OPT_NAN_FREE) == 1
    T.update(z_nan[20:40, 20:40], 20, 20)
    assert T.get_option(L.OPT_NAN_FREE) == 0
    T.update(data.z, 0, 0)
    assert T.get_option(L.OPT_NAN_FREE) == 1
    assert_bytes(launch(T), first, "whole map restored")


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["finite", "nan"])
def test_device_update(gpu, what):
    """A device update's values are unknown to the host: the option reads 0
    until the mirror has taken them in, whatever they are."""
    data = inputs()[0]
    z = data.z.copy()
    rect = (28, 26, 6, 9)
    sel = (slice(rect[0], rect[0] + rect[2]), slice(rect[1], rect[1] + rect[3]))
    z[sel] = (z[sel] + 0.03125).astype(np.float32).astype(np.float64)
    if what == "nan":
        z[NAN_CELL] = np.nan
    want = oracle_on(z)
    T = handle()
    assert T.get_option(L.OPT_NAN_FREE) == 1
    st = T.update(torch.from_numpy(np.ascontiguousarray(z[sel])).to(T.torch_device), rect[0], rect[1])
    torch.cuda.synchronize()
    assert int(st[0]) == 0
    assert T.get_option(L.OPT_NAN_FREE) == 0
    got = launch(T)
    assert T.get_option(L.OPT_NAN_FREE) == 0   # a launch reads nothing back
    assert_oracle(T, got, want, f"device update/{what}")
    back = T.read()                             # the mirror is refreshed on the way
    assert np.array_equal(np.isnan(back), np.isnan(z))
    assert T.get_option(L.OPT_NAN_FREE) == (1 if what == "finite" else 0)
    again = launch(T)
    assert_bytes(again, got, f"device update/{what}/after the refresh")
    assert_bytes(again, launch(T, nan_tests=1), f"device update/{what}/forced")
    assert ((again[3] & L.F_NAN) != 0).any() == (what == "nan")


@pytest.mark.gpu
def test_mirror_refresh_by_a_host_decision(gpu):
    """The host re-decision of FRAGILE attempts reads the mirror, which brings
    it up to date: the option returns to 1 without an explicit read."""
    data, s, a, d = inputs()[:4]
    T = handle()
    z = data.z[10:12, 10:12] + 0.5
    T.update(torch.from_numpy(np.ascontiguousarray(z)).to(T.torch_device), 10, 10)
    torch.cuda.synchronize()
    assert T.get_option(L.OPT_NAN_FREE) == 0
    T.validate_pairs_host(s[:64], a[:64], d[:64])
    assert T.get_option(L.OPT_NAN_FREE) == 1


@pytest.mark.gpu
def test_device_planner_trees(gpu):
    """The device planner loop (algorithm 3's kernel sequence, driven here on a
    handle of the test's own so that it can set the option) for 24 halves of 256
    draws, halts re-decided on the host: with and without the NaN tests the
    trees are the same bytes."""
    import global_body_planner_amd as gbp
    data = inputs()[0]
    O = oracle.OracleTerrain.from_data(data)
    hs, hg = O.ground_height(1.0, 1.0)[0], O.ground_height(5.2, 5.0)[0]
    start, goal = planner.start_goal_state(hs, 1.0, 1.0), planner.start_goal_state(hg, 5.2, 5.0)
    lib = L.load()
    batch, halves, seed = 256, 24, 20261021

    def grow(nan_tests):
        T = handle()
        T.set_option(L.OPT_NAN_TESTS, nan_tests)
        assert T.get_option(L.OPT_NAN_FREE) == 1
        ws = gbp.PlanWorkspace(T, batch)
        trees = [gbp.DeviceTree(p, device=0, capacity=1 << 15) for p in (start, goal)]
        ws.reset(0)
        attempts = 0
        for half in range(0, halves, 2):
            ws.halves(T, trees[0], trees[1], half, 2, batch, seed=seed)
            st = ws.status()
            while st["halt"]:
                h0 = st["halt_half"]
                k = h0 & 1
                resume, nres = ctypes.c_int(-1), ctypes.c_int64(0)
                L.check(lib.gbp_plan_resolve_host(T._h, ws._h, trees[k]._h, trees[k ^ 1]._h,
                                                  L.FORWARD if k == 0 else L.REVERSE, batch, 0,
                                                  ctypes.byref(resume), ctypes.byref(nres), None),
                        "plan_resolve")
                assert resume.value >= 0
                ws.halves(T, trees[0], trees[1], h0, half + 2 - h0, batch, seed=seed,
                          first_stage=resume.value)
                st = ws.status()
            assert not st["error"], st["error"]
            attempts = st["stat_attempts"]
            if st["done"]:
                break
        torch.cuda.synchronize()
        return [t.read() for t in trees], attempts

    fast, n_fast = grow(0)
    general, n_general = grow(1)
    assert n_fast == n_general and n_fast > 0
    assert len(fast[0][0]) + len(fast[1][0]) > 20    # the search went somewhere
    for k in range(2):
        for name, x, y in zip(("states", "actions", "parents", "g"), fast[k], general[k]):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (k, name)
    print(f"trees {len(fast[0][0])} + {len(fast[1][0])} vertices, {n_fast} attempts")
