"""A terrain's slope layers derived from its heights on the device
(gbp_terrain_derive_slopes_dev / _host, gbp_terrain_read_slopes_host,
GBP_OPT_DERIVE_SLOPES).

Expected values come from tests/test_slopes_host.py's numpy restatement of the
rule, evaluated on the heights as the handle stores them (float-rounded for
fp32 storage), and are compared bit for bit; any NaN equals any NaN
(tests.helpers.same_f64: inf - inf and 0 / 0 give another NaN on gfx950 than on
x86).
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import oracle
from global_body_planner_amd import _lib as L
from global_body_planner_amd import engine, terrain_data as td
from tests import prune_ref as R
from tests.helpers import bits, same_f64
from tests.test_slopes_host import cases, graded, restate, rough

pytestmark = pytest.mark.gpu

STORAGES = [L.STORAGE_F32, L.STORAGE_F64]
SENTINEL = 7.0


def stored(z, storage):
    z = np.asarray(z, np.float64)
    return z.astype(np.float32).astype(np.float64) if storage == L.STORAGE_F32 else z


def assert_layers(got, want, label=""):
    for name, g, w in zip(("dx", "dy", "dz"), got, want):
        ok = same_f64(g, w)
        assert ok.all(), (label, name, np.argwhere(~ok)[:5].tolist())


def derive(T, entry, rect=None, f32=False):
    """Through the host entry, or the device entry on torch's current stream."""
    if entry == "host":
        T.derive_slopes(rect, round_f32=f32)
    else:
        T.derive_slopes(rect, round_f32=f32, stream=torch.cuda.current_stream(0))
        torch.cuda.synchronize()   # read_slopes runs on the handle's own stream


def sentinel_handle(x, y, z, storage):
    s = np.full(z.shape, SENTINEL)
    return engine.Terrain(x, y, z, s, s, s, storage=storage)


def reset_sentinel(T, z):
    s = np.full(z.shape, SENTINEL)
    T.update(z, 0, 0, s, s, s)


def big_map(seed=21, nan=True):
    """70 x 131, graded coordinates, float-representable heights, NaN cells."""
    x, y, z = graded(70, seed), graded(131, seed + 1), rough(70, 131, seed + 2)
    if nan:
        z[10:12, 40:43] = np.nan
        z[0, 0] = z[69, 130] = z[33, 0] = np.nan
    return x, y, z


# ---- whole map -----------------------------------------------------------------
@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("storage", STORAGES)
def test_whole_map(gpu, storage, f32, entry):
    """Every map of the CPU test, 37x29-f64 among them: heights that are not
    float-representable, read as stored (rounded on the fp32 handle)."""
    for name, (x, y, z) in list(cases().items()) + [("70x131", big_map())]:
        if entry == "host":
            T = engine.Terrain(x, y, z, storage=storage)   # the entry allocates the layers
        else:
            T = sentinel_handle(x, y, z, storage)
        derive(T, entry, None, f32)
        assert_layers(T.read_slopes(), restate(x, y, stored(z, storage), f32), (name, storage))
        assert np.array_equal(bits(T.read()), bits(stored(z, storage)))   # heights untouched
        T.close()


# ---- rectangles -----------------------------------------------------------------
def all_rects(nx, ny):
    for (a, b), (c, d) in itertools.product(itertools.combinations(range(nx + 1), 2),
                                            itertools.combinations(range(ny + 1), 2)):
        yield a, c, b - a, d - c


def side_rects(nx, ny, sides=(1, 31, 32, 33, 65)):
    """Each pair of sides at each corner, each edge and the interior."""
    for sx, sy in itertools.product(sides, sides):
        for ox, oy in itertools.product({0, 3, nx - sx}, {0, 5, ny - sy}):
            if 0 <= ox <= nx - sx and 0 <= oy <= ny - sy:
                yield ox, oy, sx, sy


def check_rect(T, z_stored, x, y, rect, entry, f32, label):
    ix0, iy0, pnx, pny = rect
    derive(T, entry, rect, f32)
    want = [np.full(z_stored.shape, SENTINEL) for _ in range(3)]
    for w, r in zip(want, restate(x, y, z_stored, f32)):
        w[ix0:ix0 + pnx, iy0:iy0 + pny] = r[ix0:ix0 + pnx, iy0:iy0 + pny]
    assert_layers(T.read_slopes(), want, label)
    # the rectangle read on its own
    assert_layers(T.read_slopes(rect), [w[ix0:ix0 + pnx, iy0:iy0 + pny] for w in want], label)


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("storage", STORAGES)
def test_every_rectangle_of_a_small_map(gpu, storage, entry):
    x, y, z = cases()["5x4-nan-1-2"]
    T = sentinel_handle(x, y, z, storage)
    for k, rect in enumerate(all_rects(5, 4)):
        reset_sentinel(T, z)
        check_rect(T, stored(z, storage), x, y, rect, entry, bool(k & 1), rect)


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("storage", STORAGES)
def test_rectangles_across_wave_edges(gpu, storage, entry):
    """Sides 1 / 31 / 32 / 33 / 65 of a 70 x 131 map: one 256-lane workgroup a
    row (the next test has several)."""
    x, y, z = big_map()
    T = sentinel_handle(x, y, z, storage)
    rects = sorted(set(side_rects(70, 131)))
    assert len(rects) >= 200
    for k, rect in enumerate(rects):
        reset_sentinel(T, z)
        check_rect(T, stored(z, storage), x, y, rect, entry, bool(k & 1), rect)


def wide_map(nx, ny, seed):
    """ny > 512: k_derive_slopes runs three 256-lane workgroups a row.  Graded
    coordinates, float-representable heights, NaN beside the workgroup edges."""
    x, y, z = graded(nx, seed), graded(ny, seed + 1), rough(nx, ny, seed + 2)
    z[1, 255] = z[2, 256] = z[nx - 1, 512] = z[0, 511] = z[nx - 2, ny - 1] = np.nan
    return x, y, z


WIDE = {"5x600": (5, 600, 41), "70x515": (70, 515, 44)}
EDGES = (255, 256, 257, 511, 512, 513)


def workgroup_edge_rects(nx, ny):
    """iy ranges that begin or end at 255 / 256 / 257 and 511 / 512 / 513 (and
    at the map's edges), over the whole x range, an interior one and single rows."""
    cuts = (0,) + EDGES + (ny,)
    xr = [(0, nx), (1, nx - 2), (0, 1), (nx - 1, 1)]
    k = 0
    for a, b in itertools.combinations(cuts, 2):
        yield xr[k % len(xr)][0], a, xr[k % len(xr)][1], b - a
        k += 1


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", sorted(WIDE))
def test_whole_map_wider_than_a_workgroup(gpu, shape, storage, entry):
    x, y, z = wide_map(*WIDE[shape])
    for f32 in (False, True):
        T = engine.Terrain(x, y, z, storage=storage) if entry == "host" \
            else sentinel_handle(x, y, z, storage)
        derive(T, entry, None, f32)
        assert_layers(T.read_slopes(), restate(x, y, stored(z, storage), f32), (shape, f32))
        T.close()


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", sorted(WIDE))
def test_rectangles_across_workgroup_edges(gpu, shape, storage, entry):
    """A rectangle's lanes are counted from its own iy0, so the workgroup edges
    fall at iy0 + 256 k: ranges that begin or end beside 256 and 512 and are
    shorter than, equal to and longer than one and two workgroups."""
    nx, ny, seed = WIDE[shape]
    x, y, z = wide_map(nx, ny, seed)
    T = sentinel_handle(x, y, z, storage)
    rects = list(workgroup_edge_rects(nx, ny))
    assert any(r[3] > 512 for r in rects) and any(r[3] in (256, 257) for r in rects)
    for k, rect in enumerate(rects):
        reset_sentinel(T, z)
        check_rect(T, stored(z, storage), x, y, rect, entry, bool(k & 1), rect)


def test_rectangle_errors(gpu):
    x, y, z = cases()["5x4"]
    T = sentinel_handle(x, y, z, L.STORAGE_F64)
    for rect in ((0, 0, 0, 1), (4, 0, 2, 1), (0, 3, 1, 2), (-1, 0, 1, 1)):
        for stream in (None, torch.cuda.current_stream(0)):
            with pytest.raises(L.GbpError) as e:
                T.derive_slopes(rect, stream=stream)
            assert e.value.status == L.E_SHAPE
        with pytest.raises(L.GbpError) as e:
            T.read_slopes(rect)
        assert e.value.status == L.E_SHAPE
    lib = L.load()
    assert lib.gbp_terrain_derive_slopes_host(T._h, None, 1) == L.E_INVALID_ARG   # unknown flag
    assert lib.gbp_terrain_derive_slopes_dev(T._h, None, 4, None) == L.E_INVALID_ARG
    assert all(np.all(v == SENTINEL) for v in T.read_slopes())


# ---- a handle created without layers ------------------------------------------------
def test_a_handle_created_without_layers(gpu):
    x, y, z = big_map()
    T = engine.Terrain(x, y, z, storage=L.STORAGE_F64)
    with pytest.raises(L.GbpError) as e:
        T.derive_slopes(stream=torch.cuda.current_stream(0))
    assert e.value.status == L.E_INVALID_ARG
    with pytest.raises(L.GbpError) as e:
        T.set_option(L.OPT_DERIVE_SLOPES, 1)
    assert e.value.status == L.E_INVALID_ARG
    assert T.get_option(L.OPT_DERIVE_SLOPES) == 0
    with pytest.raises(L.GbpError) as e:
        T.read_slopes()
    assert e.value.status == L.E_INVALID_ARG
    rect = (20, 30, 33, 65)
    T.derive_slopes(rect)
    want = [np.full(z.shape, v) for v in (0.0, 0.0, 1.0)]
    for w, r in zip(want, restate(x, y, z)):
        w[20:53, 30:95] = r[20:53, 30:95]
    got = T.read_slopes()
    assert_layers(got, want)
    assert not np.signbit(got[0][0, 0])   # (+0, +0, 1), what a handle without layers reads
    # now the handle has layers: the device entry and the option are accepted
    T.set_option(L.OPT_DERIVE_SLOPES, 1 | L.SLOPES_F32)
    assert T.get_option(L.OPT_DERIVE_SLOPES) == 3
    for bad in (2, 4, 5, -1):
        with pytest.raises(L.GbpError):
            T.set_option(L.OPT_DERIVE_SLOPES, bad)
    T.set_option(L.OPT_DERIVE_SLOPES, 0)
    derive(T, "dev")
    assert_layers(T.read_slopes(), restate(x, y, z))


# ---- upkeep: update ---------------------------------------------------------------
def dilated(rect, nx, ny):
    ix0, iy0, pnx, pny = rect
    return (slice(max(ix0 - 1, 0), min(ix0 + pnx + 1, nx)), slice(max(iy0 - 1, 0), min(iy0 + pny + 1, ny)))


def patch_values(rect, seed, nan_block=False):
    p = (rough(rect[2], rect[3], seed) + 0.05).astype(np.float32).astype(np.float64)
    if nan_block:
        p[:2, :2] = np.nan
    return p


UPDATE_RECTS = [(0, 0, 1, 1), (69, 130, 1, 1), (0, 40, 5, 33), (20, 0, 32, 7), (30, 50, 31, 65),
                (66, 100, 4, 31), (0, 0, 70, 131)]


def apply_update(T, entry, patch, rect, layers=(None, None, None)):
    if entry == "host":
        T.update(patch, rect[0], rect[1], *layers)
        return None
    dev = lambda a: None if a is None else torch.as_tensor(a, device="cuda:0")
    return T.update(dev(patch), rect[0], rect[1], *[dev(v) for v in layers])


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("storage", STORAGES)
def test_an_update_without_layers_keeps_them_derived(gpu, storage, f32, entry):
    check_updates(*big_map(), UPDATE_RECTS, storage, f32, entry)


WIDE_UPDATE_RECTS = [(10, 250, 8, 10), (3, 255, 2, 258), (60, 500, 10, 15), (0, 257, 70, 255),
                     (0, 0, 70, 515)]


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("storage", STORAGES)
def test_an_update_across_workgroup_edges(gpu, storage, entry):
    """The upkeep's launch on a 70 x 515 map: dilated rectangles of more than
    one workgroup a row."""
    check_updates(*wide_map(*WIDE["70x515"]), WIDE_UPDATE_RECTS, storage, entry == "dev", entry)


def check_updates(x, y, z0, rects, storage, f32, entry):
    T = sentinel_handle(x, y, z0, storage)
    T.set_option(L.OPT_DERIVE_SLOPES, 1 | (L.SLOPES_F32 if f32 else 0))
    assert all(np.all(v == SENTINEL) for v in T.read_slopes())   # setting it launched nothing
    for k, rect in enumerate(rects):
        reset_sentinel(T, z0)
        z = z0.copy()
        # a NaN block set, then cleared by a second update of the same rectangle
        for step, patch in enumerate((patch_values(rect, 100 + k, nan_block=True),
                                      patch_values(rect, 200 + k))):
            st = apply_update(T, entry, patch, rect)
            z[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]] = patch
            want = [np.full(z.shape, SENTINEL) for _ in range(3)]
            d = dilated(rect, *z.shape)
            for w, r in zip(want, restate(x, y, stored(z, storage), f32)):
                w[d] = r[d]
            assert_layers(T.read_slopes(), want, (rect, step))
            assert np.array_equal(bits(T.read()), bits(stored(z, storage)))
            if st is not None:
                assert int(st.cpu()[0]) == 0


@pytest.mark.parametrize("storage", STORAGES)
def test_update_dev_then_normals_on_one_stream(gpu, storage):
    """No synchronise between the update and the lookup: the derive launch is
    ordered on the caller's stream behind the apply launch."""
    x, y, z0 = big_map(nan=False)
    T = sentinel_handle(x, y, z0, storage)
    derive(T, "host")
    T.set_option(L.OPT_DERIVE_SLOPES, 1)
    rect = (20, 40, 33, 65)
    patch = patch_values(rect, 77)
    z = z0.copy()
    z[20:53, 40:105] = patch
    rng = np.random.default_rng(5)
    xy = np.stack([rng.uniform(x[0], x[-1], 4096), rng.uniform(y[0], y[-1], 4096)], 1)
    dxy, dpatch = torch.as_tensor(xy, device="cuda:0"), torch.as_tensor(patch, device="cuda:0")
    torch.cuda.synchronize()
    T.update(dpatch, rect[0], rect[1])
    nrm, ood = T.normal(dxy)
    torch.cuda.synchronize()
    O = oracle.OracleTerrain(x, y, stored(z, storage), *restate(x, y, stored(z, storage)))
    want, _ = O.normal_batch(xy)
    assert same_f64(nrm.cpu().numpy(), want).all()
    assert_layers(T.read_slopes(), restate(x, y, stored(z, storage)))


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_a_rejected_update_leaves_heights_and_layers(gpu, entry):
    x, y, z0 = big_map()
    T = sentinel_handle(x, y, z0, L.STORAGE_F32)
    T.set_option(L.OPT_DERIVE_SLOPES, 1)
    rect = (20, 40, 33, 65)
    patch = patch_values(rect, 78)
    patch[7, 9] = 0.1   # no float
    if entry == "host":
        with pytest.raises(L.GbpError) as e:
            apply_update(T, entry, patch, rect)
        assert e.value.status == L.E_UNSUPPORTED
    else:
        st = apply_update(T, entry, patch, rect)
        torch.cuda.synchronize()
        assert int(st.cpu()[0]) == 1
    assert all(np.all(v == SENTINEL) for v in T.read_slopes())
    assert np.array_equal(bits(T.read()), bits(z0))


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_an_update_given_layers_writes_exactly_those(gpu, entry):
    x, y, z0 = big_map()
    T = sentinel_handle(x, y, z0, L.STORAGE_F64)
    T.set_option(L.OPT_DERIVE_SLOPES, 1 | L.SLOPES_F32)
    rect = (20, 40, 33, 65)
    patch = patch_values(rect, 79)
    layers = [np.full(patch.shape, v) + np.arange(patch.shape[1]) for v in (3.0, 4.0, 5.0)]
    apply_update(T, entry, patch, rect, layers)
    want = [np.full(z0.shape, SENTINEL) for _ in range(3)]
    for w, l in zip(want, layers):
        w[20:53, 40:105] = l
    assert_layers(T.read_slopes(), want)


# ---- upkeep: move -----------------------------------------------------------------
def window_of(big, h, ox, oy, nx, ny):
    """The window at cell (ox, oy): positions recomputed from its origin."""
    return (ox * h + np.arange(nx) * h, oy * h + np.arange(ny) * h,
            np.ascontiguousarray(big[ox:ox + nx, oy:oy + ny]))


def axis_shifts(n):
    return [0, 1, -1, 2, -2, n - 1, -(n - 1), n, -n]


def check_move(big, h, nx, ny, origin, shift, storage, f32):
    x0, y0, z0 = window_of(big, h, origin[0], origin[1], nx, ny)
    T = engine.Terrain(x0, y0, z0, storage=storage)
    T.derive_slopes(round_f32=f32)
    T.set_option(L.OPT_DERIVE_SLOPES, 1 | (L.SLOPES_F32 if f32 else 0))
    x1, y1, z1 = window_of(big, h, origin[0] + shift[0], origin[1] + shift[1], nx, ny)
    T.move(shift[0], shift[1], x1, y1, z1)
    F = engine.Terrain(x1, y1, z1, storage=storage)   # a fresh create of the moved arrays
    F.derive_slopes(round_f32=f32)
    want = F.read_slopes()
    assert_layers(T.read_slopes(), want, shift)
    assert_layers(want, restate(x1, y1, stored(z1, storage), f32), shift)
    for copy in (0, 1):
        assert np.array_equal(bits(T.read(copy=copy)), bits(F.read(copy=copy))), shift
    assert T.get_option(L.OPT_DERIVE_SLOPES) == (3 if f32 else 1)
    T.close()
    F.close()


@pytest.mark.parametrize("storage", STORAGES)
def test_every_shift_class_of_a_small_map(gpu, storage):
    """Axis-only and diagonal shifts, |shift| = n among them: no overlap."""
    nx, ny, h = 9, 7, 0.02
    big = rough(3 * nx, 3 * ny, 31, f32=storage == L.STORAGE_F32)
    big[nx + 3, ny + 2] = big[nx - 1, ny + 4] = big[2 * nx, 2 * ny] = np.nan
    for k, shift in enumerate(itertools.product(axis_shifts(nx), axis_shifts(ny))):
        check_move(big, h, nx, ny, (nx, ny), shift, storage, bool(k & 1))


@pytest.mark.parametrize("storage", STORAGES)
def test_a_move_of_a_larger_map(gpu, storage):
    big = rough(80, 140, 32)
    big[40:42, 60:70] = np.nan
    check_move(big, 0.02, 70, 131, (4, 4), (3, -2), storage, False)


@pytest.mark.parametrize("storage", STORAGES)
def test_a_move_of_a_map_wider_than_a_workgroup(gpu, storage):
    """70 x 515: the whole-map derive into the second buffer set runs three
    workgroups a row.  A small diagonal shift and one along y past a workgroup."""
    big = rough(80, 830, 34)
    big[40:42, 250:260] = big[10, 511:514] = big[70, 700] = np.nan
    for shift, f32 in (((3, -2), False), ((-1, 257), True)):
        check_move(big, 0.02, 70, 515, (4, 4), shift, storage, f32)


# ---- option off ---------------------------------------------------------------------
def test_option_off_keeps_todays_behaviour(gpu):
    """Never set, never derived: an update without layers leaves them, a move
    without layers shifts them and reads (0, 0, 1) in the strips."""
    nx, ny, h = 70, 131, 0.02
    big = rough(80, 140, 33)
    x0, y0, z0 = window_of(big, h, 4, 4, nx, ny)
    rng = np.random.default_rng(9)
    lay = [rng.uniform(-1, 1, z0.shape) for _ in range(3)]
    T = engine.Terrain(x0, y0, z0, *lay, storage=L.STORAGE_F32)
    assert T.get_option(L.OPT_DERIVE_SLOPES) == 0
    assert_layers(T.read_slopes(), lay)
    rect = (20, 40, 33, 65)
    T.update(patch_values(rect, 80), rect[0], rect[1])
    assert_layers(T.read_slopes(), lay)
    x1, y1, z1 = window_of(big, h, 7, 2, nx, ny)
    T.move(3, -2, x1, y1, z1)
    want = [np.full(z0.shape, v) for v in (0.0, 0.0, 1.0)]
    for w, l in zip(want, lay):
        w[:nx - 3, 2:] = l[3:, :ny - 2]
    assert_layers(T.read_slopes(), want)


# ---- in use -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rough256():
    d = td.synth_rough(256)
    lay = restate(d.x, d.y, d.z, f32=True)
    return d, lay


def test_normals_read_the_derived_layers(gpu, rough256):
    d, lay = rough256
    T = engine.Terrain(d.x, d.y, d.z)
    T.derive_slopes(round_f32=True)
    rng = np.random.default_rng(6)
    xy = np.stack([rng.uniform(d.x[0], d.x[-1], 4096), rng.uniform(d.y[0], d.y[-1], 4096)], 1)
    nrm, _ = T.normal(torch.as_tensor(xy, device="cuda:0"))
    torch.cuda.synchronize()
    want, _ = oracle.OracleTerrain(d.x, d.y, d.z, *lay).normal_batch(xy)
    assert same_f64(nrm.cpu().numpy(), want).all()


def test_extend_reads_the_derived_layers(gpu, rough256):
    d, lay = rough256
    n, seed = 4096, 7
    A = engine.Terrain(d.x, d.y, d.z)
    A.derive_slopes(round_f32=True)
    B = engine.Terrain(d.x, d.y, d.z, *lay)
    C = engine.Terrain(d.x, d.y, d.z)   # no layers: (0, 0, 1) everywhere
    s_near, _ = B.sample_states(n, seed=seed, stream_id=1, require_phase=L.STANCE, max_tries=64)
    target, _ = B.sample_states(n, seed=seed, stream_id=2)
    direction = (torch.arange(n, device="cuda:0") % 2).to(torch.uint8)
    out = [T.extend(s_near, target, direction, seed) for T in (A, B, C)]
    torch.cuda.synchronize()
    fields = ("result", "chosen", "s_new", "a_new", "counts", "flags")
    a, b, c = [[getattr(r, f).cpu().numpy() for f in fields] for r in out]
    for f, va, vb in zip(fields, a, b):
        if va.dtype == np.float64:
            assert same_f64(va, vb).all(), f
        else:
            assert np.array_equal(va, vb), f
    advanced = int((a[0] != L.TRAPPED).sum())
    print(f"{advanced} of {n} attempts advanced or reached")
    assert advanced >= 1 and np.any(a[4] != 0)   # the comparison is not over empty outputs
    # the sampler reads the layers: a handle without them gives other outputs
    differs = [f for f, va, vc in zip(fields, a, c)
               if not (same_f64(va, vc) if va.dtype == np.float64 else va == vc).all()]
    print("fields that differ from the handle without layers:", differs)
    assert "a_new" in differs


def plan_halves(T, ws, start, goal, halves, batch, seed):
    lib = L.load()
    trees = [engine.DeviceTree(s, device=0, capacity=1 << 16) for s in (start, goal)]
    ws.reset(0)
    st = None
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
        if st["done"]:
            break
    return [t.read() for t in trees], st


def test_the_planner_loop_on_a_workspace_created_before_the_derivation(gpu, rough256):
    d, lay = rough256
    start, goal = R.start_goal()
    batch, seed, halves = 256, 3, 50
    A = engine.Terrain(d.x, d.y, d.z)
    wa = engine.PlanWorkspace(A, batch)   # before the layers exist
    A.derive_slopes(round_f32=True)
    B = engine.Terrain(d.x, d.y, d.z, *lay)
    wb = engine.PlanWorkspace(B, batch)
    (ta, sa), (tb, sb) = (plan_halves(T, w, start, goal, halves, batch, seed)
                          for T, w in ((A, wa), (B, wb)))
    assert sum(len(t[2]) for t in ta) > 2   # the trees grew
    for k in range(2):
        for va, vb in zip(ta[k], tb[k]):
            assert va.shape == vb.shape
            assert (same_f64(va, vb) if va.dtype == np.float64 else va == vb).all()
    for f in ("ext_counter", "stat_targets", "done"):
        assert sa[f] == sb[f], f


# ---- the C++ surface ------------------------------------------------------------------
def test_fast_terrain_map_on_an_elevation_only_source(gpu, tmp_path):
    """tests/integration/terrain_slopes_node.cpp: setDeriveSlopes(true), then
    load, update, move and a reload from a mock GridMap without slope layers;
    after each, readSlopes equals a whole-map deriveSlopes on a second map."""
    import subprocess
    from tests.test_abi import build_node_callsite
    exe = build_node_callsite(tmp_path / "terrain_slopes_node", src="terrain_slopes_node.cpp")
    out = subprocess.run(["timeout", "-k", "10", "60", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines() == [f"{s}: same" for s in
                                       ("load", "update", "move", "reload", "update after reload")]
