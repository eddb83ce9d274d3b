"""A terrain handle's heights updated in place (gbp_terrain_update_dev / _host,
gbp_terrain_read_host, csrc/gbp_terrain.hip).

The yardstick throughout is a fresh engine.Terrain created on the patched
arrays with the same storage and options, with the oracle beside it; every
comparison is bit for bit.  A height lies in up to two x-pairs of the device
layout, so every case reads both copies back.
"""
import ctypes
import itertools
import subprocess

import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from global_body_planner_amd import engine, terrain_data as td, workload as W
from tests import prune_ref as R
from tests.helpers import assert_pairs_equal, bits, resolver, same_f64, u32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MASK = np.uint32(~(L.F_FRAGILE | L.F_RESOLVED) & 0xFFFFFFFF)


@pytest.fixture(autouse=True)
def _bisect():
    oracle.set_scan_mode(1)  # same brackets as the linear scan, faster
    yield
    oracle.set_scan_mode(0)


def np_(t):
    return t.cpu().numpy()


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def gridmap_layer(z, pad=3, fill=-999.0):
    """x-major z[NX][NY] as the grid_map layer it came from: float32 [NY][NX +
    pad], cell (ix, iy) at [NY-1-iy][NX-1-ix] (fast_terrain_map.cpp:57-61)."""
    nx, ny = z.shape
    out = np.full((ny, nx + pad), fill, np.float32)
    out[:, :nx] = z[::-1, ::-1].T
    return out


def apply(T, z_new, rect=None, layout=L.SRC_F64_XMAJOR, dev=False, layers=None, junk=None):
    """Update T's cells rect = (ix0, iy0, pnx, pny) to z_new's (x-major, whole
    map) through the host or the device entry.  With layout SRC_F32_GRIDMAP the
    whole layer is passed; `junk` then stands in every cell outside the
    rectangle, which the update must not take.  Returns the status tensor of
    the device entry."""
    nx, ny = z_new.shape
    ix0, iy0, pnx, pny = rect if rect is not None else (0, 0, nx, ny)
    sel = (slice(ix0, ix0 + pnx), slice(iy0, iy0 + pny))
    srcs = []
    for full in [z_new] + list(layers or []):
        if layout == L.SRC_F32_GRIDMAP:
            a = full
            if junk is not None:
                a = np.full_like(full, junk)
                a[sel] = full[sel]
            srcs.append(gridmap_layer(a))
        else:
            srcs.append(np.ascontiguousarray(full[sel]))
    if dev:
        srcs = [torch.from_numpy(s).to(T.torch_device) for s in srcs]
    kw = dict(zip(("dx", "dy", "dz"), srcs[1:]))
    return T.update(srcs[0], ix0, iy0, layout=layout,
                    shape=(pnx, pny) if layout == L.SRC_F32_GRIDMAP else None, **kw)


def assert_holds(T, z, label=""):
    """Both copies of every height T's device holds equal z."""
    for copy in (0, 1):
        got = T.read(copy=copy)
        assert got.shape == z.shape
        bad = np.argwhere(~same_f64(got, z))
        assert bad.size == 0, (label, copy, bad[:5])


def all_rects(nx, ny):
    for (a, b), (c, d) in itertools.product(itertools.combinations(range(nx + 1), 2),
                                            itertools.combinations(range(ny + 1), 2)):
        yield a, c, b - a, d - c


# ---- 1: every rectangle of a small map ---------------------------------------------
@pytest.mark.parametrize("layout", [L.SRC_F64_XMAJOR, L.SRC_F32_GRIDMAP])
@pytest.mark.parametrize("storage", [L.STORAGE_F32, L.STORAGE_F64])
@pytest.mark.parametrize("shape", [(5, 4), (2, 2)])
def test_every_rectangle_of_a_small_map(gpu, shape, storage, layout):
    """Every rectangle in turn on one living handle, host and device entry
    alternating; 2 x 2 is the map of one pair row.  The fp64 handle takes
    heights no float holds (from the fp64 source; a grid_map source is float)."""
    nx, ny = shape
    rng = np.random.default_rng(100 * nx + 10 * storage + layout)
    exact = storage == L.STORAGE_F32 or layout == L.SRC_F32_GRIDMAP
    draw = (lambda: f32(rng.uniform(-1, 1, shape))) if exact else (lambda: rng.uniform(-1, 1, shape))
    x, y = np.arange(nx) * 0.1, np.arange(ny) * 0.1
    cur = draw()
    T = engine.Terrain(x, y, cur, storage=storage)
    assert_holds(T, cur, "created")
    n = 0
    for k, rect in enumerate(all_rects(nx, ny)):
        new = draw()
        sel = (slice(rect[0], rect[0] + rect[2]), slice(rect[1], rect[1] + rect[3]))
        cur = cur.copy()
        cur[sel] = new[sel]
        st = apply(T, new, rect, layout, dev=bool(k & 1), junk=55.0)
        if st is not None:
            assert int(st[0]) == 0
        assert_holds(T, cur, rect)
        n += 1
    assert n == (150 if shape == (5, 4) else 9)
    assert T.info()["storage"] == storage
    fresh = engine.Terrain(x, y, cur, storage=storage)
    for copy in (0, 1):
        assert np.array_equal(bits(T.read(copy=copy)), bits(fresh.read(copy=copy)))


# ---- 2: tile and edge shapes -------------------------------------------------------
def _graded(n):
    return np.concatenate([[0.0], np.cumsum(0.02 * 1.03 ** np.arange(n - 1, dtype=np.float64))])


MAPS = {"37x29-graded": (_graded(37), _graded(29)),
        "70x131": (np.arange(70) * 0.02, np.arange(131) * 0.02)}


def shape_rects(nx, ny):
    """1 x 1, 1 x pny, pnx x 1 and the sides 31 / 32 / 33 / 65 (cut to the map)
    at each corner, each edge, the interior, and ending at row nx - 2."""
    sizes = [(1, 1), (1, 33), (33, 1), (31, 32), (32, 33), (33, 31), (65, 65), (32, 65), (65, 31),
             (nx, 1), (1, ny)]
    out = []
    for a, b in sizes:
        pnx, pny = min(a, nx), min(b, ny)
        for ix0 in (0, nx - pnx, (nx - pnx) // 2, nx - 1 - pnx):
            for iy0 in (0, ny - pny, (ny - pny) // 2):
                r = (ix0, iy0, pnx, pny)
                if ix0 >= 0 and r not in out:
                    out.append(r)
    return out


def probe_points(x, y, rect):
    """Four points per cell, just inside each corner, over the rectangle +- 1 cell."""
    ix0, iy0, pnx, pny = rect
    ci = np.arange(max(ix0 - 2, 0), min(ix0 + pnx + 1, x.size - 1))
    cj = np.arange(max(iy0 - 2, 0), min(iy0 + pny + 1, y.size - 1))
    px = np.concatenate([x[ci] + 1e-3 * (x[ci + 1] - x[ci]), x[ci + 1] - 1e-3 * (x[ci + 1] - x[ci])])
    py = np.concatenate([y[cj] + 1e-3 * (y[cj + 1] - y[cj]), y[cj + 1] - 1e-3 * (y[cj + 1] - y[cj])])
    return np.stack(np.meshgrid(px, py, indexing="ij"), -1).reshape(-1, 2)


@pytest.mark.parametrize("layout", [L.SRC_F64_XMAJOR, L.SRC_F32_GRIDMAP])
@pytest.mark.parametrize("name", list(MAPS))
def test_tile_and_edge_shapes(gpu, name, layout):
    """37 x 29 has graded coordinates (the general bracket search, and nx != ny
    catches a swapped pair); 70 x 131 spans more than one 64-cell tile both
    ways.  After every rectangle: both copies, and height / normal around the
    rectangle against a fresh handle and the oracle."""
    x, y = MAPS[name]
    nx, ny = x.size, y.size
    base = td.synth_rough(max(nx, ny))
    cut = lambda a: np.ascontiguousarray(a[:nx, :ny])
    lay = [cut(base.dx), cut(base.dy), cut(base.dz)]
    rng = np.random.default_rng(nx + layout)
    cur = cut(base.z)
    T = engine.Terrain(x, y, cur, *lay)
    if name.startswith("37"):
        assert T.get_option(L.OPT_COORD_MODE) == 0   # neither computed nor one-step
    rects = shape_rects(nx, ny)
    assert any(r[0] + r[2] == nx for r in rects) and any(r[0] == 0 for r in rects)
    assert any(r[0] + r[2] == nx - 1 for r in rects)
    for k, rect in enumerate(rects):
        new = f32(cur + rng.uniform(0.05, 0.3, cur.shape))
        sel = (slice(rect[0], rect[0] + rect[2]), slice(rect[1], rect[1] + rect[3]))
        cur = cur.copy()
        cur[sel] = new[sel]
        st = apply(T, new, rect, layout, dev=bool(k & 1), junk=55.0)
        if st is not None:
            assert int(st[0]) == 0
        assert_holds(T, cur, rect)
        xy = probe_points(x, y, rect)
        F = engine.Terrain(x, y, cur, *lay)
        O = oracle.OracleTerrain(x, y, cur, *lay)
        h, nan, ood = T.height(torch.from_numpy(xy))
        fh, fnan, food = F.height(torch.from_numpy(xy))
        rh, rnan, rood = O.height_batch(xy)
        assert not rood.any() and not rnan.any()
        for a, b in ((fh, h), (fnan, nan), (food, ood)):
            assert torch.equal(a, b), rect
        assert np.array_equal(bits(np_(h)), bits(rh)), rect
        nrm, nood = T.normal(torch.from_numpy(xy))
        fn, _ = F.normal(torch.from_numpy(xy))
        rn, _ = O.normal_batch(xy)
        assert torch.equal(nrm, fn) and np.array_equal(bits(np_(nrm)), bits(rn)), rect
        F.close()


# ---- 3: NaN and rejection ------------------------------------------------------------
def test_nan_blocks_set_and_cleared(gpu):
    data = td.synth_rough(64)
    T = engine.Terrain.from_data(data)
    rng = np.random.default_rng(3)
    xy = torch.from_numpy(np.stack([rng.uniform(0, data.x[-1], 20000),
                                    rng.uniform(0, data.y[-1], 20000)], 1))
    holed = data.z.copy()
    holed[10:25, 30:41] = np.nan
    holed[40, 5] = np.nan
    for z, dev, rect in ((holed, False, (10, 30, 15, 11)), (holed, True, (40, 5, 1, 1)),
                         (data.z, True, (9, 3, 33, 40))):
        apply(T, z, rect, dev=dev)
    # the two steps again, each compared
    for z, rect, dev in ((holed, (5, 5, 50, 50), True), (data.z, (5, 5, 50, 50), False)):
        apply(T, z, rect, dev=dev)
        assert_holds(T, z)
        F = engine.Terrain(data.x, data.y, z, data.dx, data.dy, data.dz)
        h, nan, ood = T.height(xy)
        fh, fnan, food = F.height(xy)
        assert torch.equal(nan, fnan) and torch.equal(ood, food)
        assert np.all(same_f64(np_(h), np_(fh)))
        assert (int(fnan.sum()) > 0) == bool(np.isnan(z).any())


def test_patch_an_fp32_handle_cannot_hold_is_rejected_whole(gpu):
    """0.1 is no float: the fp32 handle refuses the patch through either entry
    and keeps every height; an fp64-storage handle takes it.  A fresh
    STORAGE_AUTO create of the patched map picks fp64: an update never changes
    a handle's storage type, so the two are different handles by design."""
    data = td.synth_rough(64)
    T = engine.Terrain.from_data(data)
    assert T.info()["storage"] == L.STORAGE_F32
    rect = (20, 7, 9, 33)
    z = data.z.copy()
    z[20:29, 7:40] = f32(z[20:29, 7:40] + 0.25)
    z[24, 30] = 0.1
    z[21, 9] = np.nan
    with pytest.raises(L.GbpError) as e:
        apply(T, z, rect)
    assert e.value.status == L.E_UNSUPPORTED
    assert_holds(T, data.z, "host")
    st = apply(T, z, rect, dev=True)
    torch.cuda.synchronize()
    assert int(st[0]) == 1
    assert_holds(T, data.z, "dev")
    # slope layers ride on the same gate
    before = T.normal(torch.tensor([[0.45, 0.5]], dtype=torch.float64))[0].clone()
    st = apply(T, z, rect, dev=True, layers=[data.dx + 1, data.dy + 1, data.dz + 1])
    assert int(st[0]) == 1
    assert torch.equal(T.normal(torch.tensor([[0.45, 0.5]], dtype=torch.float64))[0], before)
    # the same rectangle without the 0.1 goes through, NaN included
    z2 = z.copy()
    z2[24, 30] = 0.125
    assert int(apply(T, z2, rect, dev=True)[0]) == 0
    assert_holds(T, z2)
    D = engine.Terrain(data.x, data.y, data.z, storage=L.STORAGE_F64)
    assert int(apply(D, z, rect, dev=True)[0]) == 0
    assert_holds(D, z)
    apply(D, data.z, rect)
    apply(D, z, rect)
    assert_holds(D, z)
    assert D.info()["storage"] == L.STORAGE_F64 and T.info()["storage"] == L.STORAGE_F32
    assert engine.Terrain(data.x, data.y, z).info()["storage"] == L.STORAGE_F64


def test_argument_checks(gpu):
    data = td.synth_rough(64)
    T = engine.Terrain.from_data(data)
    N = engine.Terrain(data.x, data.y, data.z)   # no slope layers
    lib = L.load()
    z = np.zeros((4, 4))
    p = z.ctypes.data_as(ctypes.c_void_p)
    call = lambda h, r, layout, ld, *src: lib.gbp_terrain_update_host(h._h, ctypes.byref(r), layout,
                                                                      ld, *src)
    for r in (L.Rect(0, 0, 0, 4), L.Rect(61, 0, 4, 4), L.Rect(0, 61, 4, 4), L.Rect(-1, 0, 4, 4)):
        assert call(T, r, 0, 4, p, None, None, None) == L.E_SHAPE
        assert lib.gbp_terrain_read_host(T._h, ctypes.byref(r), 0, p) == L.E_SHAPE
    ok = L.Rect(3, 3, 4, 4)
    assert call(T, ok, 2, 4, p, None, None, None) == L.E_INVALID_ARG      # unknown layout
    assert call(T, ok, 0, 3, p, None, None, None) == L.E_SHAPE            # ld < pny
    assert call(T, ok, 0, 4, None, None, None, None) == L.E_INVALID_ARG   # no heights
    assert call(T, ok, 0, 4, p, p, None, None) == L.E_INVALID_ARG         # partial slope layers
    assert call(N, ok, 0, 4, p, p, p, p) == L.E_INVALID_ARG               # a handle without them
    assert lib.gbp_terrain_read_host(T._h, ctypes.byref(ok), 2, p) == L.E_INVALID_ARG
    assert lib.gbp_terrain_update_dev(T._h, ctypes.byref(ok), 0, 4, p, None, None, None, None,
                                      None) == L.E_INVALID_ARG            # the check needs a status word
    assert_holds(T, data.z)
    assert call(T, ok, 0, 4, p, None, None, None) == 0
    want = data.z.copy()
    want[3:7, 3:7] = 0.0
    assert_holds(T, want)
    assert np.array_equal(T.read((2, 5, 3, 4), copy=1), want[2:5, 5:9])


# ---- 4: the hot path sees it -----------------------------------------------------------
def _patched(z, which):
    z = z.copy()
    if which == "box":
        z[100:133, 120:137] += 0.5
    elif which == "corner0":
        z[0:40, 0:40] += 0.5
    elif which == "corner1":
        z[216:256, 216:256] += 0.5
    elif which == "nan":
        z[90:155, 60:125] = np.nan
    elif which == "noise":
        z += np.random.default_rng(20251017).uniform(-0.05, 0.05, z.shape)
    return f32(z)


PATCHES = {  # name -> (rectangles, layout, device entry)
    "box": ([(100, 120, 33, 17)], L.SRC_F64_XMAJOR, True),
    "corner0": ([(0, 0, 40, 40)], L.SRC_F32_GRIDMAP, False),
    "corner1": ([(216, 216, 40, 40)], L.SRC_F64_XMAJOR, False),
    "nan": ([(90, 60, 65, 65)], L.SRC_F32_GRIDMAP, True),
    "noise": ([None], L.SRC_F64_XMAJOR, False),
}
_hot = {}


def hot_inputs():
    """synth-rough-256, its oracle, and 4,096 attempts drawn on the unpatched
    map as workload.make_attempts draws them (seed 20251017), with the
    oracle's results on the unpatched map."""
    if not _hot:
        data = td.synth_rough(256)
        T0 = engine.Terrain.from_data(data)
        s, a, d, target, _ = W.make_attempts(T0, 4096, W.CONFIG_SEEDS[2])
        O0 = oracle.OracleTerrain.from_data(data)
        s, a, d, target = np_(s), np_(a), np_(d), np_(target)
        base = {ad: O0.validate_pairs(s, a, d, adaptive=ad, nthreads=8) for ad in (False, True)}
        _hot.update(data=data, s=s, a=a, d=d, target=target, base=base)
    return _hot


def pair_tuple(res):
    return np_(res.valid), np_(res.s_new), np_(res.t_new), u32(res.flags), u32(res.counts)


@pytest.mark.parametrize("which", list(PATCHES))
def test_hot_path_sees_the_update(gpu, which):
    hi = hot_inputs()
    data, s, a, d, target = hi["data"], hi["s"], hi["a"], hi["d"], hi["target"]
    rects, layout, dev = PATCHES[which]
    z = _patched(data.z, which)
    T = engine.Terrain.from_data(data)
    for rect in rects:
        st = apply(T, z, rect, layout, dev=dev, junk=55.0 if rect is not None else None)
        assert st is None or int(st[0]) == 0
    assert_holds(T, z)
    F = engine.Terrain(data.x, data.y, z, data.dx, data.dy, data.dz)
    O = oracle.OracleTerrain(data.x, data.y, z, data.dx, data.dy, data.dz)
    ts, ta, tdir = torch.from_numpy(s), torch.from_numpy(a), torch.from_numpy(d)
    for adaptive in (False, True):
        ref = O.validate_pairs(s, a, d, adaptive=adaptive, nthreads=8)
        old = hi["base"][adaptive]
        changed = int(((ref[0] != old[0]) | (ref[4] != old[4])).sum())
        print(f"{which} adaptive {adaptive}: {changed} of {len(s)} rows differ from the unpatched map")
        # an update that did nothing cannot pass (the bound is the plain check's)
        assert changed >= (1 if adaptive else 50)
        for kernel in (L.KERNEL_PERSISTENT, L.KERNEL_DIRECT):
            T.set_option(L.OPT_KERNEL, kernel)
            F.set_option(L.OPT_KERNEL, kernel)
            got = pair_tuple(T.validate_pairs(ts, ta, tdir, adaptive=adaptive))
            want = pair_tuple(F.validate_pairs(ts, ta, tdir, adaptive=adaptive))
            for g, w in zip(got, want):
                assert np.all(same_f64(g, w)) if g.dtype == np.float64 else np.array_equal(g, w)
            assert_pairs_equal(got, ref, f"{which}/k{kernel}/ad{adaptive}",
                               resolve=resolver(T, s, a, d, adaptive))
    # isValidState
    st8 = np.concatenate([s, target])
    for phase in (L.STANCE, L.FLIGHT):
        v, f, c = T.valid_states(torch.from_numpy(st8), phase)
        fv, ff, fc = F.valid_states(torch.from_numpy(st8), phase)
        assert torch.equal(v, fv) and torch.equal(f, ff) and torch.equal(c, fc)
        rv, rf, rc = O.valid_states(st8, phase, nthreads=8)
        hv, hf, hc = T.valid_states_host(st8, phase)
        assert np.array_equal(hv, rv) and np.array_equal(hf & MASK, rf & MASK) and np.array_equal(hc, rc)
    # extend
    base = 1000
    r = T.extend(ts, torch.from_numpy(target), tdir, seed=41, extend_base=base)
    fr = F.extend(ts, torch.from_numpy(target), tdir, seed=41, extend_base=base)
    for k in ("result", "chosen", "counts", "flags"):
        assert torch.equal(getattr(r, k), getattr(fr, k)), k
    assert np.all(same_f64(np_(r.s_new), np_(fr.s_new))) and np.all(same_f64(np_(r.a_new), np_(fr.a_new)))
    nrm = O.normal_batch(target[:, :2])[0]
    dense = np_(T.sample_actions(torch.from_numpy(np.repeat(nrm, 8, axis=0)), 41, 0x45585444,
                                 base * 8)).reshape(len(s), 8, 10)
    rr, rch, rsn, ran, rc = O.extend_batch(s, target, np.ascontiguousarray(dense[:, :6]), d, nthreads=8)
    sure = (u32(r.flags) & L.F_FRAGILE) == 0   # a FRAGILE extend is the host re-decision's
    assert sure.mean() > 0.99
    assert np.array_equal(np_(r.result)[sure], rr[sure]) and np.array_equal(np_(r.chosen)[sure], rch[sure])
    assert np.array_equal(u32(r.counts)[sure], rc[sure])
    acc = sure & (rr != L.TRAPPED)
    assert np.array_equal(bits(np_(r.s_new)[acc]), bits(rsn[acc]))
    assert np.array_equal(bits(np_(r.a_new)[acc]), bits(ran[acc]))


# ---- 5: slope layers ---------------------------------------------------------------------
def test_slope_layers(gpu):
    data = td.by_name("slope-gridmap")
    nx, ny = data.z.shape
    T = engine.Terrain.from_data(data)
    rng = np.random.default_rng(5)
    x0, xN, y0, yN = data.bounds
    xy = torch.from_numpy(np.stack([rng.uniform(x0, xN, 20000), rng.uniform(y0, yN, 20000)], 1))
    before = T.normal(xy)[0].clone()
    rect = (nx // 4, ny // 5, min(70, nx // 2), min(45, ny // 2))
    sel = (slice(rect[0], rect[0] + rect[2]), slice(rect[1], rect[1] + rect[3]))
    # heights alone: the layers stay as they are
    z = data.z.copy()
    z[sel] = f32(z[sel] + 0.25)
    apply(T, z, rect)
    assert torch.equal(T.normal(xy)[0], before)
    # the three layers replaced over the rectangle, either layout and entry
    for k, (layout, dev) in enumerate(((L.SRC_F64_XMAJOR, False), (L.SRC_F32_GRIDMAP, True),
                                       (L.SRC_F64_XMAJOR, True), (L.SRC_F32_GRIDMAP, False))):
        t = rng.uniform(-0.4, 0.4, (2,) + data.z.shape)
        n = np.stack([t[0], t[1], np.ones(data.z.shape)])
        n /= np.linalg.norm(n, axis=0)
        lay = []
        for old, new in zip((data.dx, data.dy, data.dz), n):
            full = old.copy()
            full[sel] = f32(new[sel])
            lay.append(full)
        st = apply(T, z, rect, layout, dev=dev, layers=lay, junk=55.0)
        assert st is None or int(st[0]) == 0
        F = engine.Terrain(data.x, data.y, z, *lay)
        nrm, ood = T.normal(xy)
        fn, food = F.normal(xy)
        assert torch.equal(nrm, fn) and torch.equal(ood, food)
        assert not torch.equal(nrm, before)
        assert torch.equal(T.sample_actions(nrm, 31, 3), F.sample_actions(fn, 31, 3))
        assert torch.equal(T.height(xy)[0], F.height(xy)[0])
        assert_holds(T, z)


# ---- 6: stream order ---------------------------------------------------------------------
def test_update_is_ordered_on_the_callers_stream(gpu):
    """height, update (device tensors), height on one stream with no
    synchronisation in between: the first sees the old map, the second the new."""
    data = td.synth_rough(256)
    z_new = _patched(data.z, "noise")
    old = engine.Terrain.from_data(data)
    new = engine.Terrain(data.x, data.y, z_new, data.dx, data.dy, data.dz)
    T = engine.Terrain.from_data(data)
    rng = np.random.default_rng(6)
    xy = torch.from_numpy(np.stack([rng.uniform(0, data.x[-1], 100000),
                                    rng.uniform(0, data.y[-1], 100000)], 1)).cuda()
    want_old, want_new = old.height(xy)[0], new.height(xy)[0]
    src = torch.from_numpy(z_new).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        h1 = T.height(xy)[0]
        st = T.update(src)
        h2 = T.height(xy)[0]
    side.synchronize()
    assert int(st[0]) == 0
    assert torch.equal(h1, want_old) and torch.equal(h2, want_new)
    assert not torch.equal(want_old, want_new)


# ---- 7: the mirror -----------------------------------------------------------------------
@pytest.mark.parametrize("pending", [1, 2])
def test_host_mirror_follows_device_updates(gpu, pending):
    """With the FRAGILE margin at 1e-3 most attempts are re-decided on the host
    from the handle's mirror of the heights, which a device update only marks
    stale: the host entries' results equal a fresh handle's in every output.
    pending = 2: two device updates on two streams before the first host call."""
    hi = hot_inputs()
    data, s, a, d = hi["data"], hi["s"][:2048], hi["a"][:2048], hi["d"][:2048]
    eps = int(round(1e-3 * 1e15))
    T = engine.Terrain.from_data(data)
    T.set_option(L.OPT_FRAGILE_EPS, eps)
    z = data.z
    if pending == 2:   # the mirror is in use before the updates
        T.validate_pairs_host(s[:64], a[:64], d[:64])
    sts = []
    for k, which in enumerate(("box", "nan")[:pending]):
        z = _patched(z, which)
        rect = PATCHES[which][0][0]
        torch.cuda.synchronize()
        # the second one on a stream of its own: the mirror then has two entries pending
        with torch.cuda.stream(torch.cuda.Stream() if k else torch.cuda.current_stream()):
            sts.append(apply(T, z, rect, dev=True))
    torch.cuda.synchronize()   # the host entries run on the handle's own stream
    assert all(int(st[0]) == 0 for st in sts)
    F = engine.Terrain(data.x, data.y, z, data.dx, data.dy, data.dz)
    F.set_option(L.OPT_FRAGILE_EPS, eps)
    for adaptive in (False, True):
        got = T.validate_pairs_host(s, a, d, adaptive=adaptive)
        want = F.validate_pairs_host(s, a, d, adaptive=adaptive)
        assert ((want[3] & L.F_RESOLVED) != 0).sum() >= 1
        for g, w in zip(got, want):
            assert np.all(same_f64(g, w)) if g.dtype == np.float64 else np.array_equal(g, w)
        ref = oracle.OracleTerrain(data.x, data.y, z, data.dx, data.dy, data.dz).validate_pairs(
            s, a, d, adaptive=adaptive, nthreads=8)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[4], ref[4])
    for phase in (L.STANCE, L.FLIGHT):
        got = T.valid_states_host(s, phase)
        want = F.valid_states_host(s, phase)
        assert ((want[1] & L.F_RESOLVED) != 0).sum() >= 1
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    print(f"{int(((want[1] & L.F_RESOLVED) != 0).sum())} of {len(s)} states re-decided from the mirror")


# ---- 8: what hangs on the handle survives --------------------------------------------------
def test_options_and_sampling_survive(gpu):
    data = td.synth_rough(64)
    T = engine.Terrain.from_data(data)
    opts = {L.OPT_KERNEL: L.KERNEL_DIRECT, L.OPT_BLOCK: 128, L.OPT_WAVES: 3, L.OPT_LDS_COORDS: 0,
            L.OPT_HELPERS: 0, L.OPT_AFFINE_COORDS: 0, L.OPT_XCD_MAP: 1, L.OPT_FAST_RCP: 0,
            L.OPT_FRAGILE_EPS: 5000, L.OPT_NN_STATS: 1}
    for k, v in opts.items():
        T.set_option(k, v)
    T.set_sampling(L.sampling(state_flag=True, state_p=0.3, speed_direction=True, action_flag=True,
                              action_p=0.4))
    ro = {k: T.get_option(k) for k in (L.OPT_COORD_MODE, L.OPT_LAUNCH_BLOCK, L.OPT_REFILL_WINDOW)}
    z = _patched(data.z, "noise")
    apply(T, z)
    apply(T, z, (3, 4, 40, 33), dev=True)
    for k, v in opts.items():
        assert T.get_option(k) == v, k
    for k, v in ro.items():
        assert T.get_option(k) == v, k
    cfg = T.get_sampling()
    assert (cfg.state_flag, cfg.state_speed_direction, cfg.state_p, cfg.action_flag, cfg.action_p) == \
        (1, 1, 0.3, 1, 0.4)
    assert T.info() == engine.Terrain(data.x, data.y, z, data.dx, data.dy, data.dz).info()


def _box_rect(cur, new):
    """The bounding rectangle of the cells where the two maps differ."""
    diff = ~same_f64(cur, new)
    ix, iy = np.flatnonzero(diff.any(1)), np.flatnonzero(diff.any(0))
    return int(ix[0]), int(iy[0]), int(ix[-1] - ix[0] + 1), int(iy[-1] - iy[0] + 1)


def test_trees_are_pruned_against_the_updated_handle(gpu):
    """One living handle taken from the unchanged map to box 1, box 2, box 3
    (each update undoes the box before it): DeviceTree.revalidate equals the
    restatement's remap, stats and tree for sets S and C."""
    from tests.test_gpu_tree_prune import assert_prune_equals, device_prune
    base, _ = R.terrain()
    # the boxes' heights (z + 0.5 in doubles) are not floats: an fp64 handle
    T = engine.Terrain.from_data(base, storage=L.STORAGE_F64)
    cur = base.z
    for k, box in enumerate(("box1", "box2", "box3")):
        z = R.terrain(box)[0].z
        st = apply(T, z, None if k == 1 else _box_rect(cur, z), dev=bool(k))
        assert st is None or int(st[0]) == 0
        cur = z
        torch.cuda.synchronize()   # the prunes below run on the handle's own stream
        assert_holds(T, z, box)
        for which in "SC":
            r, exp = R.search(which), R.expected(which, box)
            for j, (name, direction) in enumerate((("a", L.FORWARD), ("b", L.REVERSE))):
                assert_prune_equals(device_prune(T, r[name], direction), exp[j][:3], (which, box, name))


def test_search_continues_on_the_updated_handle(gpu):
    """A PlanWorkspace created for the handle before the update serves the
    search after it: C's trees pruned against the handle updated to box 1, then
    50 halves of the device planner loop from half 200 on the pruned DeviceTree
    objects, equal to the oracle's continuation on the new map."""
    from global_body_planner_amd.engine import _stream
    from tests.test_gpu_tree_prune import assert_same_tree
    lib = L.load()
    cfg = R.SETS["C"]
    batch, seed, first, halves = cfg["batch"], cfg["seed"], 200, 50
    r = R.search("C")
    base, _ = R.terrain()
    data, O = R.terrain("box1")
    T = engine.Terrain.from_data(base, storage=L.STORAGE_F64)   # box 1's heights are not floats
    ws = engine.PlanWorkspace(T, batch)
    st = apply(T, data.z, _box_rect(base.z, data.z), dev=True)
    torch.cuda.synchronize()   # the prune below runs on the handle's own stream
    assert int(st[0]) == 0
    exp = R.expected("C", "box1")
    start, goal = R.start_goal()
    trees = []
    for name, direction in (("a", L.FORWARD), ("b", L.REVERSE)):
        dt = engine.DeviceTree(r[name]["v"][0], capacity=1 << 16)
        dt.load(r[name]["v"], r[name]["act"], r[name]["parent"])
        dt.revalidate(T, direction)
        trees.append(dt)
    ta, tb = trees
    L.check(lib.gbp_plan_reset(ws._h, int(r["ext_counter"]), _stream(0)), "plan_reset")
    st = None
    for half in range(first, first + halves, 2):
        ws.halves(T, ta, tb, half, 2, batch, seed=seed)
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
            ws.halves(T, ta, tb, h0, half + 2 - h0, batch, seed=seed, first_stage=resume.value)
            st = ws.status()
        assert not st["error"], st["error"]
        if st["done"]:
            break
    ref_init = tuple({k: e[0][k] for k in ("v", "act", "parent")} for e in exp)
    ref = O.plan(start, goal, init_trees=ref_init, nthreads=16, batch=batch, seed=seed,
                 max_halves=halves, first_half=first, extend_base=r["ext_counter"])
    assert bool(st["done"]) == bool(ref["found"])
    for dt, name in zip(trees, "ab"):
        s, a, p, g = dt.read()
        assert len(p) > len(ref_init["ab".index(name)]["parent"])   # the search went on
        assert_same_tree(dict(v=s, act=a, parent=p, g=g), ref[name], ("continued", name))
    assert st["stat_targets"] == ref["targets"] and st["ext_counter"] == ref["ext_counter"]


# ---- 9: the C++ surface ---------------------------------------------------------------------
def test_fast_terrain_map_update_calls(gpu, tmp_path):
    """tests/integration/terrain_update.cpp: updateFromGridMap keeps the handle
    on an unchanged geometry and reloads on a changed one, updateDataFlat /
    updateData patch in place; getGroundHeight equals a freshly loaded map."""
    from tests.test_abi import build_node_callsite
    exe = build_node_callsite(tmp_path / "terrain_update", src="terrain_update.cpp")
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert "terrain_update ok" in r.stdout
