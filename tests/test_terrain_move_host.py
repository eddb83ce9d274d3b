"""The engine-free part of a terrain window moved by whole cells
(csrc/host/gbp_terrain_patch.cpp: move_rects, shift_mirror,
nan_free_after_move, detect_shift), without a device.

As tests/test_terrain_patch.py: a stand-alone program
(tests/native/terrain_move_probe.cpp) built with AddressSanitizer and UBSan
from its own source only, run on heap arrays of exactly the stated sizes and
compared with a numpy restatement.  Nothing is loaded into Python under a
sanitizer.
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from tests.helpers import bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "global_body_planner_amd", "csrc", "host")
SHAPES = [(5, 4), (2, 2)]
TOL = 1.0 / 1024   # FastTerrainMap::moveFromGridMap's stated condition


def hexes(a):
    return " ".join(float(v).hex() for v in np.asarray(a, np.float64).ravel())


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("move")
    exe = str(d / "terrain_move_probe")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe,
                    os.path.join(HERE, "native", "terrain_move_probe.cpp"),
                    os.path.join(HOST, "gbp_terrain_patch.cpp")], check=True)

    def run(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True,
                           text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return [o.split() for o in out]
    return run


def shifts(nx, ny):
    return list(itertools.product(range(-nx - 1, nx + 2), range(-ny - 1, ny + 2)))


def moved(old, src, sx, sy):
    """The numpy restatement: new[ix, iy] = old[ix + sx, iy + sy] where the old
    map has that cell, src elsewhere; and the mask of the cells taken from src."""
    nx, ny = old.shape
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    jx, jy = ix + sx, iy + sy
    inside = (jx >= 0) & (jx < nx) & (jy >= 0) & (jy < ny)
    new = src.copy()
    new[inside] = old[jx[inside], jy[inside]]
    return new, ~inside


def move_cases(nx, ny, olds, srcs, storage=L.STORAGE_F64):
    return [f"M {nx} {ny} {sx} {sy} {storage} {hexes(o)} {hexes(s)}"
            for (sx, sy), o, s in zip(shifts(nx, ny), olds, srcs)]


def parse_move(tok, nx, ny):
    v = [int(t) for t in tok[:14]]
    rects = [tuple(v[5 + 4 * k:9 + 4 * k]) for k in range(v[4])]
    m = np.array([float.fromhex(t) for t in tok[14:]]).reshape(nx, ny)
    return tuple(v[:4]), rects, v[13], m


def same(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


@pytest.mark.parametrize("shape", SHAPES)
def test_rectangles_partition_the_map_and_the_mirror_shift(probe, shape):
    """Every (sx, sy) in [-nx-1, nx+1] x [-ny-1, ny+1]: the overlap and the one
    or two strips cover every cell exactly once, the overlap is the set of
    cells with an old counterpart, the L is |sx| full rows and |sy| columns of
    the remaining rows, and the shifted mirror equals numpy's."""
    nx, ny = shape
    old = 100.0 + 10.0 * np.arange(nx)[:, None] + np.arange(ny)[None, :]
    src = -old
    sh = shifts(nx, ny)
    assert len(sh) == (2 * nx + 3) * (2 * ny + 3)
    out = probe(move_cases(nx, ny, [old] * len(sh), [src] * len(sh)))
    for (sx, sy), tok in zip(sh, out):
        ov, strips, nf, m = parse_move(tok, nx, ny)
        want, from_src = moved(old, src, sx, sy)
        cover = np.zeros(shape, int)
        if ov[2] > 0 and ov[3] > 0:
            cover[ov[0]:ov[0] + ov[2], ov[1]:ov[1] + ov[3]] += 1
        in_strip = np.zeros(shape, int)
        for r in strips:
            assert r[2] > 0 and r[3] > 0 and r[0] >= 0 and r[1] >= 0, (sx, sy, r)
            assert r[0] + r[2] <= nx and r[1] + r[3] <= ny, (sx, sy, r)
            in_strip[r[0]:r[0] + r[2], r[1]:r[1] + r[3]] += 1
        assert np.array_equal(cover + in_strip, np.ones(shape, int)), (sx, sy)
        assert np.array_equal(in_strip.astype(bool), from_src), (sx, sy)
        if abs(sx) >= nx or abs(sy) >= ny:
            assert strips == [(0, 0, nx, ny)], (sx, sy)
        else:
            want_strips = []
            if sx:
                want_strips.append((0 if sx < 0 else nx - sx, 0, abs(sx), ny))
            if sy:
                want_strips.append((max(-sx, 0), 0 if sy < 0 else ny - sy, nx - abs(sx), abs(sy)))
            assert strips == want_strips, (sx, sy)
        assert same(m, want), (sx, sy)
        assert nf == 1


def test_an_fp32_handle_s_mirror_takes_the_strips_rounded_to_float(probe):
    nx, ny = 5, 4
    rng = np.random.default_rng(5)
    old = rng.uniform(-1, 1, (nx, ny)).astype(np.float32).astype(np.float64)
    src = rng.uniform(-1, 1, (nx, ny))
    sh = shifts(nx, ny)
    out = probe(move_cases(nx, ny, [old] * len(sh), [src] * len(sh), L.STORAGE_F32))
    for (sx, sy), tok in zip(sh, out):
        _, _, _, m = parse_move(tok, nx, ny)
        want, _ = moved(old, src.astype(np.float32).astype(np.float64), sx, sy)
        assert same(m, want), (sx, sy)


@pytest.mark.parametrize("shape", SHAPES)
def test_nan_free_after_a_move_equals_a_full_scan(probe, shape):
    """One NaN at every position of the old map (it leaves with a strip or
    stays), and one at every position of the source (read only when a strip
    holds it), for every shift."""
    nx, ny = shape
    base = 1.0 + np.arange(nx * ny, dtype=np.float64).reshape(nx, ny)
    sh = shifts(nx, ny)
    n_true = n_false = 0
    for where in ("old", "src"):
        for pos in itertools.product(range(nx), range(ny)):
            old, src = base.copy(), -base
            (old if where == "old" else src)[pos] = np.nan
            out = probe(move_cases(nx, ny, [old] * len(sh), [src] * len(sh)))
            for (sx, sy), tok in zip(sh, out):
                _, _, nf, m = parse_move(tok, nx, ny)
                want, _ = moved(old, src, sx, sy)
                assert same(m, want), (where, pos, sx, sy)
                assert nf == int(not np.isnan(want).any()), (where, pos, sx, sy)
                n_true += nf
                n_false += 1 - nf
    assert n_true > 0 and n_false > 0


def detect(probe, cases):
    out = probe([f"D {len(o)} {float(TOL).hex()} {hexes(o)} {hexes(n)}" for o, n in cases])
    return [(int(t[0]), int(t[1])) for t in out]


def flip_last_bit(a):
    b = np.asarray(a, np.float64).copy().view(np.uint64)
    b ^= np.uint64(1)
    return b.view(np.float64)


def test_shift_detection(probe):
    """TOL = 1 / 1024 of a cell, the condition moveFromGridMap states: exact
    shifts and shifts whose positions differ in the last bit are accepted with
    the right count; a displacement of h / 512 and a changed spacing are not."""
    n, h = 37, 0.02
    old = -1.3 + h * np.arange(n)
    ks = list(range(-n - 1, n + 2))
    exact = [(old, -1.3 + h * (np.arange(n) + k)) for k in ks]
    assert detect(probe, exact) == [(1, k) for k in ks]
    ulp = [(old, flip_last_bit(nw)) for _, nw in exact]
    assert detect(probe, ulp) == [(1, k) for k in ks]
    # grid_map's way: positions recomputed from a new centre
    centre = [(old, (-1.3 + h * k) + h * np.arange(n)) for k in ks]
    assert detect(probe, centre) == [(1, k) for k in ks]
    inside = [k for k in ks if abs(k) < n]      # some position has an old counterpart
    off = [(old, -1.3 + h * (np.arange(n) + k) + h / 512) for k in inside]
    assert detect(probe, off) == [(0, 0)] * len(inside)
    neg = [(old, -1.3 + h * (np.arange(n) + k) - h / 512) for k in inside]
    assert detect(probe, neg) == [(0, 0)] * len(inside)
    half = [(old, old + h / 2)]
    spacing = [(old, -1.3 + 1.01 * h * np.arange(n)), (old, -1.3 + 0.5 * h * np.arange(n)),
               (old, -1.3 + h * 3 + 1.001 * h * np.arange(n))]
    assert detect(probe, half + spacing) == [(0, 0)] * 4
    # one displaced entry, NaN, a degenerate old vector, the smallest map
    one = old.copy()
    one[17] += h / 100
    nan = old.copy()
    nan[5] = np.nan
    assert detect(probe, [(old, one), (old, nan), (np.zeros(4), np.zeros(4))]) == [(0, 0)] * 3
    assert detect(probe, [(np.array([0.0, 1.0]), np.array([1.0, 2.0])),
                          (np.array([0.0, 1.0]), np.array([0.25, 1.25]))]) == [(1, 1), (0, 0)]


def test_the_library_s_detection_is_the_probe_s(probe):
    lib = L.load()
    old = 0.5 + 0.02 * np.arange(11)
    for new, want in ((0.5 + 0.02 * (np.arange(11) - 3), (1, -3)), (old + 0.001, (0, 0))):
        sh = ctypes.c_int(0)
        ok = lib.gbp_coord_shift(old.ctypes.data_as(ctypes.c_void_p),
                                 new.ctypes.data_as(ctypes.c_void_p), 11, TOL, ctypes.byref(sh))
        assert (ok, sh.value) == want == detect(probe, [(old, new)])[0]


def test_the_entry_refuses_a_null_handle():
    lib = L.load()
    a = np.zeros(4)
    p = a.ctypes.data_as(ctypes.c_void_p)
    assert lib.gbp_terrain_move_host(None, 1, 0, p, p, L.SRC_F64_XMAJOR, 2, p, None, None,
                                     None) == L.E_BAD_HANDLE
