"""The engine-free part of an in-place terrain update
(csrc/host/gbp_terrain_patch.cpp), without a device.

It is built into a stand-alone program (tests/native/terrain_patch_probe.cpp)
with AddressSanitizer and UBSan from its own source only: it links no engine.
For every rectangle of a 5 x 4 map and both source layouts the mirror scatter,
the pair-row range and the round-trip check run on heap arrays of exactly the
stated sizes and are compared with numpy.
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
NX, NY = 5, 4


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("patch")
    exe = str(d / "terrain_patch_probe")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe,
                    os.path.join(HERE, "native", "terrain_patch_probe.cpp"),
                    os.path.join(HOST, "gbp_terrain_patch.cpp")], check=True)

    def run(cases, storage, nx=NX, ny=NY):
        """cases: (ix0, iy0, pnx, pny, layout, ld, flat source array) ->
        per case (rc, p0, p1, round_trips, mirror [nx][ny])."""
        text = "".join(
            f"{c[0]} {c[1]} {c[2]} {c[3]} {c[4]} {c[5]} {len(c[6])} "
            + " ".join(float(v).hex() for v in c[6]) + "\n" for c in cases)
        r = subprocess.run([exe, str(nx), str(ny), str(storage)], input=text, capture_output=True,
                           text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = []
        for line in r.stdout.splitlines():
            tok = line.split()
            out.append((int(tok[0]), int(tok[1]), int(tok[2]), int(tok[3]),
                        np.array([float.fromhex(t) for t in tok[4:]]).reshape(nx, ny)))
        assert len(out) == len(cases)
        return out
    return run


def rects(nx=NX, ny=NY):
    for (a, b), (c, d) in itertools.product(itertools.combinations(range(nx + 1), 2),
                                            itertools.combinations(range(ny + 1), 2)):
        yield a, c, b - a, d - c


def mirror0(nx=NX, ny=NY):
    return 100.0 + 10.0 * np.arange(nx)[:, None] + np.arange(ny)[None, :]


def source(rect, layout, rng, nx=NX, ny=NY):
    """(ld, flat source of exactly the size the layout needs, the rectangle's
    values [pnx][pny]); float-representable values with a NaN among them."""
    ix0, iy0, pnx, pny = rect
    if layout == L.SRC_F64_XMAJOR:
        ld = pny + 1
        flat = np.full((pnx - 1) * ld + pny, -777.0)
        vals = rng.integers(-4000, 4000, (pnx, pny)) / 8.0
        vals[rng.integers(pnx), rng.integers(pny)] = np.nan
        for i in range(pnx):
            flat[i * ld:i * ld + pny] = vals[i]
        return ld, flat, vals
    ld = nx + 1
    flat = (rng.integers(-4000, 4000, (ny - 1) * ld + nx) / 8.0).astype(np.float32)
    flat[rng.integers(flat.size)] = np.nan
    ix, iy = np.meshgrid(np.arange(ix0, ix0 + pnx), np.arange(iy0, iy0 + pny), indexing="ij")
    return ld, flat, flat[(nx - 1 - ix) + (ny - 1 - iy) * ld].astype(np.float64)


def test_there_are_150_rectangles():
    assert len(list(rects())) == 150


@pytest.mark.parametrize("layout", [L.SRC_F64_XMAJOR, L.SRC_F32_GRIDMAP])
@pytest.mark.parametrize("storage", [L.STORAGE_F32, L.STORAGE_F64])
def test_every_rectangle_scatter_pair_rows_and_check(probe, layout, storage):
    rng = np.random.default_rng(20251017 + layout)
    cases, want = [], []
    for rect in rects():
        ld, flat, vals = source(rect, layout, rng)
        cases.append((*rect, layout, ld, flat))
        m = mirror0()
        m[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]] = vals
        want.append(m)
    for rect, (rc, p0, p1, rt, m), w in zip(rects(), probe(cases, storage), want):
        assert rc == 0 and rt == 1, rect
        assert (p0, p1) == (max(rect[0] - 1, 0), min(rect[0] + rect[2], NX - 1)), rect
        both = np.isnan(m) & np.isnan(w)
        assert np.array_equal(bits(m)[~both], bits(w)[~both]) and \
            np.array_equal(np.isnan(m), np.isnan(w)), rect


def test_pair_rows_hold_every_copy_of_the_rectangle():
    """The range the probe reports is the rule of DESIGN section 4: cell row ix
    lies in slot 0 of pair row ix (ix < NX - 1) and slot 1 of pair row ix - 1."""
    for ix0, _, pnx, _ in rects():
        rows = set()
        for ix in range(ix0, ix0 + pnx):
            if ix < NX - 1:
                rows.add(ix)
            if ix > 0:
                rows.add(ix - 1)
        assert rows == set(range(max(ix0 - 1, 0), min(ix0 + pnx, NX - 1)))


def test_rejected_patches_leave_the_mirror_untouched(probe):
    """An fp64 value that is neither NaN nor float-representable rejects the
    whole patch for an fp32 handle (GBP_E_UNSUPPORTED) and is stored as it is
    by an fp64 handle."""
    rng = np.random.default_rng(7)
    cases, where = [], []
    for rect in rects():
        ld, flat, vals = source(rect, L.SRC_F64_XMAJOR, rng)
        i, j = rng.integers(rect[2]), rng.integers(rect[3])
        flat[i * ld + j] = 0.1
        cases.append((*rect, L.SRC_F64_XMAJOR, ld, flat))
        where.append((rect[0] + i, rect[1] + j))
    for rect, (rc, _, _, rt, m) in zip(rects(), probe(cases, L.STORAGE_F32)):
        assert rc == L.E_UNSUPPORTED and rt == 0, rect
        assert np.array_equal(bits(m), bits(mirror0())), rect
    for (ix, iy), (rc, _, _, rt, m) in zip(where, probe(cases, L.STORAGE_F64)):
        assert rc == 0 and rt == 0
        assert m[ix, iy] == 0.1


def test_bad_rectangles_layouts_and_leading_dimensions(probe):
    z = np.zeros(64)
    f = np.zeros(64, np.float32)
    bad = [(0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 2, 2), (0, -1, 2, 2), (4, 0, 2, 1), (0, 3, 1, 2),
           (5, 0, 1, 1), (0, 4, 1, 1), (0, 0, 6, 4), (0, 0, 5, 5), (2**31 - 1, 0, 2, 1)]
    out = probe([(*r, L.SRC_F64_XMAJOR, 8, z) for r in bad], L.STORAGE_F32)
    for r, o in zip(bad, out):
        assert o[0] == L.E_SHAPE, r
        assert np.array_equal(bits(o[4]), bits(mirror0()))
    out = probe([(0, 0, 2, 2, 2, 8, z), (0, 0, 2, 2, -1, 8, z),       # unknown layouts
                 (0, 0, 2, 3, L.SRC_F64_XMAJOR, 2, z),               # ld < pny
                 (0, 0, 2, 2, L.SRC_F32_GRIDMAP, NX - 1, f)], L.STORAGE_F32)  # ld < NX
    assert [o[0] for o in out] == [L.E_INVALID_ARG, L.E_INVALID_ARG, L.E_SHAPE, L.E_SHAPE]


def test_entries_refuse_a_null_handle():
    lib = L.load()
    r = L.Rect(0, 0, 1, 1)
    z = np.zeros(1)
    p = z.ctypes.data_as(ctypes.c_void_p)
    assert lib.gbp_terrain_update_dev(None, ctypes.byref(r), 0, 1, p, None, None, None, None,
                                      None) == L.E_BAD_HANDLE
    assert lib.gbp_terrain_update_host(None, ctypes.byref(r), 0, 1, p, None, None,
                                       None) == L.E_BAD_HANDLE
    assert lib.gbp_terrain_read_host(None, ctypes.byref(r), 0, p) == L.E_BAD_HANDLE
