"""The slope rule (csrc/gbp_slopes.h) on the host, without a device.

`restate` is the numpy restatement of the rule in the same operation order:
per axis a central difference where both neighbours are usable (in the map,
height not NaN), a one-sided one where one is, 0.0 where none is; then l =
sqrt((gx gx + gy gy) + 1) and (-gx / l, -gy / l, 1 / l); a NaN node reads
(0, 0, 1); SLOPES_F32 rounds each component through float last.  The GPU tests
(tests/test_gpu_slopes.py) take their expected values from it as well.

The header is built into a stand-alone program (tests/native/slopes_probe.cpp)
with AddressSanitizer and UBSan and compared with the restatement as uint64,
NaN results included: both run on the host.  (The GPU tests let any NaN equal
any NaN, tests.helpers.same_f64: IEEE 754 leaves the sign and payload of a
generated NaN open, and inf - inf or 0 / 0 give different ones on x86 and
gfx950.)
"""
import os
import subprocess

import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from global_body_planner_amd import terrain_data as td
from tests.helpers import bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "global_body_planner_amd", "csrc")


def _axis(z, c, axis):
    """One axis' gradient of z [nx][ny] with coordinates c along `axis`."""
    z = np.moveaxis(z, axis, 0)
    n = z.shape[0]
    zm, zp = np.full_like(z, np.nan), np.full_like(z, np.nan)  # outside the map: not usable
    zm[1:], zp[:-1] = z[:-1], z[1:]
    cm, cp = np.full(n, np.nan), np.full(n, np.nan)
    cm[1:], cp[:-1] = c[:-1], c[1:]
    shape = (n,) + (1,) * (z.ndim - 1)
    cm, cc, cp = cm.reshape(shape), np.asarray(c, np.float64).reshape(shape), cp.reshape(shape)
    um, up = ~np.isnan(zm), ~np.isnan(zp)
    with np.errstate(all="ignore"):
        both = (zp - zm) / (cp - cm)
        fwd = (zp - z) / (cp - cc)
        bwd = (z - zm) / (cc - cm)
    g = np.where(um & up, both, np.where(up, fwd, np.where(um, bwd, 0.0)))
    return np.moveaxis(g, 0, axis)


def restate(x, y, z, f32=False):
    """(dx, dy, dz) of the rule for heights z [nx][ny] as the handle stores them."""
    z = np.asarray(z, np.float64)
    gx, gy = _axis(z, np.asarray(x, np.float64), 0), _axis(z, np.asarray(y, np.float64), 1)
    with np.errstate(all="ignore"):
        l = np.sqrt((gx * gx + gy * gy) + 1.0)
        n = [(-gx) / l, (-gy) / l, 1.0 / l]
        if f32:
            n = [v.astype(np.float32).astype(np.float64) for v in n]
    nan = np.isnan(z)
    return tuple(np.ascontiguousarray(np.where(nan, fill, v)) for v, fill in zip(n, (0.0, 0.0, 1.0)))


def uniform(n, h=0.02, o=0.0):
    return o + np.arange(n, dtype=np.float64) * h


def rough(nx, ny, seed, f32=True):
    """Heights with slopes of order 1 over a 0.02 grid, float-representable when f32."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(-0.02, 0.02, (nx, ny)) + 0.1 * np.sin(np.arange(nx) / 3.0)[:, None]
    return z.astype(np.float32).astype(np.float64) if f32 else z


def graded(n, seed):
    """Ascending coordinates with a different spacing at every step."""
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.uniform(0.01, 0.03, n))


def cases():
    """name -> (x, y, z): the maps of the issue's list (every height
    float-representable unless the name says f64)."""
    out = {}
    for nx, ny in ((2, 2), (3, 2), (5, 4)):
        out[f"{nx}x{ny}"] = (uniform(nx), uniform(ny, 0.02, -0.04), rough(nx, ny, nx * 10 + ny))
    x, y, z = out["5x4"]
    for i in range(5):
        for j in range(4):
            zz = z.copy()
            zz[i, j] = np.nan
            out[f"5x4-nan-{i}-{j}"] = (x, y, zz)
    zz = z.copy()
    zz[1:3, 1:3] = np.nan
    out["5x4-nan-block"] = (x, y, zz)
    out["5x4-all-nan"] = (x, y, np.full((5, 4), np.nan))
    out["5x4-flat"] = (x, y, np.full((5, 4), 0.25))
    out["37x29-graded"] = (graded(37, 1), graded(29, 2), rough(37, 29, 3))
    xr, yr = graded(37, 4), graded(29, 5)
    xr[11], yr[0], yr[28] = xr[10], yr[1], yr[27]  # repeated: interior, first, last
    xr[21] = xr[20] = xr[19]                       # three in a row: a central difference over 0
    out["37x29-repeated"] = (xr, yr, rough(37, 29, 6))
    zi = rough(37, 29, 7)
    zi[5, 5], zi[5, 7], zi[20, 10], zi[21, 10], zi[0, 0], zi[36, 28] = (np.inf, np.inf, np.inf, -np.inf,
                                                                        -np.inf, np.inf)
    zi[30, 3], zi[30, 4] = np.nan, np.inf
    out["37x29-inf"] = (graded(37, 8), graded(29, 9), zi)
    out["37x29-f64"] = (graded(37, 10), graded(29, 11), rough(37, 29, 12, f32=False))
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("slopes")
    exe = str(d / "slopes_probe")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-sanitize=float-divide-by-zero",
                    "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, "-o", exe, os.path.join(HERE, "native", "slopes_probe.cpp")],
                   check=True)

    def run(maps):
        """maps: [(x, y, z, flags)] -> [(dx, dy, dz)]"""
        hexs = lambda a: " ".join(float(v).hex() for v in np.asarray(a, np.float64).ravel())
        text = "".join(f"{len(x)} {len(y)} {fl}\n{hexs(x)}\n{hexs(y)}\n{hexs(z)}\n"
                       for x, y, z, fl in maps)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        lines = r.stdout.splitlines()
        assert len(lines) == 3 * len(maps)
        out = []
        for k, (x, y, z, fl) in enumerate(maps):
            out.append(tuple(np.array([int(t, 16) for t in lines[3 * k + c].split()], np.uint64)
                             .view(np.float64).reshape(len(x), len(y)) for c in range(3)))
        return out
    return run


def assert_layers(got, want, label):
    for name, g, w in zip(("dx", "dy", "dz"), got, want):
        ok = bits(g) == bits(w)
        assert ok.all(), (label, name, np.argwhere(~ok)[:5].tolist())


@pytest.mark.parametrize("f32", [False, True])
def test_the_header_equals_the_restatement(probe, f32):
    flags = L.SLOPES_F32 if f32 else 0
    cs = cases()
    got = probe([(x, y, z, flags) for x, y, z in cs.values()])
    for (name, (x, y, z)), g in zip(cs.items(), got):
        assert_layers(g, restate(x, y, z, f32), (name, f32))


def test_the_rule_on_cases_worked_by_hand():
    """The restatement itself: signs, the one-sided rule, the NaN node."""
    x, y = uniform(3, 0.5), uniform(3, 0.5)
    z = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [4.0, 4.0, 4.0]])  # a slope along x only
    dx, dy, dz = restate(x, y, z)
    # edges one-sided (2, 6), the middle row central (4); gy = 0 gives -0.0
    for i, g in enumerate((2.0, 4.0, 6.0)):
        l = np.sqrt(g * g + 1.0)
        assert np.all(dx[i] == -g / l) and np.all(dz[i] == 1.0 / l)
    assert np.all(dy == 0.0) and np.all(np.signbit(dy))
    flat = restate(x, y, np.zeros((3, 3)))
    assert np.all(np.signbit(flat[0])) and np.all(np.signbit(flat[1])) and np.all(flat[2] == 1.0)
    z[1, 1] = np.nan
    dx, dy, dz = restate(x, y, z)
    assert (dx[1, 1], dy[1, 1], dz[1, 1]) == (0.0, 0.0, 1.0) and not np.signbit(dx[1, 1])
    assert dx[0, 1] == 0.0 and np.signbit(dx[0, 1])  # (0, 1): neither x neighbour usable
    assert dx[2, 1] == 0.0 and np.isfinite(dx).all()
    # (1, 0) beside the NaN along y: one-sided towards... the map edge: none usable
    assert dy[1, 0] == 0.0 and dx[1, 0] == -4.0 / np.sqrt(17.0)


def test_the_restatement_reproduces_synth_fractal_257():
    t = td.by_name("synth-fractal-257")
    got = restate(t.x, t.y, t.z, f32=True)
    for name, g, w in zip(("dx", "dy", "dz"), got, (t.dx, t.dy, t.dz)):
        assert np.all(g == w), name
