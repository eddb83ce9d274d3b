"""`no height of the map is NaN`, the fact a terrain handle keeps for the
validate kernel's state check without NaN tests (GBP_OPT_NAN_FREE), without a
device: the scan of gbp_terrain_create and the rule behind every write of the
host mirror (csrc/host/gbp_terrain_patch.cpp: nan_free, nan_free_after).

Built into a stand-alone program (tests/native/nan_free_probe.cpp) with
AddressSanitizer and UBSan from its own source only, as
tests/test_terrain_patch.py does.  The program keeps one mirror through a
sequence of patches; after each the fact must equal numpy's scan of the same
mirror.
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

from global_body_planner_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "global_body_planner_amd", "csrc", "host")
NX, NY = 5, 4
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("nanfree")
    exe = str(d / "nan_free_probe")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe,
                    os.path.join(HERE, "native", "nan_free_probe.cpp"),
                    os.path.join(HOST, "gbp_terrain_patch.cpp")], check=True)

    def run(z0, patches, storage=L.STORAGE_F64):
        """z0 [nx][ny], patches: (ix0, iy0, values [pnx][pny]) applied in order ->
        [(rc, fact)]: the create scan first, then one entry per patch."""
        z0 = np.asarray(z0, np.float64)
        lines = [" ".join(float(v).hex() for v in z0.ravel())]
        for ix0, iy0, vals in patches:
            vals = np.asarray(vals, np.float64)
            lines.append(f"{ix0} {iy0} {vals.shape[0]} {vals.shape[1]} "
                         + " ".join(float(v).hex() for v in vals.ravel()))
        r = subprocess.run([exe, str(z0.shape[0]), str(z0.shape[1]), str(storage)],
                           input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = [tuple(int(t) for t in line.split()) for line in r.stdout.splitlines()]
        assert len(out) == 1 + len(patches)
        return out
    return run


def z_finite():
    return 100.0 + 10.0 * np.arange(NX)[:, None] + np.arange(NY)[None, :]


def test_create_scan(probe):
    """Every position of a single NaN, none, and infinities (heights like any other)."""
    assert probe(z_finite(), []) == [(0, 1)]
    for ix, iy in itertools.product(range(NX), range(NY)):
        z = z_finite()
        z[ix, iy] = NAN
        assert probe(z, []) == [(0, 0)], (ix, iy)
    z = z_finite()
    z[0, 0], z[NX - 1, NY - 1] = INF, -INF
    assert probe(z, []) == [(0, 1)]
    # an fp32 handle's mirror: a NaN stays one, 1e300 becomes inf, not NaN
    z = z_finite()
    z[2, 1] = 1e300
    assert probe(z, [], L.STORAGE_F32) == [(0, 1)]
    z[2, 2] = NAN
    assert probe(z, [], L.STORAGE_F32) == [(0, 0)]


def test_patch_rule(probe):
    """Finite patch keeps the fact, NaN patch clears it, overwriting the only
    NaN restores it; with two NaNs the fact returns only with the second."""
    one = np.array([[NAN]])
    fin = np.array([[1.5, 2.5], [3.5, INF]])
    got = probe(z_finite(), [
        (1, 1, fin),                     # finite (and an infinity) into a NaN-free map: kept
        (2, 2, one),                     # a NaN: cleared
        (0, 0, fin),                     # finite elsewhere: still a NaN in the map
        (2, 2, [[7.0]]),                 # the only NaN overwritten: restored
        (4, 3, one), (0, 0, one),        # two NaNs, in the map's last and first cell
        (4, 3, [[1.0]]),                 # one of them overwritten: still 0
        (0, 0, np.full((NX, NY), 2.0)),  # the whole map: restored
        (3, 0, [[1.0, NAN, 2.0, 3.0]]),  # a NaN inside a row of the rectangle
        (3, 1, [[NAN]]),                 # NaN over NaN
        (3, 1, [[0.0]]),
    ])
    assert got == [(0, 1), (0, 1), (0, 0), (0, 0), (0, 1), (0, 0), (0, 0), (0, 0), (0, 1), (0, 0),
                   (0, 0), (0, 1)]


def test_rejected_patch_keeps_the_fact(probe):
    """A patch an fp32 handle cannot hold (0.1 is not float-representable) is
    rejected whole: its NaN is not written, the fact stays."""
    got = probe(z_finite(), [(1, 1, [[0.1, NAN]]), (1, 1, [[0.5, NAN]]), (0, 0, [[0.1]])],
                L.STORAGE_F32)
    assert got == [(0, 1), (L.E_UNSUPPORTED, 1), (0, 0), (L.E_UNSUPPORTED, 0)]
    got = probe(z_finite(), [(4, 3, np.zeros((2, 1)))])   # leaves the map
    assert got == [(0, 1), (L.E_SHAPE, 1)]


@pytest.mark.parametrize("storage", [L.STORAGE_F32, L.STORAGE_F64])
def test_random_patch_sequences_equal_a_full_scan(probe, storage):
    """200 random rectangles in sequence, a NaN in about a third of them (often
    on the rectangle's edge), patches that cover earlier NaNs among them: after
    each the fact equals numpy's scan of the mirror."""
    rng = np.random.default_rng(20261020 + storage)
    z = z_finite()
    m = z.copy()
    patches, want = [], [int(not np.isnan(m).any())]
    for _ in range(200):
        a, b = sorted(rng.choice(NX + 1, 2, replace=False))
        c, d = sorted(rng.choice(NY + 1, 2, replace=False))
        vals = rng.integers(-4000, 4000, (b - a, d - c)) / 8.0
        if rng.random() < 0.35:
            vals[rng.integers(b - a), rng.integers(d - c)] = NAN
        patches.append((a, c, vals))
        m[a:b, c:d] = vals
        want.append(int(not np.isnan(m).any()))
    got = probe(z, patches, storage)
    assert [g[0] for g in got] == [0] * len(got)
    assert [g[1] for g in got] == want
    assert 20 < sum(want) < 180   # both values and both transitions occur
