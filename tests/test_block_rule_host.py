"""The workgroup size of the persistent validate launch,
host side, no device: gbp_validate_lds_plan with block 0 answers for a caller
who has not set GBP_OPT_BLOCK, with a block for one who has.

The LDS of a launch is the staged coordinate vectors (8 (nx + ny) bytes, when
they are staged) and, per wave, 64 rows of 19 doubles and a ring of 128
16-byte records: 11,776 B.  From the bytes the plan returns, the block it
sized for follows.
"""
import ctypes

import pytest

from global_body_planner_amd import _lib as L

CU_LDS = 160 * 1024
PER_WAVE = 8 * 19 * 64 + 16 * 128


def plan(nxy, block, waves, limit=CU_LDS):
    lib = L.load()
    cm, pf, nbytes = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(0)
    rc = lib.gbp_validate_lds_plan(nxy, nxy, block, waves, limit, ctypes.byref(cm), ctypes.byref(pf),
                                   ctypes.byref(nbytes))
    assert rc == 0, rc
    return cm.value, pf.value, nbytes.value


def block_of(nxy, cm, pf, nbytes):
    """The block a plan without a window sized its rows for."""
    assert pf == 0
    rows = nbytes - (8 * 2 * nxy if cm else 0)
    assert rows % PER_WAVE == 0, rows
    return 64 * (rows // PER_WAVE)


def has_window():
    return plan(256, 256, 1)[1] > 0


def test_128_lanes_at_1024():
    """128 lanes, 2 waves per SIMD, 1024^2: the coordinates stay staged, a
    workgroup asks for at most 40,960 B and four of them fit a CU."""
    cm, pf, nbytes = plan(1024, 128, 2)
    assert cm == 1
    assert nbytes <= 40960
    assert 4 * nbytes <= 163840
    if not pf:
        assert nbytes == 16384 + 2 * PER_WAVE


@pytest.mark.parametrize("nxy", [256, 1024])
def test_unset_block_is_128_where_it_fits(nxy):
    """Block not set, 2 waves per SIMD: the plan is the 128-lane one, coordinate mode 1."""
    assert plan(nxy, 0, 2) == plan(nxy, 128, 2)
    cm, pf, nbytes = plan(nxy, 0, 2)
    assert cm == 1 and 4 * nbytes <= 163840
    if not has_window():
        assert block_of(nxy, cm, pf, nbytes) == 128


def test_unset_block_keeps_256_at_4096():
    """4096^2: four workgroups with their 64 KB of coordinate vectors do not
    fit a CU, so the rule keeps 256 lanes (and the coordinates out of LDS, as before)."""
    assert plan(4096, 0, 2) == plan(4096, 256, 2)
    assert plan(4096, 0, 2)[0] == 0
    if not has_window():
        assert block_of(4096, *plan(4096, 0, 2)) == 256


def test_unset_block_keeps_256_at_four_waves():
    """OPT_WAVES 4: eight 128-lane workgroups with staged coordinates do not fit;
    256 lanes and coordinate mode 0, as before."""
    assert plan(1024, 0, 4) == plan(1024, 256, 4)
    assert plan(1024, 0, 4)[0] == 0


@pytest.mark.parametrize("block", [64, 128, 256, 512])
def test_explicit_block_is_honoured(block):
    cm, pf, nbytes = plan(1024, block, 2)
    if not has_window():
        assert block_of(1024, cm, pf, nbytes) == block
    # the modes the 256-lane launches had before the rule
    if block == 256:
        assert cm == 1 and plan(256, 256, 2)[0] == 1 and plan(1024, 256, 4)[0] == 0


def test_bad_blocks_rejected():
    lib = L.load()
    for block in (-64, 32, 100, 576):
        assert lib.gbp_validate_lds_plan(256, 256, block, 2, CU_LDS, None, None, None) != 0
