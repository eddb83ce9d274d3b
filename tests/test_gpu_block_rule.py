"""The persistent validate launch's workgroup size (128 lanes where four
workgroups fit a CU with their coordinate vectors, GBP_OPT_BLOCK as given once
it is set; GBP_OPT_LAUNCH_BLOCK reports it), each wave's first fill, and the
coordinate staging in 16-byte pieces.

Bar: at blocks 128 and 256 and with the block not set, `valid`, `flags`,
`counts`, and `t_new` / `s_new` where their *_SET flags say they are assigned,
of k_validate_persistent equal k_validate_direct's bit for bit; for n <= 4096
the oracle's as well (FRAGILE attempts re-decided on the host, as the product
does).  The batch sizes put every first-fill case in front of the kernel: empty
slices (n = 1, 2, 3), a first fill of 63 / 64 / 65 in one wave, one attempt per
wave and one more, the first fill exactly full for every wave of the full grid,
one short of it, one refill after it, and two refills with uneven slices.
"""
import ctypes

import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from global_body_planner_amd import terrain_data as td
from global_body_planner_amd import workload as W
from tests.helpers import assert_pairs_equal, resolver, same_f64, u32
from tests.test_gpu_refill_window import assert_same, run

torch = pytest.importorskip("torch")

WAVE = 64
NAME = "synth-rough-256"
BLOCKS = [128, 256, 0]   # 0: GBP_OPT_BLOCK not set
_cache = {}


def waves_of(T, n):
    """Waves of the persistent launch for n attempts, as launch_validate_w sizes it."""
    block = T.get_option(L.OPT_LAUNCH_BLOCK)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    resident = cus * max(1, T.get_option(L.OPT_WAVES) * 256 // block)
    return max(1, min(resident, (n + WAVE - 1) // WAVE)) * (block // WAVE)


def setup():
    """(Terrain, oracle terrain, the attempts of the largest batch), made once."""
    import global_body_planner_amd as gbp
    if not _cache:
        data = td.by_name(NAME)
        T = gbp.Terrain.from_data(data, device=0)
        O = oracle.OracleTerrain.from_data(data)
        full = waves_of(T, 1 << 30)   # the same at every block: num_cus * opt_waves * 4
        s, a, d, _, _ = W.make_attempts(T, 129 * full + 7 + 1024, 4243)
        _cache["v"] = (T, O, (s, a, d), {})
    return _cache["v"]


def sizes(T):
    """name -> n at the handle's current block, the slice lengths each must produce checked."""
    full = waves_of(T, 1 << 30)
    one = T.get_option(L.OPT_LAUNCH_BLOCK) // WAVE     # n == waves_of(n): one attempt per wave
    out = {"n1": 1, "n2": 2, "n3": 3, "n63": 63, "n64": 64, "n65": 65,
           "waves": one, "waves+1": one + 1, "grid": full, "grid+1": full + 1,
           "64w-1": 64 * full - 1, "64w": 64 * full, "64w+5": 64 * full + 5, "129w+7": 129 * full + 7}
    assert waves_of(T, one) == one
    for k in ("64w-1", "64w", "64w+5", "129w+7"):
        assert waves_of(T, out[k]) == full
    return out


SIZES = ["n1", "n2", "n3", "n63", "n64", "n65", "waves", "waves+1", "grid", "grid+1",
         "64w-1", "64w", "64w+5", "129w+7"]


def check(block, size, mode, off=0):
    T, O, (s, a, d), memo = setup()
    T.set_option(L.OPT_BLOCK, block)
    try:
        assert T.get_option(L.OPT_LAUNCH_BLOCK) == (block or 128)   # 256^2, 2 waves: the rule says 128
        assert T.get_option(L.OPT_COORD_MODE) == 1
        n = sizes(T)[size]
        label = f"block {block}/{size}/{mode}"
        sl = slice(off, off + n)
        s, a, d = s[sl].contiguous(), a[sl].contiguous(), d[sl].contiguous()
        adaptive = mode == "adaptive"
        dd = {"fwd": L.FORWARD, "rev": L.REVERSE}.get(mode, d)
        s_new = mode != "snew_null"
        key = (n, off, mode if mode in ("fwd", "rev", "adaptive") else "dir")
        if key not in memo:   # the direct kernel's answer, computed once per input
            memo[key] = run(T, L.KERNEL_DIRECT, s, a, dd, adaptive)
        ref = memo[key]
        T.set_option(L.OPT_HELPERS, 0 if mode == "nohelpers" else 1)
        try:
            got = run(T, L.KERNEL_PERSISTENT, s, a, dd, adaptive, s_new=s_new)
        finally:
            T.set_option(L.OPT_HELPERS, 1)
        assert_same(got, ref, label, s_new=s_new)
        if n <= 4096 and s_new:
            sh, ah = s.cpu().numpy(), a.cpu().numpy()
            dh = d.cpu().numpy() if isinstance(dd, torch.Tensor) else np.full(n, dd, np.uint8)
            oracle.set_scan_mode(1)
            try:
                oref = O.validate_pairs(sh, ah, dh, adaptive=adaptive, nthreads=8)
            finally:
                oracle.set_scan_mode(0)
            assert_pairs_equal(got, oref, label + "/oracle", resolve=resolver(T, sh, ah, dh, adaptive))
    finally:
        T.set_option(L.OPT_BLOCK, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("block", BLOCKS)
def test_first_fill_sizes(gpu, block, size):
    """dir given, plain loops: every first-fill case at every block."""
    check(block, size, "dir")


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["n65", "waves+1", "64w+5"])
@pytest.mark.parametrize("mode", ["fwd", "rev", "adaptive", "snew_null", "nohelpers"])
@pytest.mark.parametrize("block", BLOCKS)
def test_modes(gpu, block, mode, size):
    """dir_all (null dir) in both directions, adaptive steps, s_new null, helpers off."""
    check(block, size, mode)


def launch(T, s, a, d, out, stream):
    VP = ctypes.c_void_p
    valid, sn, tn, fl, ct = out
    rc = T.validate_pairs_raw(s.shape[0], VP(s.data_ptr()), VP(a.data_ptr()), VP(d.data_ptr()), 0, 0,
                              VP(valid.data_ptr()), VP(sn.data_ptr()), VP(tn.data_ptr()),
                              VP(fl.data_ptr()), VP(ct.data_ptr()), VP(stream.cuda_stream))
    assert rc == 0, rc


def fresh_out(n, dev):
    return (torch.full((n,), 7, dtype=torch.uint8, device=dev),
            torch.full((n, 8), float("nan"), dtype=torch.float64, device=dev),
            torch.full((n,), float("nan"), dtype=torch.float64, device=dev),
            torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))


def host(out):
    valid, sn, tn, fl, ct = out
    return (valid.cpu().numpy(), sn.cpu().numpy(), tn.cpu().numpy(), u32(fl), u32(ct))


@pytest.mark.gpu
@pytest.mark.parametrize("block", BLOCKS)
def test_two_launches_at_once(gpu, block):
    """Two launches on two streams at once, separate inputs and outputs, 64 w + 5
    attempts each (workgroups of both share the CUs): each equals its serial run."""
    T, _, (s, a, d), _ = setup()
    T.set_option(L.OPT_BLOCK, block)
    try:
        n = sizes(T)["64w+5"]
        dev = s.device
        ins = [tuple(t[o:o + n].contiguous() for t in (s, a, d)) for o in (0, 1000)]
        serial = [run(T, L.KERNEL_PERSISTENT, *i) for i in ins]
        streams = [torch.cuda.Stream(device=dev) for _ in ins]
        outs = [fresh_out(n, dev) for _ in ins]
        torch.cuda.synchronize()
        for k in (0, 1, 0, 1):   # the second pair overlaps the first pair's drain as well
            launch(T, *ins[k], outs[k], streams[k])
        torch.cuda.synchronize()
        for k, (o, ref) in enumerate(zip(outs, serial)):
            got = host(o)
            assert_same(got, ref, f"block {block}/stream {k}")
            assert np.all(same_f64(got[1], ref[1])) and np.all(same_f64(got[2], ref[2]))
    finally:
        T.set_option(L.OPT_BLOCK, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("block", [0, 256])
def test_odd_nx_staging(gpu, block):
    """255 x 253 lines of synth-rough-256: x's last and y's first coordinate share
    one 16-byte piece of the staging, and the vectors' total is even (255 + 253)
    with y starting 8 bytes off.  Mode 1; the persistent kernel equals the direct
    one on 64 w + 5 attempts and both equal the oracle on the first 4,096."""
    import global_body_planner_amd as gbp
    if "odd" not in _cache:
        data = td.by_name(NAME)
        cut = td.TerrainData(data.x[:255].copy(), data.y[:253].copy(),
                             *[np.ascontiguousarray(v[:255, :253]) for v in (data.z, data.dx, data.dy, data.dz)],
                             name="synth-rough-255x253")
        T = gbp.Terrain.from_data(cut, device=0)
        O = oracle.OracleTerrain.from_data(cut)
        _cache["odd"] = (T, O, W.make_attempts(T, 64 * waves_of(T, 1 << 30) + 5, 4244)[:3])
    T, O, (s, a, d) = _cache["odd"]
    T.set_option(L.OPT_BLOCK, block)
    try:
        assert T.info()["nx"] == 255 and T.info()["ny"] == 253
        assert T.get_option(L.OPT_COORD_MODE) == 1
        ref = run(T, L.KERNEL_DIRECT, s, a, d)
        got = run(T, L.KERNEL_PERSISTENT, s, a, d)
        assert_same(got, ref, f"odd/block {block}")
        m = 4096
        sh, ah, dh = s[:m].cpu().numpy(), a[:m].cpu().numpy(), d[:m].cpu().numpy()
        oracle.set_scan_mode(1)
        try:
            oref = O.validate_pairs(sh, ah, dh, nthreads=8)
        finally:
            oracle.set_scan_mode(0)
        for name, res in (("persistent", got), ("direct", ref)):
            assert_pairs_equal(tuple(x[:m] for x in res), oref, f"odd/block {block}/{name}/oracle",
                               resolve=resolver(T, sh, ah, dh))
    finally:
        T.set_option(L.OPT_BLOCK, 0)


@pytest.mark.gpu
def test_block_reported_and_planner_block(gpu):
    """GBP_OPT_LAUNCH_BLOCK reports the next persistent launch's block: 128 by the
    rule at 256^2, an explicit GBP_OPT_BLOCK as given, the rule again once that is
    set back to 0; GBP_OPT_BLOCK itself reads as the caller's value, 256 until set."""
    T, _, _, _ = setup()
    assert T.get_option(L.OPT_LAUNCH_BLOCK) == 128 and T.get_option(L.OPT_BLOCK) == 256
    for b in (64, 256, 512):
        T.set_option(L.OPT_BLOCK, b)
        assert T.get_option(L.OPT_LAUNCH_BLOCK) == b and T.get_option(L.OPT_BLOCK) == b
    T.set_option(L.OPT_BLOCK, 0)
    assert T.get_option(L.OPT_LAUNCH_BLOCK) == 128
    T.set_option(L.OPT_WAVES, 4)   # eight workgroups with coordinates do not fit: 256, not staged
    try:
        assert T.get_option(L.OPT_LAUNCH_BLOCK) == 256
        assert T.get_option(L.OPT_COORD_MODE) != 1
    finally:
        T.set_option(L.OPT_WAVES, 2)
