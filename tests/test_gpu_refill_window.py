"""The persistent validate kernel's refill: the direct
refill (rows and dir in one round trip), which is the default build, and, in a
-DGBP_REFILL_WINDOW build, the per-wave prefetch window in LDS (slot swap)
with the first refill issued ahead of the coordinate staging.  The same cases
run against whichever form the library was built with; where the build has no
window the slice lengths are those of the window's full size (32).

Bar: `valid`, `flags`, `counts`, `t_new` and `s_new` of k_validate_persistent
equal k_validate_direct's bit for bit on the same inputs (s_new / t_new where
their *_SET flags say they are assigned); for n <= 4096 the oracle's as well.
The batch sizes put every per-wave slice length the refill treats differently
in front of it: 1, the window's size PF and its neighbours, 64 + PF + 1 (the
window's queue wraps, uneven slices), empty slices.
"""
import ctypes

import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from global_body_planner_amd import terrain_data as td
from global_body_planner_amd import workload as W
from tests.helpers import assert_pairs_equal, resolver, same_f64, u32

torch = pytest.importorskip("torch")

WAVE = 64
PF_MAX = 32
_cache = {}


def setup(name):
    """(data, Terrain, oracle terrain, the attempts of the largest batch) of a terrain, made once."""
    import global_body_planner_amd as gbp
    if name not in _cache:
        data = td.by_name(name)
        T = gbp.Terrain.from_data(data, device=0)
        O = oracle.OracleTerrain.from_data(data)
        n_max = waves_of(T, 1 << 30) * (WAVE + PF_MAX + 1) + 5
        s, a, d, _, _ = W.make_attempts(T, n_max, 4242)
        _cache[name] = (data, T, O, (s, a, d))
    return _cache[name]


def waves_of(T, n):
    """Waves of the persistent launch for n attempts, as launch_validate_w sizes it."""
    block = T.get_option(L.OPT_BLOCK)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    resident = cus * max(1, T.get_option(L.OPT_WAVES) * 256 // block)
    return max(1, min(resident, (n + WAVE - 1) // WAVE)) * (block // WAVE)


def slice_lengths(T, n):
    wv = waves_of(T, n)
    return {n * (w + 1) // wv - n * w // wv for w in range(wv)}


def batch_size(T, case):
    """n for a named case, with the slice lengths it must produce checked."""
    pf = T.get_option(L.OPT_REFILL_WINDOW) or PF_MAX   # 0: a build without the window
    assert 0 < pf <= PF_MAX, pf
    full = waves_of(T, 1 << 30)       # every resident slot
    if case.startswith("n"):
        return int(case[1:])
    if case == "slice1":
        n = T.get_option(L.OPT_BLOCK) // WAVE   # one workgroup, one attempt per wave
        assert slice_lengths(T, n) == {1}
    elif case == "empty":
        n = 3
        assert 0 in slice_lengths(T, n)
    elif case == "wrap":
        n = full * (WAVE + pf + 1) + 5
        assert slice_lengths(T, n) == {WAVE + pf + 1, WAVE + pf + 2}
    else:
        k = {"pf-1": pf - 1, "pf": pf, "pf+1": pf + 1}[case]
        n = full * k
        assert slice_lengths(T, n) == {k}
    return n


def run(T, kernel, s, a, d, adaptive=False, s_new=True):
    """One launch through the pointer-level entry; d: a uint8 tensor or FORWARD / REVERSE."""
    n = s.shape[0]
    dev = s.device
    VP = ctypes.c_void_p
    T.set_option(L.OPT_KERNEL, kernel)
    valid = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    sn = torch.full((n, 8), float("nan"), dtype=torch.float64, device=dev)
    tn = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    fl = torch.zeros(n, dtype=torch.int32, device=dev)
    ct = torch.zeros(n, dtype=torch.int32, device=dev)
    dptr, dall = (VP(d.data_ptr()), 0) if isinstance(d, torch.Tensor) else (None, int(d))
    rc = T.validate_pairs_raw(n, VP(s.data_ptr()), VP(a.data_ptr()), dptr, dall, int(adaptive),
                              VP(valid.data_ptr()), VP(sn.data_ptr()) if s_new else None,
                              VP(tn.data_ptr()), VP(fl.data_ptr()), VP(ct.data_ptr()),
                              VP(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    T.set_option(L.OPT_KERNEL, L.KERNEL_PERSISTENT)
    return (valid.cpu().numpy(), sn.cpu().numpy(), tn.cpu().numpy(), u32(fl), u32(ct))


def assert_same(got, ref, label, s_new=True):
    gv, gsn, gtn, gf, gc = got
    rv, rsn, rtn, rf, rc = ref
    assert np.array_equal(gv, rv), f"{label}: valid differs at {np.flatnonzero(gv != rv)[:10]}"
    assert np.array_equal(gf, rf), f"{label}: flags differ at {np.flatnonzero(gf != rf)[:10]}"
    assert np.array_equal(gc, rc), f"{label}: counts differ at {np.flatnonzero(gc != rc)[:10]}"
    tset = (rf & L.F_TNEW_SET) != 0
    assert np.all(same_f64(gtn[tset], rtn[tset])), f"{label}: t_new differs"
    assert np.all(np.isnan(gtn[~tset])), f"{label}: t_new written where it is not assigned"
    sset = (rf & L.F_SNEW_SET) != 0
    if s_new:
        assert np.all(same_f64(gsn[sset], rsn[sset])), f"{label}: s_new differs"
        assert np.all(np.isnan(gsn[~sset])), f"{label}: s_new written where it is not assigned"
    else:
        assert np.all(np.isnan(gsn)), f"{label}: s_new written through a null pointer's stand-in"


def check(name, n, mode, label):
    data, T, O, (s, a, d) = setup(name)
    s, a, d = s[:n].contiguous(), a[:n].contiguous(), d[:n].contiguous()
    adaptive = mode == "adaptive"
    dd = {"fwd": L.FORWARD, "rev": L.REVERSE}.get(mode, d)
    s_new = mode != "snew_null"
    ref = run(T, L.KERNEL_DIRECT, s, a, dd, adaptive)
    got = run(T, L.KERNEL_PERSISTENT, s, a, dd, adaptive, s_new=s_new)
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


SIZES = ["n1", "n63", "n64", "n65", "slice1", "pf-1", "pf", "pf+1", "wrap", "empty"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SIZES)
def test_slice_lengths(gpu, case):
    """dir given, plain loops: every slice length the refill treats differently."""
    _, T, _, _ = setup("synth-rough-256")
    check("synth-rough-256", batch_size(T, case), "dir", case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["n65", "pf+1", "wrap"])
@pytest.mark.parametrize("mode", ["fwd", "rev", "adaptive", "snew_null"])
def test_modes(gpu, case, mode):
    """dir_all (null dir) in both directions, adaptive steps, s_new null."""
    _, T, _, _ = setup("synth-rough-256")
    check("synth-rough-256", batch_size(T, case), mode, f"{case}/{mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8192, None])
def test_window_beside_staged_coordinates(gpu, n):
    """synth-rough-1024: the coordinate vectors stay in LDS and the window fits
    behind them; 8,192 attempts, and the batch whose slices wrap the window."""
    _, T, _, _ = setup("synth-rough-1024")
    assert T.get_option(L.OPT_COORD_MODE) == 1
    assert 0 <= T.get_option(L.OPT_REFILL_WINDOW) <= PF_MAX
    check("synth-rough-1024", n or batch_size(T, "wrap"), "dir", f"1024/{n}")


@pytest.mark.gpu
def test_device_count_path(gpu):
    """The batch size read on the device (n_dev): the planner loop resident on
    the device against the host-driven batched loop, and its path against the
    oracle."""
    from global_body_planner_amd import planner
    from tests.test_gpu_planner import _start_goal, check_path
    data = td.by_name("synth-rough-256")
    O = oracle.OracleTerrain.from_data(data)
    start, goal = _start_goal(O, 1.0, 2.55, 4.02, 2.55)
    kw = dict(batch=4096, max_time=120.0, seed=3)
    host = planner.plan_rrt_connect(data, start, goal, **kw)
    dev = planner.plan_rrt_connect_device(data, start, goal, **kw)
    assert host["found"] == 1 and dev["found"] == 1
    check_path(O, dev, start, goal)
    assert np.array_equal(dev["states"], host["states"])
    assert np.array_equal(dev["actions"], host["actions"])
    for k in ("vertices_a", "vertices_b", "extends", "attempts_checked"):
        assert dev[k] == host[k], (k, dev[k], host[k])


@pytest.mark.parametrize("nxy", [256, 1024, 4096])
@pytest.mark.parametrize("block", [256, 512])
@pytest.mark.parametrize("waves", [2, 4])
def test_lds_request_fits(nxy, block, waves):
    """Host side (no device): the LDS a launch requests never exceeds the
    workgroup limit (160 KB on gfx950), and a window is added only where the
    workgroups that share a CU still fit its 160 KB together."""
    lib = L.load()
    limit = 160 * 1024
    cm, pf, nbytes = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(0)
    rc = lib.gbp_validate_lds_plan(nxy, nxy, block, waves, limit, ctypes.byref(cm),
                                   ctypes.byref(pf), ctypes.byref(nbytes))
    assert rc == 0
    assert 0 <= pf.value <= PF_MAX
    assert nbytes.value <= limit
    if pf.value:   # a window never costs a workgroup its place on the CU
        assert max(1, waves * 256 // block) * nbytes.value <= limit
    if nxy <= 1024 and waves == 2:
        assert cm.value == 1   # the window never displaces the coordinates
        assert pf.value > 0 or not has_window(lib)


def has_window(lib):
    """Was the library built with the prefetch window (-DGBP_REFILL_WINDOW)?"""
    pf = ctypes.c_int(-1)
    assert lib.gbp_validate_lds_plan(256, 256, 256, 1, 160 * 1024, None, ctypes.byref(pf), None) == 0
    return pf.value > 0


def test_window_degrades_to_none():
    """A limit that holds the coordinates, the 64 rows and the rings but not one
    more row: the window is 0, the coordinates stay staged, no error."""
    lib = L.load()
    block, nxy = 256, 1024
    base = 8 * 2 * nxy + (8 * 19 * WAVE + 16 * 128) * (block // WAVE)
    for extra, want in ((0, 0), (100, 0), (8 * 19 * (block // WAVE) + 16, 1)):
        cm, pf, nbytes = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(0)
        rc = lib.gbp_validate_lds_plan(nxy, nxy, block, 1, base + extra, ctypes.byref(cm),
                                       ctypes.byref(pf), ctypes.byref(nbytes))
        want = want if has_window(lib) else 0
        assert rc == 0 and cm.value == 1 and pf.value == want, (extra, cm.value, pf.value)
        assert nbytes.value <= base + extra
