"""The persistent validate kernel's register ring: past a
wave's first fill, lane l holds the slice's next row k = l (mod 64) in
registers, loaded a step ahead, and a refill's holders write their rows into
the idle lanes' LDS rows.  synth-rough-256 with fp32 heights and staged
coordinates runs an instantiation that has the ring; the launch takes the
ring's kernel where some wave's slice is longer than 64 and the kernel without
it below that, so the 63 / 64 / 65 cases sit on both sides of that choice.

Bar: `valid`, `flags`, `counts`, and `t_new` / `s_new` where their *_SET flags
say they are assigned, of k_validate_persistent equal k_validate_direct's bit
for bit; the first 4,096 attempts also equal the oracle's (FRAGILE attempts
re-decided on the host, as the product does).  The batch sizes give every wave
a slice of 1; 63 / 64 / 65 (the ring never filled, filled by one row, consumed
by one); 127 / 128 / 129 (exactly drained, then one reload); 191 / 192 / 193
(a third generation in the same lane); uneven slices (129 and 130); empty
slices (n = 3 at 256 lanes, n = 1 at 128).  `dir` is drawn at random (the
workload's alternation would hide a row / dir mismatch of even distance).
Every case at 128 lanes (the rule) and at GBP_OPT_BLOCK = 256.
"""
import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from global_body_planner_amd import terrain_data as td
from global_body_planner_amd import workload as W
from tests.helpers import assert_pairs_equal, resolver, same_f64
from tests.test_gpu_block_rule import fresh_out, host, launch, waves_of
from tests.test_gpu_refill_window import assert_same, run

torch = pytest.importorskip("torch")

WAVE = 64
NAME = "synth-rough-256"
BLOCKS = [0, 256]   # 0: GBP_OPT_BLOCK not set, the rule's 128 lanes
SLICES = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193]
N_ORACLE = 4096
_cache = {}


def setup():
    """(Terrain, oracle terrain, the attempts of the largest batch with a random dir), made once."""
    import global_body_planner_amd as gbp
    if not _cache:
        data = td.by_name(NAME)
        T = gbp.Terrain.from_data(data, device=0)
        O = oracle.OracleTerrain.from_data(data)
        assert T.info()["storage"] == L.STORAGE_F32   # the ring's instantiations
        full = waves_of(T, 1 << 30)   # the same at every block: num_cus * opt_waves * 4
        s, a, _, _, _ = W.make_attempts(T, 193 * full + 1024, 4245)
        g = torch.Generator().manual_seed(4246)
        d = torch.randint(0, 2, (s.shape[0],), generator=g, dtype=torch.uint8).to(s.device)
        _cache["v"] = (T, O, (s, a, d), {}, {})
    return _cache["v"]


def slice_lengths(T, n):
    wv = waves_of(T, n)
    return {n * (w + 1) // wv - n * w // wv for w in range(wv)}


def batch_size(T, case):
    """n of a named case at the handle's current block, the slice lengths it produces checked."""
    full = waves_of(T, 1 << 30)
    nwv = T.get_option(L.OPT_LAUNCH_BLOCK) // WAVE
    if case == "n1":
        n, want = 1, {0, 1}
    elif case == "n3":
        n, want = 3, {0, 1} if nwv == 4 else {1, 2}
    elif case == "uneven":
        n, want = full * 129 + 7, {129, 130}
    elif case == "slice1":
        n, want = nwv, {1}   # one workgroup, one attempt per wave
    else:
        k = int(case[5:])
        n, want = full * k, {k}
        assert waves_of(T, n) == full
    assert slice_lengths(T, n) == want, (case, n, slice_lengths(T, n))
    return n


def check(block, case, mode):
    T, O, (s, a, d), memo, omemo = setup()
    T.set_option(L.OPT_BLOCK, block)
    try:
        assert T.get_option(L.OPT_LAUNCH_BLOCK) == (block or 128)
        assert T.get_option(L.OPT_COORD_MODE) == 1
        n = batch_size(T, case)
        label = f"block {block}/{case}/{mode}"
        s, a, d = s[:n].contiguous(), a[:n].contiguous(), d[:n].contiguous()
        adaptive = mode == "adaptive"
        dd = {"fwd": L.FORWARD, "rev": L.REVERSE}.get(mode, d)
        s_new = mode != "snew_null"
        kind = mode if mode in ("fwd", "rev", "adaptive") else "dir"
        if (n, kind) not in memo:   # the direct kernel's answer, computed once per input
            memo[(n, kind)] = run(T, L.KERNEL_DIRECT, s, a, dd, adaptive)
        ref = memo[(n, kind)]
        T.set_option(L.OPT_HELPERS, 0 if mode == "nohelpers" else 1)
        try:
            got = run(T, L.KERNEL_PERSISTENT, s, a, dd, adaptive, s_new=s_new)
        finally:
            T.set_option(L.OPT_HELPERS, 1)
        assert_same(got, ref, label, s_new=s_new)
        if s_new:   # every batch is a prefix of one input: the oracle runs once per kind
            m = min(n, N_ORACLE)
            sh, ah = s[:m].cpu().numpy(), a[:m].cpu().numpy()
            dh = d[:m].cpu().numpy() if isinstance(dd, torch.Tensor) else np.full(m, dd, np.uint8)
            if (m, kind) not in omemo:
                oracle.set_scan_mode(1)
                try:
                    omemo[(m, kind)] = O.validate_pairs(sh, ah, dh, adaptive=adaptive, nthreads=8)
                finally:
                    oracle.set_scan_mode(0)
            assert_pairs_equal(tuple(x[:m] for x in got), omemo[(m, kind)], label + "/oracle",
                               resolve=resolver(T, sh, ah, dh, adaptive))
    finally:
        T.set_option(L.OPT_BLOCK, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["slice1"] + [f"slice{k}" for k in SLICES[1:]] + ["uneven", "n3", "n1"])
@pytest.mark.parametrize("block", BLOCKS)
def test_slice_lengths(gpu, block, case):
    """A random dir, plain loops: every slice length the ring treats differently."""
    check(block, case, "dir")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["slice65", "slice129", "slice193"])
@pytest.mark.parametrize("mode", ["fwd", "rev", "adaptive", "snew_null", "nohelpers"])
@pytest.mark.parametrize("block", BLOCKS)
def test_modes(gpu, block, mode, case):
    """dir_all (null dir) in both directions, adaptive steps, s_new null, helpers off."""
    check(block, case, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("block", BLOCKS)
def test_two_launches_at_once(gpu, block):
    """Two launches on two streams at once, separate inputs and outputs, slices of
    129 and 130 each (two ring generations; workgroups of both share the CUs):
    each equals its serial run."""
    T, _, (s, a, d), _, _ = setup()
    T.set_option(L.OPT_BLOCK, block)
    try:
        n = batch_size(T, "uneven")
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
