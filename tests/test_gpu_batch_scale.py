"""The batched entries past one pass of their capped grids: k_height (8 x CUs
workgroups), k_normal, k_valid_states, k_sample_states, k_extend_prep and
k_extend_select (16 x CUs), k_sample_actions and k_sample_actions_dir (4096)
are grid-stride loops, and no other test hands them more than 262,144 elements.

One call of n = 16 x CUs x 256 + 256 + 37 elements is compared, bit for bit in
every output, with the same inputs in chunks of 262,144: the size
test_gpu_parity.py pins to the oracle.  The chunked form is the reference,
never the single call.  Where the oracle's entry needs no index base, the last
1,024 elements of the single call (the second turn and the boundary) are
compared with the oracle directly as well.
"""
import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from global_body_planner_amd import terrain_data as td
from global_body_planner_amd import workload as W
from tests import grid_cases as G
from tests import scale_cases as X
from tests.helpers import bits, same_f64, u32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TERRAINS = ["synth-rough-256", "gradedxtwostep-ripple"]
TAIL = 1024
BASE = 3 << 20            # the samplers' index base: no draw of a chunk starts at index 0
SEED = 20261150
EXTD = 0x45585444         # the stream of an extend's candidate actions
S_FROM = np.array([1.0, 2.55, 0.6, 1.0, 0.0, 0.0, 0.0, 0.0])
S_TO = np.array([4.02, 1.10, 0.5, 0.2, 0.4, 0.0, 0.0, 0.0])
_cache = {}


@pytest.fixture(autouse=True)
def _bisect():
    oracle.set_scan_mode(1)
    yield
    oracle.set_scan_mode(0)


def terrain_pair(name):
    import global_body_planner_amd as gbp
    if name not in _cache:
        data = td.by_name(name) if name.startswith("synth") else G.terrain("graded", "twostep", "ripple")
        assert name.startswith("synth") or data.name == name
        _cache[name] = (data, gbp.Terrain.from_data(data, device=0), oracle.OracleTerrain.from_data(data))
    return _cache[name]


def big_n():
    n = X.batch_n(torch.cuda.get_device_properties(0).multi_processor_count)
    assert n > X.CHUNK and n % X.CHUNK                # several chunks, the last one short
    return n


def chunked(fn, n):
    """fn(offset, count) -> tensor or tuple of tensors, over chunks of 262,144, joined."""
    parts = [fn(o, min(X.CHUNK, n - o)) for o in range(0, n, X.CHUNK)]
    if isinstance(parts[0], torch.Tensor):
        return torch.cat(parts)
    return tuple(torch.cat([p[k] for p in parts]) for k in range(len(parts[0])))


def same(a, b):
    """Bit equality of two device tensors."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


def assert_same(one, ref, label):
    one = (one,) if isinstance(one, torch.Tensor) else tuple(one)
    ref = (ref,) if isinstance(ref, torch.Tensor) else tuple(ref)
    assert len(one) == len(ref)
    for k, (a, b) in enumerate(zip(one, ref)):
        if not same(a, b):
            bad = torch.nonzero((a != b).reshape(len(a), -1).any(dim=1)).flatten()[:5].tolist()
            raise AssertionError((label, k, "first rows that differ", bad))


def np_(t):
    return t.cpu().numpy()


def inputs(name):
    """The terrain's n states (plain and STANCE draws), points, normals and
    directions, every one of them made in chunks of 262,144."""
    key = ("inputs", name)
    if key not in _cache:
        _, T, _ = terrain_pair(name)
        n = big_n()
        st = chunked(lambda o, m: T.sample_states(m, SEED, 1, index_base=BASE + o), n)
        near = chunked(lambda o, m: T.sample_states(m, SEED, 2, index_base=BASE + o, require_phase=L.STANCE,
                                                    max_tries=W.MAX_TRIES), n)
        xy = st[0][:, :2].contiguous()
        xy[::97] += 100.0                            # out of the map
        xy[5::1009, 1] = float("nan")
        nrm = chunked(lambda o, m: T.normal(xy[o:o + m].contiguous()), n)
        d = (torch.arange(n, device=xy.device) % 2).to(torch.uint8)
        _cache[key] = dict(n=n, states=st, near=near, xy=xy, normals=nrm, direction=d)
    return _cache[key]


# ---- lookups and the state check -----------------------------------------------------------------
@pytest.mark.parametrize("name", TERRAINS)
def test_height_and_normal(gpu, name):
    _, T, O = terrain_pair(name)
    i = inputs(name)
    n, xy = i["n"], i["xy"]
    one = T.height(xy)
    assert_same(one, chunked(lambda o, m: T.height(xy[o:o + m].contiguous()), n), "height")
    h, nan, ood = (np_(t[-TAIL:]) for t in one)
    rh, rnan, rood = O.height_batch(np_(xy[-TAIL:]), nthreads=8)
    assert np.array_equal(nan, rnan) and np.array_equal(ood, rood) and np.all(same_f64(h, rh))
    assert 0 < rood.sum() < TAIL
    one = T.normal(xy)
    assert_same(one, i["normals"], "normal")
    nrm, nood = (np_(t[-TAIL:]) for t in one)
    rn, rnood = O.normal_batch(np_(xy[-TAIL:]), nthreads=8)
    assert np.array_equal(nood, rnood)
    assert np.array_equal(bits(nrm[rnood == 0]), bits(rn[rnood == 0]))


@pytest.mark.parametrize("name", TERRAINS)
def test_valid_states(gpu, name):
    _, T, O = terrain_pair(name)
    i = inputs(name)
    n, st, phase = i["n"], i["states"][0], i["direction"]        # phase 0 / 1 by index
    one = T.valid_states(st, phase)
    ref = chunked(lambda o, m: T.valid_states(st[o:o + m].contiguous(), phase[o:o + m].contiguous()), n)
    assert_same(one, ref, "valid_states")
    v, f, c = np_(one[0][-TAIL:]), u32(one[1][-TAIL:]), u32(one[2][-TAIL:])
    tail, ph = np_(st[-TAIL:]), np_(phase[-TAIL:])
    rv, rf, rc = O.valid_states(tail, ph, nthreads=8)
    m = np.uint32(~(L.F_FRAGILE | L.F_RESOLVED) & 0xFFFFFFFF)
    sure = (f & L.F_FRAGILE) == 0
    assert np.array_equal(v[sure], rv[sure]) and np.array_equal(f[sure] & m, rf[sure] & m)
    assert np.array_equal(c[sure], rc[sure]) and 0 < rv.sum() < TAIL
    hv, hf, hc = T.valid_states_host(tail, ph)           # FRAGILE states re-decided: every state
    assert np.array_equal(hv, rv) and np.array_equal(hf & m, rf & m) and np.array_equal(hc, rc)


# ---- the samplers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TERRAINS)
def test_sample_states(gpu, name):
    _, T, O = terrain_pair(name)
    i = inputs(name)
    n = i["n"]
    assert_same(T.sample_states(n, SEED, 1, index_base=BASE), i["states"], "sample_states")
    one = T.sample_states(n, SEED, 2, index_base=BASE, require_phase=L.STANCE, max_tries=W.MAX_TRIES)
    assert_same(one, i["near"], "sample_states STANCE")
    assert int((one[1] < 0).sum()) == 0 and int((one[1] > 1).sum()) > 0     # redrawn states among them
    cfg = L.sampling(state_flag=True, state_p=0.5, speed_direction=True)
    one = T.sample_states_dir(n, SEED, 7, S_FROM, S_TO, index_base=BASE, cfg=cfg)
    ref = chunked(lambda o, m: T.sample_states_dir(m, SEED, 7, S_FROM, S_TO, index_base=BASE + o, cfg=cfg), n)
    assert_same(one, ref, "sample_states_dir")
    assert not same(one, i["states"][0])


def test_sample_actions(gpu):
    _, T, O = terrain_pair(TERRAINS[0])
    i = inputs(TERRAINS[0])
    n, nrm = i["n"], i["normals"][0]
    one = T.sample_actions(nrm, SEED, 3, index_base=BASE)
    ref = chunked(lambda o, m: T.sample_actions(nrm[o:o + m].contiguous(), SEED, 3, index_base=BASE + o), n)
    assert_same(one, ref, "sample_actions")
    st, near, d = i["states"][0], i["near"][0], i["direction"]
    cfg = L.sampling(action_flag=True, action_p=0.5)
    one_dir = T.sample_actions_dir(nrm, st, near, d, SEED, 3, index_base=BASE, cfg=cfg)
    ref = chunked(lambda o, m: T.sample_actions_dir(nrm[o:o + m].contiguous(), st[o:o + m].contiguous(),
                                                    near[o:o + m].contiguous(), d[o:o + m].contiguous(),
                                                    SEED, 3, index_base=BASE + o, cfg=cfg), n)
    assert_same(one_dir, ref, "sample_actions_dir")
    moved = (one_dir != one).any(dim=1).double().mean().item()
    assert 0.4 < moved < 0.6, moved


# ---- extend --------------------------------------------------------------------------------------------
def extend_tuple(r):
    return (r.result, r.chosen, r.s_new, r.a_new, r.counts, r.flags)


@pytest.mark.parametrize("size", ["prep", "select"])
def test_extend(gpu, size):
    """175,003 extends: 6 n candidates cross k_extend_prep's cap; n extends:
    k_extend_select's too.  Chunks carry their extend_base."""
    name = TERRAINS[0]
    _, T, O = terrain_pair(name)
    i = inputs(name)
    n = X.N_EXTEND_PREP if size == "prep" else i["n"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 6 * n > 16 * cus * 256 and (size == "prep" or n > 16 * cus * 256)
    near, tgt, d = i["near"][0][:n].contiguous(), i["states"][0][:n].contiguous(), i["direction"][:n].contiguous()
    base = 1000
    one = T.extend(near, tgt, d, seed=41, extend_base=base)
    ref = chunked(lambda o, m: extend_tuple(T.extend(near[o:o + m].contiguous(), tgt[o:o + m].contiguous(),
                                                     d[o:o + m].contiguous(), seed=41, extend_base=base + o)), n)
    assert_same(extend_tuple(one), ref, ("extend", size))
    # the last 1,024 against the oracle, their candidates regenerated through the public sampler
    s_h, t_h, d_h = np_(near[-TAIL:]), np_(tgt[-TAIL:]), np_(d[-TAIL:])
    nrm = O.normal_batch(t_h[:, :2])[0]
    dense = np_(T.sample_actions(torch.from_numpy(np.repeat(nrm, 8, axis=0)), 41, EXTD,
                                 (base + n - TAIL) * 8)).reshape(TAIL, 8, 10)
    rr, rch, rsn, ran, rc = O.extend_batch(s_h, t_h, np.ascontiguousarray(dense[:, :6]), d_h, nthreads=8)
    got = [np_(t[-TAIL:]) for t in extend_tuple(one)]
    frag = (got[5].view(np.uint32) & L.F_FRAGILE) != 0
    assert frag.sum() <= 4
    if frag.any():      # re-decided on the host, as the product does
        host = T.extend_host(s_h, t_h, d_h, seed=41, extend_base=base + n - TAIL)
        for k in range(5):
            got[k][frag] = host[k][frag]
    assert np.array_equal(got[0], rr) and np.array_equal(got[1], rch)
    assert np.array_equal(got[4].view(np.uint32), rc)
    acc = rr != L.TRAPPED
    assert np.array_equal(bits(got[2][acc]), bits(rsn[acc])) and np.array_equal(bits(got[3][acc]), bits(ran[acc]))
    assert 0 < acc.sum() < TAIL
