"""Informed sampling on the device (include/gbp.h gbp_informed, DESIGN 5.14;
csrc/gbp_informed.hip, the draw in csrc/gbp_device.h, the planner loop's
k_targets_informed in csrc/gbp_plan.hip) against tests/informed_ref.py's restatement
from the oracle's primitives, bit for bit, on synth-rough-256 with fp32 and
fp64 storage.

The reference of a case (20,000 draws) is computed once; draws are addressed by
(seed, stream, index), so a shorter call is a prefix of it.  Against the
restatement a NaN equals a NaN (tests.helpers.same_f64: x86 and gfx950 give
their default NaNs different payloads); every other value is compared by bits.
"""
import ctypes

import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from global_body_planner_amd import terrain_data as td
from tests import informed_ref as R
from tests.helpers import bits, same_f64
from tests.test_gpu_planner import _start_goal

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 20000
SEED, STREAM, BASE = 31, 7, 5
# (focus a, focus b, cost)
CASES = {
    "session": (R.SESSION_START, R.SESSION_GOAL, 3.9813),
    "wide": (R.SESSION_START, R.SESSION_GOAL, 6.0),      # leaves the map
    "diagonal": ((0.7, 0.9), (3.3, 4.1), 4.5),
}
STORAGES = [L.STORAGE_F32, L.STORAGE_F64]
_cache = {}


def data_and_oracle():
    if "data" not in _cache:
        d = td.by_name("synth-rough-256")
        _cache["data"] = (d, oracle.OracleTerrain.from_data(d))
    return _cache["data"]


def terrain(storage):
    import global_body_planner_amd as gbp
    key = ("T", storage)
    if key not in _cache:
        _cache[key] = gbp.Terrain.from_data(data_and_oracle()[0], device=0, storage=storage)
        assert _cache[key].info()["storage"] == storage
    return _cache[key]


def bounds():
    d = data_and_oracle()[0]
    return (float(d.x[0]), float(d.x[-1]), float(d.y[0]), float(d.y[-1]))


def case(name):
    """(the _lib.Informed record, the restated ellipse, the 20,000 reference draws)"""
    key = ("case", name)
    if key not in _cache:
        fa, fb, c = CASES[name]
        e = R.ellipse(fa, fb, c, bounds())
        assert e["active"] == 1
        ref = R.draws(data_and_oracle()[1], e, N, SEED, STREAM, BASE)
        ref.setflags(write=False)
        _cache[key] = (L.informed_ellipse(fa, fb, c, bounds()), e, ref)
    return _cache[key]


def np_(t):
    return t.cpu().numpy()


def focal_sum(q, name):
    fa, fb, _ = CASES[name]
    return (np.hypot(q[:, 0] - fa[0], q[:, 1] - fa[1]) + np.hypot(q[:, 0] - fb[0], q[:, 1] - fb[1]))


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, N])
def test_sampler_equals_restatement(gpu, storage, name, n):
    T = terrain(storage)
    inf, e, ref = case(name)
    g = np_(T.sample_states_informed(n, SEED, STREAM, index_base=BASE, inf=inf))
    assert g.shape == (n, 8)
    assert np.all(same_f64(g, ref[:n]))
    if n == 1:   # the _host entry stages the same launch
        h = np.empty((1, 8))
        L.check(L.load().gbp_sample_states_informed_host(
            T._h, 1, SEED, STREAM, BASE, None, ctypes.byref(inf), None, None,
            h.ctypes.data_as(ctypes.c_void_p)), "sample_states_informed_host")
        assert np.all(same_f64(h, ref[:1]))


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", list(CASES))
def test_draws_lie_in_the_ellipse_uniformly(gpu, storage, name):
    T = terrain(storage)
    inf, e, _ = case(name)
    g = np_(T.sample_states_informed(N, SEED, STREAM, index_base=BASE, inf=inf))
    c = CASES[name][2]
    s = focal_sum(g, name)
    print(f"{name}: largest focal sum {s.max():.15g} of c = {c}")
    assert np.all(s <= c * (1 + 1e-12))
    # uniform over the area: the ellipse scaled by 1/2 holds a quarter of the draws
    # (sigma = sqrt(.25 * .75 / 20000) = 0.0031: +-0.02 is more than 6 sigma)
    px = (g[:, 0] - e["cx"]) * e["ux"] + (g[:, 1] - e["cy"]) * e["uy"]
    py = -(g[:, 0] - e["cx"]) * e["uy"] + (g[:, 1] - e["cy"]) * e["ux"]
    share = np.mean((px / e["a"]) ** 2 + (py / e["b"]) ** 2 <= 0.25)
    print(f"{name}: share inside the half-scale ellipse {share:.4f}")
    assert abs(share - 0.25) <= 0.02
    # a draw outside the map comes back with NaN z and nothing else does
    b = bounds()
    off = ~((g[:, 0] >= b[0]) & (g[:, 0] < b[1]) & (g[:, 1] >= b[2]) & (g[:, 1] < b[3]))
    assert np.array_equal(np.isnan(g[:, 2]), off)
    assert not np.isnan(np.delete(g, 2, axis=1)).any()
    print(f"{name}: {off.mean():.4f} of the draws leave the map")
    if name == "wide":
        # the c = 6.0 ellipse (axis along x) passes all four edges of the map; the
        # segment of an ellipse beyond a line at u semi-axes from its centre is
        # (acos(u) - u sqrt(1 - u^2)) / pi of its area, and the four segments do not
        # meet: 7.1 % in all.  sigma = sqrt(.071 * .929 / 20000) = 0.0018; +-0.011 is 6 sigma
        seg = lambda u: (np.arccos(u) - u * np.sqrt(1 - u * u)) / np.pi
        out = (seg((e["cx"] - b[0]) / e["a"]) + seg((b[1] - e["cx"]) / e["a"]) +
               seg((e["cy"] - b[2]) / e["b"]) + seg((b[3] - e["cy"]) / e["b"]))
        assert 0.06 < out < 0.08
        assert abs(off.mean() - out) <= 0.011
    else:
        assert not off.any()


@pytest.mark.parametrize("storage", STORAGES)
def test_stance_valid_share_of_the_session_draws(gpu, storage):
    """The draws are usable targets: the STANCE-valid share of the c = 3.9813
    draws exceeds 0.3 (plain draws over the map: 0.43)."""
    T = terrain(storage)
    inf, _, _ = case("session")
    g = T.sample_states_informed(N, SEED, STREAM, index_base=BASE, inf=inf)
    valid, _, _ = T.valid_states_host(g, L.STANCE)
    print(f"STANCE-valid share {valid.mean():.4f}")
    assert valid.mean() > 0.3


@pytest.mark.parametrize("storage", STORAGES)
def test_inactive_ellipse_is_the_plain_sampler(gpu, storage):
    T = terrain(storage)
    plain = np_(T.sample_states(N, SEED, STREAM, BASE)[0])
    fa, fb, _ = CASES["session"]
    off = L.informed_ellipse(fa, fb, 3.9813, bounds())
    off.active = 0
    inf_cost = L.informed_ellipse(fa, fb, float("inf"), bounds())
    too_wide = L.informed_ellipse(fa, fb, 7.0, bounds())
    assert inf_cost.active == 0 and too_wide.active == 0
    for inf in (off, inf_cost, too_wide, L.Informed()):
        g = np_(T.sample_states_informed(N, SEED, STREAM, index_base=BASE, inf=inf))
        assert np.array_equal(bits(g), bits(plain))
    # inf None: the handle's, off until it is set
    assert T.get_informed().active == 0
    g = np_(T.sample_states_informed(N, SEED, STREAM, index_base=BASE))
    assert np.array_equal(bits(g), bits(plain))


@pytest.mark.parametrize("storage", STORAGES)
def test_handle_setting(gpu, storage):
    T = terrain(storage)
    inf, _, ref = case("diagonal")
    try:
        T.set_informed(inf)
        got = T.get_informed()
        assert bytes(got) == bytes(inf)
        g = np_(T.sample_states_informed(257, SEED, STREAM, index_base=BASE))
        assert np.all(same_f64(g, ref[:257]))
        # the other samplers do not read it
        plain = np_(T.sample_states(257, SEED, STREAM, BASE)[0])
        assert not np.array_equal(bits(plain), bits(g))
        bad = L.Informed.from_buffer_copy(bytes(inf))
        bad.a = float("nan")
        with pytest.raises(L.GbpError) as err:
            T.set_informed(bad)
        assert err.value.status == L.E_INVALID_ARG
        assert bytes(T.get_informed()) == bytes(inf)
    finally:
        T.set_informed(None)
    assert T.get_informed().active == 0


@pytest.mark.parametrize("storage", STORAGES)
def test_direction_coin_keeps_its_draws(gpu, storage):
    """state_flag on: the coin is drawn as before; where it lands the draw is
    sample_states_dir's, elsewhere the informed one."""
    T = terrain(storage)
    inf, _, ref = case("session")
    s_from = np.array([1.0, 2.55, 0.6, 1.0, 0.0, 0.0, 0.0, 0.0])
    s_to = np.array([4.02, 1.10, 0.5, 0.2, 0.4, 0.0, 0.0, 0.0])
    plain = np_(T.sample_states(N, SEED, STREAM, BASE)[0])
    for speed in (False, True):
        cfg = L.sampling(state_flag=True, state_p=0.5, speed_direction=speed)
        d = np_(T.sample_states_dir(N, SEED, STREAM, s_from, s_to, index_base=BASE, cfg=cfg))
        g = np_(T.sample_states_informed(N, SEED, STREAM, s_from, s_to, index_base=BASE, cfg=cfg,
                                         inf=inf))
        landed = np.any(bits(d) != bits(plain), axis=1)
        assert 0.45 < landed.mean() < 0.55
        assert np.array_equal(bits(g[landed]), bits(d[landed]))
        assert np.all(same_f64(g[~landed], ref[~landed]))
    # state_flag needs its two states
    with pytest.raises(L.GbpError):
        T.sample_states_informed(4, SEED, STREAM, cfg=L.sampling(state_flag=True), inf=inf)


@pytest.mark.parametrize("storage", STORAGES)
def test_past_one_grid_pass(gpu, storage):
    """n = 1,048,869 with an index_base: the capped grid (16 workgroups of 256
    per CU, 1,048,576 lanes on 256 CUs) takes a second pass; rows [k, k + 256)
    equal a 256-draw call at index_base + k for a k in each pass."""
    T = terrain(storage)
    inf, _, _ = case("session")
    n, base = 1048869, 123456789
    big = T.sample_states_informed(n, SEED, STREAM, index_base=base, inf=inf)
    assert big.shape == (n, 8)
    for k in (0, 777, 1048576 - 100, 1048576 + 20, n - 256):
        part = T.sample_states_informed(256, SEED, STREAM, index_base=base + k, inf=inf)
        assert torch.equal(big[k:k + 256].view(torch.int64), part.view(torch.int64)), k


def run_halves(T, ws, trees, first, count, batch, seed, at_once):
    """halves first .. first + count - 1 of RRT-Connect, FRAGILE halts resolved
    on the host; -> the status after each group (one half or all of them)"""
    out = []
    step = count if at_once else 1
    for h in range(first, first + count, step):
        ws.halves(T, trees[0], trees[1], h, step, batch, seed=seed)
        st = ws.status()
        while st["halt"]:
            h0 = st["halt_half"]
            k = h0 & 1
            resume, _ = ws.resolve(T, trees[k], trees[k ^ 1], L.FORWARD if k == 0 else L.REVERSE,
                                   batch)
            assert resume >= 0
            ws.halves(T, trees[0], trees[1], h0, h + step - h0, batch, seed=seed,
                      first_stage=resume)
            st = ws.status()
        assert not st["error"]
        out.append(st)
    return out


@pytest.mark.parametrize("storage", STORAGES)
def test_planner_loop_draws_its_targets_in_the_ellipse(gpu, storage):
    """k_targets_informed, the planner loop's targets with the handle's ellipse:
    a half's n_targets is the count of
    STANCE-valid rows (the oracle's decision) among the public sampler's draws
    for that half's stream and index base; the halves enqueued one by one and
    all at once (no look-ahead search either way) build the same trees; with
    the ellipse off the counts differ."""
    from global_body_planner_amd import engine
    _, O = data_and_oracle()
    T = terrain(storage)
    start, goal = _start_goal(O, *R.SESSION_START, *R.SESSION_GOAL)
    inf = L.informed_ellipse(start, goal, 4.0, bounds())
    assert inf.active == 1
    batch, seed, halves = 512, 5, 4
    runs = {}
    try:
        for label, on, at_once in (("one by one", True, False), ("at once", True, True),
                                   ("off", False, False)):
            T.set_informed(inf if on else None)
            trees = [engine.DeviceTree(start, device=0), engine.DeviceTree(goal, device=0)]
            ws = engine.PlanWorkspace(T, batch)
            ws.reset()
            sts = run_halves(T, ws, trees, 0, halves, batch, seed, at_once)
            runs[label] = (sts, [t.read() for t in trees])
        T.set_informed(inf)
        expect = []
        for h in range(halves):
            g = np_(T.sample_states_informed(batch, seed, 102 if h & 1 else 101,
                                             index_base=(h >> 1) * batch))
            expect.append(int(O.valid_states(g, L.STANCE, nthreads=8)[0].sum()))
    finally:
        T.set_informed(None)
    sts, tr = runs["one by one"]
    checked = 0
    for h, st in enumerate(sts):
        assert st["n_targets"] == expect[h], (h, st["n_targets"], expect[h])
        checked += 1
        if st["done"]:   # the halves after a connection are gated
            break
    assert checked >= 2
    assert runs["at once"][0][-1]["stat_targets"] == sts[-1]["stat_targets"]
    for a, b in zip(tr, runs["at once"][1]):
        for x, y in zip(a, b):
            assert np.array_equal(bits(x) if x.dtype == np.float64 else x,
                                  bits(y) if y.dtype == np.float64 else y)
    off = [s["n_targets"] for s in runs["off"][0]]
    print(f"targets per half: informed {[s['n_targets'] for s in sts]}, expected {expect}, "
          f"plain {off}")
    assert off[:checked] != expect[:checked]
