"""GPU parity on non-uniform terrain grids (tests/grid_cases.py): the general
bracket search — the `ONE = false` instantiation of the persistent validate
kernel, the `while` loops of bracket() / bracket_ax<..., false> in every other
kernel, one axis exact and the other not, repeated coordinates (empty cells),
two-line axes (the n - 2 == 0 clamps) — against the oracle, which scans any
ascending vector.

Bar: that of tests/test_gpu_parity.py — bit for bit (NaN == NaN), FRAGILE
decisions re-decided through the host entries first, none excluded.
"""
import dataclasses

import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from global_body_planner_amd import planner
from global_body_planner_amd import terrain_data as td
from tests import grid_cases as G
from tests import prune_ref as R
from tests.helpers import assert_pairs_equal, attempts_oracle, bits, resolver, same_f64, u32
from tests.test_gpu_oracle_loop import assert_counters_equal, assert_trees_equal
from tests.test_gpu_planner import _start_goal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# every terrain with storage AUTO (fp32: the layers are float-rounded), and
# graded x graded also with fp64 heights forced
CASES = [(p, L.STORAGE_AUTO) for p in G.TERRAINS] + [(("graded", "graded"), L.STORAGE_F64)]
CASE_IDS = [G.terrain_id(p) + ("-f64" if st == L.STORAGE_F64 else "") for p, st in CASES]

_terrains, _batches = {}, {}


def terrain_pair(pair, storage=L.STORAGE_AUTO):
    import global_body_planner_amd as gbp
    key = (tuple(pair), storage)
    if key not in _terrains:
        data = G.terrain(*pair)
        _terrains[key] = (data, gbp.Terrain.from_data(data, device=0, storage=storage),
                          oracle.OracleTerrain.from_data(data))
    return _terrains[key]


def pair_batch(pair, O):
    """The terrain's attempts and the oracle's results, (plain, adaptive): computed once."""
    key = tuple(pair)
    if key not in _batches:
        s, a, d, _, _ = attempts_oracle(O, G.N_PAIRS, seed=G.pair_seed(pair))
        refs = {ad: O.validate_pairs(s, a, d, adaptive=ad, nthreads=8) for ad in (False, True)}
        for r in refs.values():
            for arr in r:
                arr.setflags(write=False)
        _batches[key] = (s, a, d, refs)
    return _batches[key]


@pytest.fixture(autouse=True)
def _bisect():
    oracle.set_scan_mode(1)  # same brackets as the linear scan (test_grid_cases.py), faster
    yield
    oracle.set_scan_mode(0)


def np_(t):
    return t.cpu().numpy()


# ---- the class the host analysis gave the terrain ------------------------------------

@pytest.mark.parametrize("pair,storage", CASES, ids=CASE_IDS)
def test_kernel_class_follows_the_grid(gpu, pair, storage):
    """gbp_terrain_create's analysis, read back through the read-only options:
    the persistent kernel stages the vectors in LDS (coordinate mode 1, the
    straight-line bracket) exactly when both axes are one-step exact, computes
    them (mode 2) exactly when they are also affine, and otherwise reads them
    from global memory with the general search (mode 0)."""
    data, T, O = terrain_pair(pair, storage)
    one_x, one_y, affine = G.predicted(pair)
    one = bool(one_x and one_y)
    assert T.info()["storage"] == (L.STORAGE_F32 if storage == L.STORAGE_AUTO else storage)
    try:
        T.set_option(L.OPT_KERNEL, L.KERNEL_PERSISTENT)
        T.set_option(L.OPT_WAVES, 2)
        T.set_option(L.OPT_AFFINE_COORDS, 1)
        T.set_option(L.OPT_LDS_COORDS, 1)
        assert T.get_option(L.OPT_COORD_MODE) == (1 if one else 0)
        T.set_option(L.OPT_LDS_COORDS, 0)
        assert T.get_option(L.OPT_COORD_MODE) == (2 if one and affine else 0)
        # the direct kernel branches at run time: LDS whatever the class
        T.set_option(L.OPT_KERNEL, L.KERNEL_DIRECT)
        T.set_option(L.OPT_LDS_COORDS, 1)
        assert T.get_option(L.OPT_COORD_MODE) == 1
    finally:
        T.set_option(L.OPT_LDS_COORDS, 1)
        T.set_option(L.OPT_KERNEL, L.KERNEL_PERSISTENT)
    rcp = T.get_option(L.OPT_FAST_RCP)
    assert rcp in (0, 1)
    print(f"{data.name}: one_x {one_x} one_y {one_y} affine {affine}, fast reciprocal {rcp}")
    if tuple(pair) == ("uniform", "uniform"):
        import global_body_planner_amd as gbp
        S = gbp.Terrain.from_data(td.by_name("synth-rough-256"), device=0)
        assert rcp == S.get_option(L.OPT_FAST_RCP)
    if "dups" in pair:
        assert rcp == 0   # a zero spacing has no reciprocal to verify


# ---- lookups ----------------------------------------------------------------------------
@pytest.mark.parametrize("pair,storage", CASES, ids=CASE_IDS)
def test_lookups_parity(gpu, pair, storage):
    """height / normal at test_height_and_normal_parity's points (on and beside
    the repeated lines too) from every coordinate source, and valid_states in
    stance and flight."""
    data, T, O = terrain_pair(pair, storage)
    xy = G.lookup_points(data)
    rh, rnan, rood = O.height_batch(xy, nthreads=8)
    rn, rnood = O.normal_batch(xy, nthreads=8)
    assert 0 < rood.sum() < len(rood)
    try:
        for coords in (1, 2, 0):
            T.set_option(L.OPT_LDS_COORDS, 1 if coords == 1 else 0)
            T.set_option(L.OPT_AFFINE_COORDS, 1 if coords == 2 else 0)
            h, nan, ood = T.height(torch.from_numpy(xy))
            assert np.array_equal(np_(ood), rood), coords
            assert np.array_equal(np_(nan), rnan), coords
            assert np.all(same_f64(np_(h), rh)), (coords, np.flatnonzero(~same_f64(np_(h), rh))[:10])
            nrm, nood = T.normal(torch.from_numpy(xy))
            assert np.array_equal(np_(nood), rnood), coords
            ok = rnood == 0
            assert np.array_equal(bits(np_(nrm)[ok]), bits(rn[ok])), coords
    finally:
        T.set_option(L.OPT_LDS_COORDS, 1)
        T.set_option(L.OPT_AFFINE_COORDS, 1)
    st, _ = O.sample_states(8192, 11, 7, 0, -1, 1, nthreads=8)
    # centres on and beside grid lines (the repeated ones among them)
    k = min(len(st), 3 * (data.x.size + data.y.size))
    lines = np.concatenate([data.x, np.nextafter(data.x, -np.inf), np.nextafter(data.x, np.inf)])
    st[:lines.size, 0] = lines
    lines = np.concatenate([data.y, np.nextafter(data.y, -np.inf), np.nextafter(data.y, np.inf)])
    st[k - lines.size:k, 1] = lines
    m = np.uint32(~(L.F_FRAGILE | L.F_RESOLVED) & 0xFFFFFFFF)
    for phase in (L.STANCE, L.FLIGHT):
        v, f, c = T.valid_states(torch.from_numpy(st), phase)
        rv, rf, rc = O.valid_states(st, phase, nthreads=8)
        frag = (u32(f) & L.F_FRAGILE) != 0
        # the host entry re-decides FRAGILE states with glibc: every state matches
        hv, hf, hc = T.valid_states_host(st, phase)
        assert np.array_equal(hv, rv) and np.array_equal(hf & m, rf & m) and np.array_equal(hc, rc)
        assert np.array_equal(np_(v)[~frag], rv[~frag])
        assert np.array_equal(u32(f)[~frag] & m, rf[~frag] & m)
        assert np.array_equal(u32(c)[~frag], rc[~frag])
        assert rv.sum() > 0


# ---- the hot path -----------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("kernel", [L.KERNEL_DIRECT, L.KERNEL_PERSISTENT])
@pytest.mark.parametrize("pair,storage", CASES, ids=CASE_IDS)
def test_validate_pairs_parity(gpu, pair, storage, kernel, adaptive):
    """8,192 attempts through the direct and the persistent kernel at 2 and 4
    waves (the direct kernel also with its coordinates in global memory)."""
    data, T, O = terrain_pair(pair, storage)
    s, a, d, refs = pair_batch(pair, O)
    ref = refs[adaptive]
    n = len(d)
    assert ref[0].sum() > 0
    variants = [(2, 1), (4, 1)] + ([(2, 0)] if kernel == L.KERNEL_DIRECT else [])
    T.set_option(L.OPT_KERNEL, kernel)
    try:
        for waves, lds in variants:
            T.set_option(L.OPT_WAVES, waves)
            T.set_option(L.OPT_LDS_COORDS, lds)
            res = T.validate_pairs(torch.from_numpy(s), torch.from_numpy(a), torch.from_numpy(d),
                                   adaptive=adaptive)
            gpu_t = (np_(res.valid), np_(res.s_new), np_(res.t_new), u32(res.flags), u32(res.counts))
            nfrag = assert_pairs_equal(gpu_t, ref, f"{data.name}/k{kernel}/ad{adaptive}/w{waves}/l{lds}",
                                       resolve=resolver(T, s, a, d, adaptive))
            assert nfrag <= n * 1e-3
    finally:
        T.set_option(L.OPT_WAVES, 2)
        T.set_option(L.OPT_LDS_COORDS, 1)
        T.set_option(L.OPT_KERNEL, L.KERNEL_PERSISTENT)


@pytest.mark.parametrize("pair,storage", CASES, ids=CASE_IDS)
def test_validate_pairs_host_entry(gpu, pair, storage):
    """The host entry re-decides FRAGILE attempts itself (std::upper_bound on
    the host copy of the vectors): its outputs are final."""
    data, T, O = terrain_pair(pair, storage)
    s, a, d, refs = pair_batch(pair, O)
    out = T.validate_pairs_host(s, a, d)
    assert_pairs_equal(out, refs[False], f"host {data.name}", resolve=lambda g: g)


# ---- extend -----------------------------------------------------------------------------
def test_extend_parity(gpu):
    data, T, O = terrain_pair(("graded", "twostep"))
    n = 4096
    s_near, _, d, target, _ = attempts_oracle(O, n, seed=41)
    base = 1000
    r = T.extend(torch.from_numpy(s_near), torch.from_numpy(target), torch.from_numpy(d),
                 seed=41, extend_base=base)
    # the engine's candidate actions, regenerated through the public sampler:
    # candidate j of extend i is stream EXTD (0x45585444), index (base+i)*8+j
    nrm = O.normal_batch(target[:, :2])[0]
    dense = np_(T.sample_actions(torch.from_numpy(np.repeat(nrm, 8, axis=0)), 41, 0x45585444,
                                 base * 8)).reshape(n, 8, 10)
    cand = np.ascontiguousarray(dense[:, :6])
    rr, rch, rsn, ran, rc = O.extend_batch(s_near, target, cand, d, nthreads=8)
    assert np.array_equal(np_(r.result), rr)
    assert np.array_equal(np_(r.chosen), rch)
    assert np.array_equal(u32(r.counts), rc)
    acc = rr != L.TRAPPED
    assert np.array_equal(bits(np_(r.s_new)[acc]), bits(rsn[acc]))
    assert np.array_equal(bits(np_(r.a_new)[acc]), bits(ran[acc]))
    assert (rch >= 0).sum() > 0


def test_samplers_match_oracle(gpu):
    """The state sampler's stance filter looks heights up with bracket()."""
    data, T, O = terrain_pair(("dups", "jitter"))
    n = 8192
    g, gt = T.sample_states(n, 31, 1, 0, require_phase=L.STANCE, max_tries=256)
    r, rt = O.sample_states(n, 31, 1, 0, L.STANCE, 256, nthreads=8)
    assert np.array_equal(np_(gt), rt)
    assert np.all(same_f64(np_(g), r))
    assert (rt > 1).sum() > 0


# ---- the planner loop -------------------------------------------------------------------
PLAN = {
    # terrain: (start x, y, goal x, y), seed, max_halves, vertices both trees pass
    ("graded", "twostep"): ((11.26, 2.76, 1.45, 1.45), 3, 5000, 100),
    ("dups", "uniform"): ((0.77, 0.31, 2.39, 3.97), 1, 4000, 50),
    ("graded", "twostep", "ripple"): ((13.45, 1.14, 5.19, 4.58), 3, 2000, 60),
}
STAR = ((8.71, 1.61, 11.56, 0.64), 5, 200)   # graded x twostep, batch 256
BOX = (0.3, 3.0, 9.0, 1.0, 3.0)              # graded x twostep: z + 0.3 for x in [3, 9], y in [1, 3]
_plans = {}


def oracle_plan(pair):
    if pair not in _plans:
        data, _, O = terrain_pair(pair)
        xy, seed, halves, _ = PLAN[pair]
        start, goal = _start_goal(O, *xy)
        ref = O.plan(start, goal, batch=64, seed=seed, max_halves=halves, nthreads=8)
        _plans[pair] = (data, O, start, goal, seed, halves, ref)
    return _plans[pair]


@pytest.mark.parametrize("algorithm", [3, 0])
@pytest.mark.parametrize("pair", list(PLAN), ids=[G.terrain_id(p) for p in PLAN])
def test_planner_loop_equals_oracle(gpu, pair, algorithm):
    """The device-resident search (3) and the host-driven one (0) at batch 64
    against orc_plan: targets, nearest vertices, extends, connects, the stance
    filter and every pair check on the general bracket search.

    Chosen on the CPU (oracle runs of 3-5 s, 8 threads):
      graded x twostep  (11.26, 2.76) -> (1.45, 1.45), seed 3: found after
        4,604 halves, trees of 105 + 115 vertices;
      dups x uniform    (0.77, 0.31) -> (2.39, 3.97), seed 1: found after 3,495
        halves, trees of 57 + 81 vertices.  On this 5 m map every search tried
        (60 start / goal pairs, 4 seeds, 4,000 halves) connects or stalls
        before both trees reach 100 vertices; this is the largest pair found;
      graded x twostep, rippled heights  (13.45, 1.14) -> (5.19, 4.58), seed 3:
        found after 1,290 halves, trees of 63 + 61 vertices, two of tree a's in
        the last cell of x (a bracket one cell off changes the trees here; on
        the block-flat heights above it mostly does not)."""
    data, O, start, goal, seed, halves, ref = oracle_plan(pair)
    dev = planner.plan_rrt_connect(data, start, goal, algorithm=algorithm, batch=64, max_time=300.0,
                                   seed=seed, max_halves=halves, trees=True)
    assert dev["found"] == ref["found"] == 1
    assert_counters_equal(dev, ref)
    assert_trees_equal(dev, ref)
    assert (dev["meet_a"], dev["meet_b"]) == (ref["meet_a"], ref["meet_b"])
    assert np.array_equal(bits(dev["states"]), bits(ref["states"]))
    assert np.array_equal(bits(dev["actions"]), bits(ref["actions"]))
    assert dev["reported_length"] == ref["path_length"]
    assert dev["path_cost"] == ref["path_length"]
    assert dev["reported_yaw"] == ref["path_yaw"]
    assert min(len(ref["a"]["v"]), len(ref["b"]["v"])) > PLAN[pair][3]
    print(f"{data.name} alg {algorithm}: {ref['halves']} halves, trees {len(ref['a']['v'])}+"
          f"{len(ref['b']['v'])}, {ref['attempts']} pair checks, {dev['fragile_resolved']} re-decided")


def test_post_process_equals_oracle(gpu):
    """postProcessPath on graded x twostep's found path (k_shortcut_pairs and
    the host walk): 46 states shortcut to 7, path_length_ 10.41 against
    path_cost_ 10.74 (the walk's fallback branch ran)."""
    data, O, start, goal, seed, halves, raw = oracle_plan(("graded", "twostep"))
    ps, pa, plen, pyaw, pcost = O.post_process_path(raw["states"], raw["actions"])
    dev = planner.plan_rrt_connect(data, start, goal, batch=64, max_time=300.0, seed=seed,
                                   max_halves=halves, algorithm=3, post_process=True)
    assert dev["found"] == 1
    assert 2 < ps.shape[0] < raw["states"].shape[0]
    assert np.array_equal(bits(dev["states"]), bits(ps))
    assert np.array_equal(bits(dev["actions"]), bits(pa))
    assert dev["reported_length"] == plen
    assert dev["reported_yaw"] == pyaw
    assert dev["path_cost"] == pcost
    print(f"{data.name}: {raw['states'].shape[0]} -> {ps.shape[0]} states")


def test_rrt_star_equals_oracle(gpu):
    """RRT*-Connect resident on the device (algorithm 5) on graded x twostep:
    (8.71, 1.61) -> (11.56, 0.64), seed 5, batch 256, 200 halves: trees of
    73 + 52 vertices, 11 rewires, 9 connections (oracle: 0.7 s)."""
    data, _, O = terrain_pair(("graded", "twostep"))
    xy, seed, halves = STAR
    start, goal = _start_goal(O, *xy)
    dev = planner.plan_rrt_star_connect(data, start, goal, batch=256, max_time=600.0, seed=seed,
                                        max_halves=halves, trees=True, device_loop=True)
    ref = O.plan(start, goal, batch=256, seed=seed, max_halves=halves, star=True, stream_a=401,
                 stream_b=402, nthreads=8)
    assert dev["halves"] == ref["halves"] == halves
    assert dev["found"] == ref["found"] == 1
    assert dev["rewires"] == ref["rewires"] > 0
    assert dev["solutions"] == ref["solutions"]
    assert_counters_equal(dev, ref)
    assert_trees_equal(dev, ref)
    assert (dev["meet_a"], dev["meet_b"]) == (ref["best_a"], ref["best_b"])
    assert dev["path_cost"] == ref["best_cost"]


# ---- prune ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [p for p in PLAN if p[0] == "graded"],
                         ids=[G.terrain_id(p) for p in PLAN if p[0] == "graded"])
def test_revalidate_after_a_height_change(gpu, pair):
    """graded x twostep's trees revalidated on the map with a raised box
    (the prune's pair checks), against the restatement in prune_ref.py: tree a
    keeps 71 of 105 vertices (3 of the pruned through an ancestor only), tree b
    40 of 115 (8); with the rippled heights 41 of 63 and 30 of 61."""
    import global_body_planner_amd as gbp
    from tests.test_gpu_tree_prune import assert_prune_equals, device_prune
    data, O, start, goal, seed, halves, ref = oracle_plan(pair)
    dz, x0, x1, y0, y1 = BOX
    z = np.array(data.z, np.float64)
    z[np.ix_((data.x >= x0) & (data.x <= x1), (data.y >= y0) & (data.y <= y1))] += dz
    changed = dataclasses.replace(data, z=z, name=data.name + "-box")
    T2 = gbp.Terrain.from_data(changed, device=0)
    O2 = oracle.OracleTerrain.from_data(changed)
    pruned = 0
    for name, direction in (("a", L.FORWARD), ("b", L.REVERSE)):
        tree = ref[name]
        ok = R.edge_valid(O2, tree, direction)
        want = R.prune(tree, ok)
        dev = device_prune(T2, tree, direction)
        assert_prune_equals(dev, want, (data.name, name))
        pruned += want[2]["n_before"] - want[2]["n_kept"]
        print(f"tree {name}: {dev[2]}")
        assert want[2]["n_kept"] > 1
    assert pruned > 0
