"""ReplanSession::setInformed / ReplanSession.informed (include/gbp_planner.h,
planner.py) on the session test's search (synth-rough-256, batch
1,024, seed 11, 200 halves).

tests/integration/replan_informed_node.cpp runs the scenario through the C++
class; py_scenario below produces the same records through
planner.ReplanSession.  The two must hold identical records, and each test
checks them against the public entries (informed_ellipse, the informed
sampler, the oracle's state check).
"""
import subprocess

import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from tests import prune_ref as R
from tests import trim_ref as TR
from tests.helpers import bits
from tests.test_gpu_replan_session import list_of, path_of, read_records, tree_of

pytestmark = pytest.mark.gpu

BATCH, SEED, H = TR.SESSION["batch"], TR.SESSION["seed"], TR.SESSION_HALVES
INF_FIELDS = ("active", "cost", "cx", "cy", "ux", "uy", "a", "b")


def inf_row(e):
    return np.array([float(getattr(e, k)) for k in INF_FIELDS])


def py_scenario():
    """The scenario through planner.ReplanSession, in replan_informed_node.cpp's records."""
    from global_body_planner_amd import engine, planner
    data, _ = R.terrain(None)
    start, goal = R.start_goal()
    rec = {}

    def put_state(tag, s):
        for name, t in zip("ab", s.dump()):
            rec[f"{tag}.{name}.v"], rec[f"{tag}.{name}.act"] = t["v"].ravel(), t["act"].ravel()
            rec[f"{tag}.{name}.parent"], rec[f"{tag}.{name}.g"] = t["parent"], t["g"]
        pairs, best, cost = s.shared_connections()
        rec[tag + ".pairs"] = np.asarray(pairs, np.int32).ravel()
        rec[tag + ".best"], rec[tag + ".best_cost"] = np.array(best, np.int64), np.array([cost])

    def put_path(tag, s):
        p = s.best_path()
        rec[tag + ".found"] = np.array([int(p is not None)])
        rec[tag + ".states"] = p["states"].ravel() if p else np.zeros(0)
        rec[tag + ".actions"] = p["actions"].ravel() if p else np.zeros(0)
        cost = s.status["best_cost"]
        rec[tag + ".length_yaw_cost"] = np.array([p["length"], p["yaw"], p["cost"], cost] if p
                                                 else [0.0, 0.0, 0.0, cost])
        return p

    kw = dict(batch=BATCH, seed=SEED)
    T = engine.Terrain.from_data(data, storage=L.STORAGE_F64)
    T2 = engine.Terrain.from_data(data, storage=L.STORAGE_F64)
    mark = L.Informed()
    mark.cost, mark.a = 42.0, 1.5
    T2.set_informed(mark)
    P, I = planner.ReplanSession(T), planner.ReplanSession(T2)
    I.informed = True
    rec["flags"] = np.array([int(P.informed), int(I.informed)])
    P.begin(start, goal, **kw)
    I.begin(start, goal, **kw)
    rec["inf_begin"] = inf_row(I.informed_state)
    sizes_p, sizes_i, held, calls = [], [], False, 0
    while not held and calls < H // 2:
        P.search(1e9, 2)
        held = I.search(1e9, 2)
        calls += 1
        put_state(f"first.P.{calls}", P)   # every dump and list on the way
        put_state(f"first.I.{calls}", I)
        sizes_p += [*P.known, P.status["n_shared"], P.status["ext_counter"]]
        sizes_i += [*I.known, I.status["n_shared"], I.status["ext_counter"]]
    rec["first.calls"] = np.array([calls, int(held)])
    rec["first.sizes_p"], rec["first.sizes_i"] = np.array(sizes_p), np.array(sizes_i)
    put_state("first.P", P)
    put_state("first.I", I)
    rec["first.inf"] = inf_row(I.informed_state)
    P.end()
    if H > 2 * calls:
        I.search(1e9, H - 2 * calls)
    put_state("s200", I)
    rec["s200.inf"] = inf_row(I.informed_state)
    rec["s200.half"] = np.array([I.half, I.status["stat_targets"]])
    I.search(1e9, 2)
    rec["nt"] = np.array([I.half, I.status["stat_targets"]])
    rec["py.n_targets"] = np.array([I.status["n_targets"]])   # the last half's own (Python only)
    costs, targets = [], []
    for _ in range(50):
        I.search(1e9, 2)
        costs.append(I.status["best_cost"])
        targets.append(I.status["stat_targets"])
    rec["costs"], rec["stat_targets"] = np.array(costs), np.array(targets)
    put_path("p_on", I)
    rec["p_on.inf"] = inf_row(I.informed_state)
    I.informed = False
    rec["p_off.inf"] = inf_row(I.informed_state)
    put_path("p_off", I)
    I.informed = True
    rec["p_on2.inf"] = inf_row(I.informed_state)
    p = put_path("p_on2", I)
    I.robot_at(p["states"][1])
    put_state("robot", I)
    rec["robot.inf"] = inf_row(I.informed_state)
    T2.update(np.full(data.z.shape, np.nan))
    I.map_changed()
    put_state("map", I)
    rec["map.inf"] = inf_row(I.informed_state)
    I.end()
    rec["inf_end"] = inf_row(T2.get_informed())
    rec["flags_end"] = np.array([int(I.informed)])
    return rec


def cpp_scenario(tmp_path_factory):
    from tests.test_abi import build_node_callsite
    d = tmp_path_factory.mktemp("replan_informed")
    exe = build_node_callsite(d / "replan_informed_node", src="replan_informed_node.cpp")
    data, _ = R.terrain(None)
    start, goal = R.start_goal()
    nx, ny = data.z.shape
    slopes = data.dx is not None
    with open(d / "input.bin", "wb") as f:
        f.write(np.array([nx, ny, int(slopes)], np.int32).tobytes())
        for arr in (data.x, data.y, data.z) + ((data.dx, data.dy, data.dz) if slopes else ()):
            f.write(np.ascontiguousarray(arr, np.float64).tobytes())
        f.write(np.ascontiguousarray(np.r_[start, goal], np.float64).tobytes())
        f.write(np.array([BATCH, H], np.int32).tobytes())
        f.write(np.array([SEED], np.uint64).tobytes())
    out = subprocess.run(["timeout", "-k", "10", "120", exe, str(d / "input.bin"), str(d / "output.bin")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return read_records(d / "output.bin")


@pytest.fixture(scope="module")
def both(gpu, tmp_path_factory):
    return dict(cpp=cpp_scenario(tmp_path_factory), python=py_scenario())


@pytest.fixture(scope="module", params=["cpp", "python"])
def rec(request, both):
    return both[request.param]


def bounds():
    data, _ = R.terrain(None)
    return (float(data.x[0]), float(data.x[-1]), float(data.y[0]), float(data.y[-1]))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float64 or b.dtype == np.float64:
        return np.array_equal(bits(a), bits(b))
    return np.array_equal(a, b)


def assert_ellipse_of(rec, inf_tag, state_tag):
    """the recorded ellipse is informed_ellipse(the recorded roots, best cost, bounds)"""
    a, b = tree_of(rec, state_tag, "a"), tree_of(rec, state_tag, "b")
    _, best, cost = list_of(rec, state_tag)
    assert best[0] >= 0 and best[1] >= 0
    e = L.informed_ellipse(a["v"][0], b["v"][0], cost, bounds())
    assert same(rec[inf_tag], inf_row(e)), (inf_tag, rec[inf_tag], inf_row(e))
    return e


def test_cpp_and_python_hold_identical_records(both):
    cpp, py = both["cpp"], both["python"]
    assert set(py) - set(cpp) == {"py.n_targets"} and set(cpp) <= set(py)
    for k in cpp:
        assert same(cpp[k], py[k]), k


def test_identical_to_the_plain_session_until_a_connection_is_held(rec):
    assert list(rec["flags"]) == [0, 1]
    assert rec["inf_begin"][0] == 0             # on, nothing held: the handle's ellipse is off
    calls, held = rec["first.calls"]
    assert held == 1 and calls >= 1
    assert same(rec["first.sizes_p"], rec["first.sizes_i"])
    # every dump and list, after every call up to and including the first held group
    for tag in [f".{c}" for c in range(1, calls + 1)] + [""]:
        for name in "ab":
            tp, ti = tree_of(rec, "first.P" + tag, name), tree_of(rec, "first.I" + tag, name)
            for k in tp:
                assert same(tp[k], ti[k]), (tag, name, k)
        lp, li = list_of(rec, "first.P" + tag), list_of(rec, "first.I" + tag)
        assert np.array_equal(lp[0], li[0]) and lp[1] == li[1] and bits(lp[2]) == bits(li[2]), tag
        assert (lp[1][0] >= 0) == (tag in ("", f".{calls}"))   # held at the last call only
    e = assert_ellipse_of(rec, "first.inf", "first.I")   # computed after that group's status read
    print(f"a connection after {2 * calls} halves, cost {li[2]:.4f}, ellipse active {e.active}")


def test_state_after_200_halves_is_the_ellipse_of_roots_and_best_cost(rec):
    assert rec["s200.half"][0] == H
    e = assert_ellipse_of(rec, "s200.inf", "s200")
    assert e.active == 1
    print(f"best cost {e.cost:.4f}: ellipse {3.14159 * e.a * e.b:.2f} m^2 of the map's 26.0")


def test_targets_of_a_group_are_the_public_samplers_valid_draws(rec, both):
    """The group after the 200 halves ran under the recorded ellipse: its two
    halves' targets are the STANCE-valid rows (the oracle's decision) among the
    informed sampler's draws for each half's stream and index base."""
    from global_body_planner_amd import engine
    data, _ = R.terrain(None)
    O = oracle.OracleTerrain.from_data(data)
    T = engine.Terrain.from_data(data, storage=L.STORAGE_F64)
    e = L.Informed(*[int(rec["s200.inf"][0]), 0, *[float(v) for v in rec["s200.inf"][1:]]])
    assert e.active == 1
    half, before = (int(v) for v in rec["s200.half"])
    assert int(rec["nt"][0]) == half + 2
    counts = []
    for h in (half, half + 1):
        g = T.sample_states_informed(BATCH, SEED, 402 if h & 1 else 401, index_base=(h >> 1) * BATCH,
                                     inf=e).cpu().numpy()
        counts.append(int(O.valid_states(g, L.STANCE, nthreads=8)[0].sum()))
    assert int(rec["nt"][1]) - before == sum(counts), (rec["nt"], before, counts)
    assert int(both["python"]["py.n_targets"][0]) == counts[1]   # the status's own n_targets
    plain = [int(O.valid_states(T.sample_states(BATCH, SEED, 402 if h & 1 else 401,
                                                (h >> 1) * BATCH)[0].cpu().numpy(), L.STANCE,
                                nthreads=8)[0].sum()) for h in (half, half + 1)]
    print(f"targets of halves {half}, {half + 1}: {counts} (plain draws: {plain})")
    assert counts != plain


def test_best_cost_never_rises_and_the_search_goes_on(rec):
    costs = np.r_[list_of(rec, "s200")[2], rec["costs"]]
    assert np.all(np.diff(costs) <= 0), costs
    t = np.r_[rec["nt"][1], rec["stat_targets"]]
    assert np.all(np.diff(t) > 0)               # every group drew valid targets
    print(f"best cost {costs[0]:.4f} -> {costs[-1]:.4f} over 100 halves, "
          f"{(t[-1] - t[0]) / 100:.0f} targets per half")


def test_best_path_is_the_same_with_the_property_toggled(rec):
    on, off, on2 = path_of(rec, "p_on"), path_of(rec, "p_off"), path_of(rec, "p_on2")
    assert on[0] and off[0] and on2[0]
    for other in (off, on2):
        for x, y in zip(on[1:], other[1:]):
            assert same(x, y)
    assert rec["p_on.inf"][0] == 1
    # off: what the handle held at begin is back at once; on again: the ellipse of the status
    assert same(rec["p_off.inf"], [0.0, 42.0, 0.0, 0.0, 0.0, 0.0, 1.5, 0.0])
    assert same(rec["p_on2.inf"], rec["p_on.inf"])


def test_robot_at_moves_the_focus(rec):
    _, states, _, _ = path_of(rec, "p_on2")
    a = tree_of(rec, "robot", "a")
    assert same(a["v"][0], states[1])           # the new root: the path's second state
    e = assert_ellipse_of(rec, "robot.inf", "robot")
    assert not same(rec["robot.inf"], rec["p_on2.inf"])
    assert e.cost < rec["p_on2.inf"][1]         # the remaining path is shorter


def test_map_change_that_drops_the_best_connection_turns_it_off(rec):
    pairs, best, _ = list_of(rec, "map")
    assert len(pairs) == 0 and best == (-1, -1)
    assert rec["map.inf"][0] == 0


def test_end_restores_the_handles_setting(rec):
    assert same(rec["inf_end"], [0.0, 42.0, 0.0, 0.0, 0.0, 0.0, 1.5, 0.0])
    assert list(rec["flags_end"]) == [1]        # the property is the object's: it outlives end
