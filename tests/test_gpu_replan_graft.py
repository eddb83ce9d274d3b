"""ReplanSession::robotOff / goalAt (include/gbp_planner.h) and
planner.ReplanSession.robot_off / goal_at: RRT*-Connect kept on the device
while the robot leaves its tree and the goal moves, on synth-rough-256.

tests/integration/replan_graft_node.cpp runs the scenario once through the C++
class and writes every intermediate state (trees, list of kept connections,
best, paths, counters); py_scenario below produces the same records through
planner.ReplanSession.  Each test runs on both and compares one step with the
oracle's search, tests/graft_ref.py and tests/shared_ref.py, bit for bit.

The input: batch 1,024, seed 3, 300 halves (target streams 401 / 402, the
device RRT*'s): 110 + 86 vertices and 6 kept connections.  The robot is then
half way along the edge into start-tree vertex 5 (7 vertices attached, 34 kept,
one connection survives), the goal at goal-tree vertex 30's state shifted by
(+0.05, -0.03) on the ground (23 attached, 42 kept, the last connection goes),
and 100 more halves find new ones: found on the CPU with the oracle.
"""
import subprocess

import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from tests import graft_ref as G
from tests import prune_ref as R
from tests import shared_ref as SR
from tests.helpers import bits
from tests.test_gpu_replan_session import assert_list, list_of, path_of, read_records, tree_of
from tests.test_gpu_tree_prune import assert_same_tree

pytestmark = pytest.mark.gpu

BATCH, SEED, H, H2, RADIUS = 1024, 3, 300, 100, 3.0
STAR = dict(star=True, stream_a=401, stream_b=402, batch=BATCH, seed=SEED, nthreads=16)


@pytest.fixture(scope="module")
def ref():
    """The oracle's side of every step."""
    _, O = R.terrain(None)
    oracle.set_scan_mode(1)
    start, goal = R.start_goal()
    r1 = O.plan(start, goal, max_halves=H, **STAR)
    assert (len(r1["a"]["v"]), len(r1["b"]["v"]), r1["solutions"]) == (110, 86, 6)
    same = np.abs(r1["a"]["v"][:, None, :] - r1["b"]["v"][None, :, :]).max(axis=2) < 1e-9
    out = dict(r1=r1, met={(int(a), int(b)) for a, b in np.argwhere(same)}, O=O, start=start, goal=goal)
    out["root_a"] = G.mid_edge(r1["a"], 5, G.FORWARD)
    out["root_b"] = G.on_ground(O, r1["b"]["v"][30], 0.05, -0.03)
    out["goal_shift"] = np.array(goal, np.float64)
    out["goal_shift"][:2] += (0.10, 0.05)
    out["bad"] = np.array(start, np.float64)
    out["bad"][2] -= 1.0          # a metre under the ground: valid in no phase
    for key, phases in (("root_a", (1,)), ("root_b", (1, 0)), ("goal_shift", (0,))):
        assert any(O.valid_states(out[key][None], ph)[0][0] for ph in phases), key
    assert not O.valid_states(out["goal_shift"][None], 1)[0][0]   # a goal in FLIGHT alone
    assert not any(O.valid_states(out["bad"][None], ph)[0][0] for ph in (0, 1))
    out["ga"] = G.graft_on(O, r1["a"], out["root_a"], RADIUS, G.FORWARD)
    out["gb"] = G.graft_on(O, r1["b"], out["root_b"], RADIUS, G.REVERSE)
    out["g5"] = G.graft_on(O, r1["b"], out["goal_shift"], RADIUS, G.REVERSE)
    assert (out["ga"][2]["n_attached"], out["ga"][2]["n_kept"]) == (7, 34)
    assert (out["gb"][2]["n_attached"], out["gb"][2]["n_kept"]) == (23, 42)
    assert (out["g5"][2]["n_attached"], out["g5"][2]["n_kept"], out["g5"][2]["n_candidates"]) == (0, 1, 73)
    return out


def py_scenario(ref):
    """The same scenario through planner.ReplanSession (Python over the engine's
    entries), in the records replan_graft_node.cpp writes."""
    from global_body_planner_amd import engine, planner
    data, _ = R.terrain(None)
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

    def put_graft(tag, out):
        rec[tag + ".ok"] = np.array([int(out is not None)])
        rec[tag + ".graft"] = np.array([out[0][k] for k in G.STATS])
        rec[tag + ".shared"] = np.array([out[1][k] for k in SR.STATS])

    kw = dict(batch=BATCH, seed=SEED)
    T = engine.Terrain.from_data(data, storage=L.STORAGE_F64)
    s = planner.ReplanSession(T).begin(ref["start"], ref["goal"], **kw)
    s.search(1e9, H)
    put_state("s1", s)
    st = s.status
    rec["s1.counters"] = np.array([s.half, st["n_shared"], st["stat_rewires"], s.half, st["ext_counter"]])
    rec["s1b.ok"] = np.array([int(s.robot_off(ref["bad"], RADIUS) is not None),
                              int(s.goal_at(ref["bad"], RADIUS) is not None)])
    put_state("s1b", s)
    put_graft("s2", s.robot_off(ref["root_a"], RADIUS))
    put_state("s2", s)
    put_path("s2.path", s)
    put_graft("s3", s.goal_at(ref["root_b"], RADIUS))
    put_state("s3", s)
    put_path("s3.path", s)
    rec["s3.counters"] = np.array([s.half, s.status["ext_counter"]])
    h0 = s.half
    s.search(1e9, H2)
    put_state("s4", s)
    st = s.status
    rec["s4.counters"] = np.array([s.half - h0, st["n_shared"], st["stat_rewires"], s.half,
                                   st["ext_counter"]])
    put_path("s4.path", s)
    s.end()
    T5 = engine.Terrain.from_data(data, storage=L.STORAGE_F64)
    s5 = planner.ReplanSession(T5).begin(ref["start"], ref["goal"], **kw)
    s5.search(1e9, H)
    put_graft("s5", s5.goal_at(ref["goal_shift"], RADIUS))
    put_state("s5", s5)
    put_path("s5.path", s5)
    return rec


@pytest.fixture(scope="module", params=["cpp", "python"])
def scenario(request, gpu, ref, tmp_path_factory):
    if request.param == "python":
        return py_scenario(ref)
    from tests.test_abi import build_node_callsite
    d = tmp_path_factory.mktemp("replan_graft")
    exe = build_node_callsite(d / "replan_graft_node", src="replan_graft_node.cpp")
    data, _ = R.terrain(None)
    nx, ny = data.z.shape
    slopes = data.dx is not None
    with open(d / "input.bin", "wb") as f:
        f.write(np.array([nx, ny, int(slopes)], np.int32).tobytes())
        for arr in (data.x, data.y, data.z) + ((data.dx, data.dy, data.dz) if slopes else ()):
            f.write(np.ascontiguousarray(arr, np.float64).tobytes())
        states = [ref[k] for k in ("start", "goal", "root_a", "root_b", "goal_shift", "bad")]
        f.write(np.ascontiguousarray(np.concatenate(states), np.float64).tobytes())
        f.write(np.array([RADIUS], np.float64).tobytes())
        f.write(np.array([BATCH, H, H2], np.int32).tobytes())
        f.write(np.array([SEED], np.uint64).tobytes())
    out = subprocess.run(["timeout", "-k", "10", "120", exe, str(d / "input.bin"), str(d / "output.bin")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return read_records(d / "output.bin")


def assert_state_equals(scenario, tag, other):
    for name in "ab":
        assert_same_tree(tree_of(scenario, tag, name), tree_of(scenario, other, name), (tag, other, name))
    a, b = list_of(scenario, tag), list_of(scenario, other)
    assert_list(a, b[0], b[1] + (b[2],), (tag, other))


# ---- 1: begin + search, and a root that is valid nowhere ---------------------------------------
def test_search_and_an_invalid_root(scenario, ref):
    r1 = ref["r1"]
    for name in "ab":
        assert_same_tree(tree_of(scenario, "s1", name), r1[name], ("session", name))
    pairs, best, cost = list_of(scenario, "s1")
    assert {tuple(p) for p in pairs.tolist()} == ref["met"] and len(pairs) == 6
    assert best == (r1["best_a"], r1["best_b"]) and bits(cost) == bits(r1["best_cost"])
    assert list(scenario["s1b.ok"]) == [0, 0]
    assert_state_equals(scenario, "s1b", "s1")


# ---- 2: the robot is off the tree ----------------------------------------------------------------
def step2(scenario, ref):
    ta, remap, stats, _ = ref["ga"]
    pairs, shared = SR.remap_pairs(list_of(scenario, "s1")[0], remap, None)
    return ta, ref["r1"]["b"], pairs, shared, SR.rank(pairs, ta["g"], ref["r1"]["b"]["g"]), stats


def test_robot_off_grafts_the_start_tree_and_carries_the_list(scenario, ref):
    ta, tb, pairs, shared, best, stats = step2(scenario, ref)
    assert int(scenario["s2.ok"][0]) == 1
    assert [int(x) for x in scenario["s2.graft"]] == [stats[k] for k in G.STATS]
    assert_same_tree(tree_of(scenario, "s2", "a"), ta, "grafted a")
    assert_same_tree(tree_of(scenario, "s2", "b"), tb, "b untouched")
    assert [int(x) for x in scenario["s2.shared"]] == [shared[k] for k in SR.STATS]
    assert (shared["n_before"], shared["n_kept"]) == (6, 1)
    assert_list(list_of(scenario, "s2"), pairs, best, "carried through the graft")
    found, states, actions, lyc = path_of(scenario, "s2.path")
    assert found and np.array_equal(bits(states[0]), bits(ref["root_a"]))
    assert np.array_equal(bits(states[-1]), bits(ref["goal"]))
    ws, wa, wlen, na, nb = SR.join(ta, best[0], tb, best[1])
    assert np.array_equal(bits(states), bits(ws)) and np.array_equal(bits(actions), bits(wa))
    assert bits(lyc[0]) == bits(ta["g"][best[0]] + tb["g"][best[1]]) == bits(best[2])
    # the path's first edge is a connect action from the new root, valid on the map
    assert ta["parent"][SR.chain(ta["parent"], best[0])[1]] == 0
    assert ref["O"].validate_pairs(states[:1], actions[:1], L.FORWARD)[0][0] == 1


# ---- 3: the goal moved -----------------------------------------------------------------------------
def step3(scenario, ref):
    ta, _, pairs, _, _, _ = step2(scenario, ref)
    tb, remap, stats, _ = ref["gb"]
    pairs3, shared = SR.remap_pairs(pairs, None, remap)
    return ta, tb, pairs3, shared, SR.rank(pairs3, ta["g"], tb["g"]), stats


def test_goal_at_grafts_the_goal_tree_and_carries_the_list(scenario, ref):
    ta, tb, pairs, shared, best, stats = step3(scenario, ref)
    assert int(scenario["s3.ok"][0]) == 1
    assert [int(x) for x in scenario["s3.graft"]] == [stats[k] for k in G.STATS]
    assert_same_tree(tree_of(scenario, "s3", "a"), ta, "a untouched")
    assert_same_tree(tree_of(scenario, "s3", "b"), tb, "grafted b")
    assert [int(x) for x in scenario["s3.shared"]] == [shared[k] for k in SR.STATS]
    assert_list(list_of(scenario, "s3"), pairs, best, "carried through the goal's graft")
    assert len(pairs) == 0 and best == (-1, -1, np.inf)    # the last connection hung outside
    found, states, actions, _ = path_of(scenario, "s3.path")
    assert not found and len(states) == 0
    assert list(scenario["s3.counters"]) == [H, ref["r1"]["ext_counter"]]


# ---- 4: the search goes on -------------------------------------------------------------------------
def test_resumed_search_equals_the_oracles_continuation(scenario, ref):
    ta, tb, pairs3, _, _, _ = step3(scenario, ref)
    init = tuple({key: t[key] for key in ("v", "act", "parent")} for t in (ta, tb))
    r4 = ref["O"].plan(ta["v"][0], tb["v"][0], init_trees=init, max_halves=H2, first_half=H,
                       extend_base=ref["r1"]["ext_counter"], **STAR)
    for name in "ab":
        assert_same_tree(tree_of(scenario, "s4", name), r4[name], ("continued", name))
    pairs4, best4, cost4 = list_of(scenario, "s4")
    assert len(pairs4) == len(pairs3) + r4["solutions"] and r4["solutions"] >= 1
    halves, solutions, rewires, half, ext = (int(x) for x in scenario["s4.counters"])
    assert (halves, solutions, half) == (H2, len(pairs4), H + H2)
    assert rewires == ref["r1"]["rewires"] + r4["rewires"] and ext == r4["ext_counter"]
    assert best4 == (r4["best_a"], r4["best_b"]) and bits(cost4) == bits(r4["best_cost"])
    found, states, actions, lyc = path_of(scenario, "s4.path")
    ws, wa, wlen, na, nb = SR.join(r4["a"], best4[0], r4["b"], best4[1])
    assert found and np.array_equal(bits(states), bits(ws)) and np.array_equal(bits(actions), bits(wa))
    assert np.array_equal(bits(states[0]), bits(ref["root_a"]))
    assert np.array_equal(bits(states[-1]), bits(ref["root_b"]))
    print(f"continued: {r4['solutions']} new connections, best {cost4!r}, {r4['rewires']} rewires, "
          f"{len(r4['a']['v'])} + {len(r4['b']['v'])} vertices")


# ---- 5: a goal that nothing connects to ----------------------------------------------------------------
def test_goal_at_can_leave_the_root_alone(scenario, ref):
    tb, remap, stats, _ = ref["g5"]
    assert int(scenario["s5.ok"][0]) == 1
    assert [int(x) for x in scenario["s5.graft"]] == [stats[k] for k in G.STATS]
    assert_same_tree(tree_of(scenario, "s5", "a"), ref["r1"]["a"], "a untouched")
    assert_same_tree(tree_of(scenario, "s5", "b"), tb, "the goal alone")
    assert len(tb["parent"]) == 1
    assert [int(x) for x in scenario["s5.shared"]] == [6, 0, 0, 6]
    pairs, best, cost = list_of(scenario, "s5")
    assert len(pairs) == 0 and best == (-1, -1) and cost == np.inf
    assert not path_of(scenario, "s5.path")[0]
