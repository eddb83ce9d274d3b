"""ReplanSession (include/gbp_planner.h): RRT*-Connect kept on the device
through a map change, a step of the robot and a resumed search, on
synth-rough-256 with the box-1 changed map of tests/test_gpu_tree_prune.py.

tests/integration/replan_session_node.cpp runs the scenario once through the
C++ class and writes every intermediate state (trees, list of kept
connections, best, paths, counters); py_scenario below produces the same
records through planner.ReplanSession and plan_rrt_star_connect(init_shared=)
(Python over the engine's entries).  Each test runs on both and compares one
step with the
oracle's search, tests/prune_ref.py, tests/reroot_ref.py and
tests/shared_ref.py, bit for bit.

The input: batch 1,024, seed 11, 200 halves (target streams 401 / 402, the
device RRT*'s).  The oracle's run ends with 5 kept connections (the pairs of a
start-tree and a goal-tree vertex at the same state, one per REACHED connect),
of which 2 survive box 1 and 3 do not, the best among the 3: found on the CPU
with the oracle (seeds 3, 5 and 7 leave no survivor).
"""
import struct
import subprocess

import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from tests import prune_ref as R
from tests import reroot_ref as RR
from tests import shared_ref as SR
from tests.helpers import bits
from tests.test_gpu_tree_prune import assert_same_tree

pytestmark = pytest.mark.gpu

BATCH, SEED, H, H2 = 1024, 11, 200, 100
KEPT, SURVIVE = 5, 2
STAR = dict(star=True, stream_a=401, stream_b=402, batch=BATCH, seed=SEED, nthreads=16)


def read_records(path):
    out = {}
    with open(path, "rb") as f:
        blob = f.read()
    at = 0
    while at < len(blob):
        (ln,) = struct.unpack_from("<I", blob, at)
        name = blob[at + 4:at + 4 + ln].decode()
        kind = chr(blob[at + 4 + ln])
        (n,) = struct.unpack_from("<q", blob, at + 5 + ln)
        dt = {"d": np.float64, "i": np.int32, "q": np.int64}[kind]
        at += 13 + ln
        out[name] = np.frombuffer(blob, dt, n, at).copy()
        at += n * np.dtype(dt).itemsize
    return out


def tree_of(rec, tag, name):
    t = f"{tag}.{name}."
    return dict(v=rec[t + "v"].reshape(-1, 8), act=rec[t + "act"].reshape(-1, 10),
                parent=rec[t + "parent"], g=rec[t + "g"])


def list_of(rec, tag):
    return (rec[tag + ".pairs"].reshape(-1, 2), tuple(int(x) for x in rec[tag + ".best"]),
            float(rec[tag + ".best_cost"][0]))


def path_of(rec, tag):
    return (bool(rec[tag + ".found"][0]), rec[tag + ".states"].reshape(-1, 8),
            rec[tag + ".actions"].reshape(-1, 10), rec[tag + ".length_yaw_cost"])


def assert_list(got, pairs, best, label):
    gp, gb, gc = got
    assert gp.shape == np.asarray(pairs).reshape(-1, 2).shape and np.array_equal(gp, pairs), label
    assert gb == best[:2] and bits(gc) == bits(best[2]), (label, gb, gc, best)


def py_scenario():
    """The same scenario through planner.ReplanSession (Python over the engine's
    entries), in the records replan_session_node.cpp writes."""
    from global_body_planner_amd import engine, planner
    data, _ = R.terrain(None)
    boxed, _ = R.terrain("box1")
    start, goal = R.start_goal()
    rec = {}

    def put_trees(tag, trees):
        for name, t in zip("ab", trees):
            rec[f"{tag}.{name}.v"], rec[f"{tag}.{name}.act"] = t["v"].ravel(), t["act"].ravel()
            rec[f"{tag}.{name}.parent"], rec[f"{tag}.{name}.g"] = t["parent"], t["g"]

    def put_list(tag, pairs, best, cost):
        rec[tag + ".pairs"] = np.asarray(pairs, np.int32).ravel()
        rec[tag + ".best"], rec[tag + ".best_cost"] = np.array(best, np.int64), np.array([cost])

    def put_state(tag, s):
        put_trees(tag, s.dump())
        put_list(tag, *s.shared_connections())

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
    b = planner.plan_rrt_star_connect(data, start, goal, device_loop=True, max_time=1e9, max_halves=H,
                                      trees=True, **kw)
    put_trees("build", (b["a"], b["b"]))
    rec["build.best"], rec["build.best_cost"] = np.array([b["meet_a"], b["meet_b"]]), np.array([b["path_cost"]])
    rec["build.counters"] = np.array([b["halves"], b["solutions"], b["rewires"]])
    T = engine.Terrain.from_data(data, storage=L.STORAGE_F64)   # box 1's heights are not floats
    s = planner.ReplanSession(T).begin(start, goal, **kw)
    s.search(1e9, H)
    put_state("s1", s)
    st = s.status
    rec["s1.counters"] = np.array([s.half, st["n_shared"], st["stat_rewires"], s.half, st["ext_counter"]])
    changed = np.argwhere(bits(np.asarray(boxed.z)) != bits(np.asarray(data.z)))
    (ix0, iy0), (ix1, iy1) = changed.min(axis=0), changed.max(axis=0) + 1
    T.update(np.asarray(boxed.z)[ix0:ix1, iy0:iy1], ix0, iy0)
    pruned, shared = s.map_changed()
    for name, ps in zip("ab", pruned):
        rec[f"s2.prune.{name}"] = np.array([ps[k] for k in ("n_before", "n_kept", "n_edge_invalid",
                                                            "n_inherited")])
    rec["s2.shared"] = np.array([shared[k] for k in SR.STATS])
    put_state("s2", s)
    path = put_path("s2.path", s)
    rs, shared = s.robot_at(path["states"][1])
    rec["s3.reroot"] = np.array([rs[k] for k in RR.STATS])
    rec["s3.shared"] = np.array([shared[k] for k in SR.STATS])
    put_state("s3", s)
    put_path("s3.path", s)
    rec["s3.counters"] = np.array([s.half, s.status["ext_counter"]])
    d3, (list3, _, _), half3, ext3 = s.dump(), s.shared_connections(), s.half, s.status["ext_counter"]
    h0 = s.half
    s.search(1e9, H2)
    put_state("s4", s)
    st = s.status
    rec["s4.counters"] = np.array([s.half - h0, st["n_shared"], st["stat_rewires"], s.half,
                                   st["ext_counter"]])
    put_path("s4.path", s)
    s.end()
    w = planner.plan_rrt_star_connect(T, d3[0]["v"][0], goal, device_loop=True, init_shared=list3,
                                      init_trees=d3, first_half=half3, extend_base=ext3, max_time=1e9,
                                      max_halves=H2, **kw)
    put_trees("warm", (w["a"], w["b"]))
    put_list("warm", w["shared"], (w["meet_a"], w["meet_b"]), w["path_cost"])
    rec["warm.counters"] = np.array([w["halves"], w["solutions"], w["rewires"]])
    T6 = engine.Terrain.from_data(data, storage=L.STORAGE_F64)
    s6 = planner.ReplanSession(T6).begin(start, goal, **kw)
    s6.search(1e9, H)
    T6.update(np.asarray(data.z, np.float64) + 50.0)
    pruned, shared = s6.map_changed()
    rec["s6.kept"] = np.array([p["n_kept"] for p in pruned])
    rec["s6.shared"] = np.array([shared[k] for k in SR.STATS])
    put_state("s6", s6)
    put_path("s6.path", s6)
    return rec


@pytest.fixture(scope="module", params=["cpp", "python"])
def scenario(request, gpu, tmp_path_factory):
    if request.param == "python":
        return py_scenario()
    from tests.test_abi import build_node_callsite
    d = tmp_path_factory.mktemp("replan")
    exe = build_node_callsite(d / "replan_session_node", src="replan_session_node.cpp")
    data, _ = R.terrain(None)
    boxed, _ = R.terrain("box1")
    start, goal = R.start_goal()
    nx, ny = data.z.shape
    changed = np.argwhere(bits(np.asarray(boxed.z)) != bits(np.asarray(data.z)))
    (ix0, iy0), (ix1, iy1) = changed.min(axis=0), changed.max(axis=0) + 1
    slopes = data.dx is not None
    with open(d / "input.bin", "wb") as f:
        f.write(np.array([nx, ny, int(slopes)], np.int32).tobytes())
        for arr in (data.x, data.y, data.z) + ((data.dx, data.dy, data.dz) if slopes else ()):
            f.write(np.ascontiguousarray(arr, np.float64).tobytes())
        f.write(np.array([ix0, iy0, ix1 - ix0, iy1 - iy0], np.int32).tobytes())
        f.write(np.ascontiguousarray(np.asarray(boxed.z)[ix0:ix1, iy0:iy1], np.float64).tobytes())
        f.write(np.ascontiguousarray(np.r_[start, goal], np.float64).tobytes())
        f.write(np.array([BATCH, H, H2], np.int32).tobytes())
        f.write(np.array([SEED], np.uint64).tobytes())
    out = subprocess.run(["timeout", "-k", "10", "120", exe, str(d / "input.bin"), str(d / "output.bin")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return read_records(d / "output.bin")


@pytest.fixture(scope="module")
def ref():
    """The oracle's side of every step."""
    import oracle
    _, O = R.terrain(None)
    _, O1 = R.terrain("box1")
    oracle.set_scan_mode(1)
    start, goal = R.start_goal()
    r1 = O.plan(start, goal, max_halves=H, **STAR)
    same = np.abs(r1["a"]["v"][:, None, :] - r1["b"]["v"][None, :, :]).max(axis=2) < 1e-9
    out = dict(r1=r1, met={(int(a), int(b)) for a, b in np.argwhere(same)}, O1=O1, goal=goal)
    out["pruned"] = [R.prune(r1[n], R.edge_valid(O1, r1[n], d)) for n, d in (("a", 0), ("b", 1))]
    return out


# ---- 1: begin + search = the one-call build ----------------------------------------------------
def test_begin_and_search_equal_the_build(scenario, ref):
    r1 = ref["r1"]
    assert r1["solutions"] == KEPT == len(ref["met"])
    for name in "ab":
        assert_same_tree(tree_of(scenario, "build", name), r1[name], ("build", name))
        assert_same_tree(tree_of(scenario, "s1", name), r1[name], ("session", name))
    sess = list_of(scenario, "s1")
    if "build.pairs" in scenario:   # (the flat C entry behind the Python build returns no list)
        built = list_of(scenario, "build")
        assert_list(sess, built[0], built[1] + (built[2],), "session = build")
    assert sess[1] == tuple(int(x) for x in scenario["build.best"])
    assert bits(sess[2]) == bits(scenario["build.best_cost"][0])
    assert {tuple(p) for p in sess[0].tolist()} == ref["met"] and len(sess[0]) == KEPT
    assert sess[1] == (r1["best_a"], r1["best_b"]) and bits(sess[2]) == bits(r1["best_cost"])
    assert sess[1] == SR.rank(sess[0], r1["a"]["g"], r1["b"]["g"])[:2]
    assert list(scenario["s1.counters"][:3]) == [H, KEPT, r1["rewires"]]
    assert list(scenario["s1.counters"][3:]) == [H, r1["ext_counter"]]
    assert list(scenario["build.counters"]) == [H, KEPT, r1["rewires"]]


# ---- 2: the map changes ------------------------------------------------------------------------
def step2(scenario, ref):
    (ta, ra, sa), (tb, rb, sb) = ref["pruned"]
    pairs, stats = SR.remap_pairs(list_of(scenario, "s1")[0], ra, rb)
    return ta, tb, pairs, stats, SR.rank(pairs, ta["g"], tb["g"])


def test_map_change_prunes_both_trees_and_carries_the_list(scenario, ref):
    ta, tb, pairs, stats, best = step2(scenario, ref)
    for name, (t, remap, st), in zip("ab", ref["pruned"]):
        got = [int(x) for x in scenario[f"s2.prune.{name}"]]
        assert got == [st["n_before"], st["n_kept"], st["n_edge_invalid"], st["n_inherited"]], name
        assert st["n_kept"] < st["n_before"]
        assert_same_tree(tree_of(scenario, "s2", name), t, ("pruned", name))
    assert (stats["n_before"], stats["n_kept"]) == (KEPT, SURVIVE)
    assert [int(x) for x in scenario["s2.shared"]] == [stats[k] for k in SR.STATS]
    assert_list(list_of(scenario, "s2"), pairs, best, "carried")
    # the best of step 1 is among the dropped: a best that was only lowered would still name it
    old_best = list_of(scenario, "s1")[1]
    assert ref["pruned"][0][1][old_best[0]] < 0 or ref["pruned"][1][1][old_best[1]] < 0
    assert best[2] > list_of(scenario, "s1")[2]


def test_best_path_after_the_map_change(scenario, ref):
    ta, tb, pairs, stats, best = step2(scenario, ref)
    found, states, actions, lyc = path_of(scenario, "s2.path")
    ws, wa, wlen, na, nb = SR.join(ta, best[0], tb, best[1])
    assert found and np.array_equal(bits(states), bits(ws)) and np.array_equal(bits(actions), bits(wa))
    assert bits(lyc[0]) == bits(wlen) == bits(best[2]) and bits(lyc[2]) == bits(wlen) == bits(lyc[3])
    # the yaw: the oracle's sums along the two chains (a prune moves rows, it changes no chain)
    r1 = ref["r1"]
    oa = int(np.flatnonzero(ref["pruned"][0][1] == best[0])[0])
    ob = int(np.flatnonzero(ref["pruned"][1][1] == best[1])[0])
    assert bits(lyc[1]) == bits(r1["a"]["y"][oa] + r1["b"]["y"][ob])
    start, goal = R.start_goal()
    assert np.array_equal(bits(states[0]), bits(start)) and np.array_equal(bits(states[-1]), bits(goal))
    # every edge of the path holds on the new map: the start tree's FORWARD from
    # the edge's first state, the goal tree's REVERSE from its last
    fwd = ref["O1"].validate_pairs(states[:na - 1], actions[:na - 1], L.FORWARD)[0]
    rev = ref["O1"].validate_pairs(states[na:], actions[na - 1:], L.REVERSE)[0]
    assert len(fwd) + len(rev) == len(actions) and np.all(fwd == 1) and np.all(rev == 1)


# ---- 3: the robot steps --------------------------------------------------------------------------
def step3(scenario, ref):
    ta, tb, pairs, stats, best = step2(scenario, ref)
    k = SR.chain(ta["parent"], best[0])[1]          # the vertex of the path's second state
    ta3, remap, rstats = RR.reroot(ta, k)
    pairs3, stats3 = SR.remap_pairs(pairs, remap, None)
    return ta3, tb, pairs3, stats3, SR.rank(pairs3, ta3["g"], tb["g"]), rstats, k


def test_robot_step_reroots_the_start_tree_and_carries_the_list(scenario, ref):
    ta3, tb, pairs3, stats3, best3, rstats, k = step3(scenario, ref)
    assert [int(x) for x in scenario["s3.reroot"]] == [rstats[s] for s in RR.STATS]
    assert rstats["n_kept"] < rstats["n_before"]
    assert_same_tree(tree_of(scenario, "s3", "a"), ta3, "re-rooted a")
    assert_same_tree(tree_of(scenario, "s3", "b"), tb, "b untouched")
    assert [int(x) for x in scenario["s3.shared"]] == [stats3[s] for s in SR.STATS]
    assert stats3["n_kept"] >= 1
    assert_list(list_of(scenario, "s3"), pairs3, best3, "carried through the re-root")
    found, states, actions, lyc = path_of(scenario, "s3.path")
    second = path_of(scenario, "s2.path")[1][1]
    assert found and np.array_equal(bits(states[0]), bits(second))
    assert np.array_equal(bits(states[0]), bits(ta3["v"][0]))
    ws, wa, wlen, na, nb = SR.join(ta3, best3[0], tb, best3[1])
    assert np.array_equal(bits(states), bits(ws)) and np.array_equal(bits(actions), bits(wa))
    # the length is the derived g of the re-rooted tree, not the old one less g[k]
    assert bits(lyc[0]) == bits(ta3["g"][best3[0]] + tb["g"][best3[1]]) == bits(best3[2])
    assert list(scenario["s3.counters"]) == [H, ref["r1"]["ext_counter"]]


# ---- 4: the search goes on -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def continued(scenario, ref):
    ta3, tb, pairs3, stats3, best3, rstats, k = step3(scenario, ref)
    init = tuple({key: t[key] for key in ("v", "act", "parent")} for t in (ta3, tb))
    r4 = ref["O1"].plan(ta3["v"][0], ref["goal"], init_trees=init, max_halves=H2, first_half=H,
                        extend_base=ref["r1"]["ext_counter"], **STAR)
    return r4, pairs3, best3, ref["r1"]["rewires"]


def test_resumed_search_equals_the_oracles_continuation(scenario, continued):
    r4, pairs3, best3, rewires1 = continued
    for name in "ab":
        assert_same_tree(tree_of(scenario, "s4", name), r4[name], ("continued", name))
    pairs4, best4, cost4 = list_of(scenario, "s4")
    assert np.array_equal(pairs4[:len(pairs3)], pairs3)          # the carried ones, unchanged
    assert len(pairs4) == len(pairs3) + r4["solutions"]          # carried + new
    halves, solutions, rewires, half, ext = (int(x) for x in scenario["s4.counters"])
    assert (halves, solutions, half) == (H2, len(pairs4), H + H2)
    # (the session's counters are its totals: the first search's rewires and the continuation's)
    assert rewires == rewires1 + r4["rewires"] and ext == r4["ext_counter"]
    assert cost4 <= best3[2] and best4 in {tuple(p) for p in pairs4.tolist()}
    # rewiring only lowers g, so the cheapest of the final list is what the
    # ranking after the last half held (its pair may differ only on an exact tie)
    assert bits(cost4) == bits(SR.rank(pairs4, r4["a"]["g"], r4["b"]["g"])[2])
    found, states, actions, lyc = path_of(scenario, "s4.path")
    ws, wa, wlen, na, nb = SR.join(r4["a"], best4[0], r4["b"], best4[1])
    assert found and np.array_equal(bits(states), bits(ws)) and np.array_equal(bits(actions), bits(wa))
    assert bits(lyc[1]) == bits(r4["a"]["y"][best4[0]] + r4["b"]["y"][best4[1]])
    print(f"continued: {len(pairs3)} carried + {r4['solutions']} new connections, best {best3[2]!r} -> "
          f"{cost4!r}, {rewires} rewires")


# ---- 5: the same continuation as a warm start of the build ----------------------------------------
def test_warm_start_with_the_list_equals_the_session(scenario):
    for name in "ab":
        assert_same_tree(tree_of(scenario, "warm", name), tree_of(scenario, "s4", name), name)
    s4 = list_of(scenario, "s4")
    assert_list(list_of(scenario, "warm"), s4[0], s4[1] + (s4[2],), "warm start")
    assert [int(x) for x in scenario["warm.counters"]][:2] == [H2, len(s4[0])]


# ---- 6: a map change that leaves nothing ---------------------------------------------------------
def test_best_path_is_false_when_no_connection_survives(scenario):
    assert list(scenario["s6.kept"]) == [1, 1]                       # the roots alone
    assert [int(x) for x in scenario["s6.shared"]] == [KEPT, 0, KEPT, 0]
    pairs, best, cost = list_of(scenario, "s6")
    assert len(pairs) == 0 and best == (-1, -1) and cost == np.inf
    found, states, actions, _ = path_of(scenario, "s6.path")
    assert not found and len(states) == 0 and len(actions) == 0


# ---- 7: the node's sequence through the reference's names ------------------------------------------
def test_node_replan_on_the_slope_csv(gpu, tmp_path):
    """tests/integration/node_replan.cpp: plan, updateDataFlat of a rectangle,
    mapChanged, bestPath (the search resumed only if nothing survives),
    getInterpPath, on the slope CSV of config 1."""
    import json
    from tests.test_abi import build_node_callsite
    from tests.test_csv_ingest import write_csvs
    exe = build_node_callsite(tmp_path / "node_replan", src="node_replan.cpp")
    d = write_csvs("slope", tmp_path / "slope")
    r = subprocess.run(["timeout", "-k", "10", "100", exe, str(d), "1024", "3"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    x = json.loads(r.stdout.splitlines()[-1])
    print("node_replan", json.dumps(x))
    assert x["first_ok"] == 1 and x["second_ok"] == 1 and x["interp"] > x["second_states"]
    assert x["connections"] >= 1 and x["of_a"] >= x["kept_a"] >= 1 and x["of_b"] >= x["kept_b"] >= 1
