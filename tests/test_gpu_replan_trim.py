"""ReplanSession::trim and setTreeLimit (include/gbp_planner.h) on
the session test's search (synth-rough-256, batch 1,024, seed 11, 200 halves).

tests/integration/replan_trim_node.cpp runs the scenario through the C++ class
and writes every state; py_scenario below produces the same records through
planner.ReplanSession.  Each test runs on both and compares with the oracle's
search and tests/trim_ref.py, bit for bit.

The budgets: 0 (the bound alone: 36 + 40 of 61 + 71 vertices stay), 40 (35 and
39 vertices pass the bound, so this budget cuts nothing more) and 24 (the
budget cuts, and the best connection's chains are kept by the protection).
"""
import subprocess

import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from tests import prune_ref as R
from tests import shared_ref as SR
from tests import trim_ref as TR
from tests.helpers import bits
from tests.test_gpu_replan_session import (assert_list, list_of, path_of, read_records, tree_of)
from tests.test_gpu_tree_prune import assert_same_tree

pytestmark = pytest.mark.gpu

BATCH, SEED, H, H2 = TR.SESSION["batch"], TR.SESSION["seed"], TR.SESSION_HALVES, 100
BUDGETS = (0, 40, 24)
CALLS, LIMIT, TRIM_TO = 150, 48, 32
TRIM_FIELDS = ("n_before", "n_kept", "n_over_bound", "n_over_budget", "n_protected", "n_inherited")


def py_scenario():
    """The scenario through planner.ReplanSession, in replan_trim_node.cpp's records."""
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

    kw = dict(batch=BATCH, seed=SEED)
    T = engine.Terrain.from_data(data, storage=L.STORAGE_F64)
    for B in BUDGETS:
        tag = f"t{B}"
        s = planner.ReplanSession(T).begin(start, goal, **kw)
        s.search(1e9, H)
        put_state(tag + ".s1", s)
        put_path(tag + ".p1", s)
        stats, shared = s.trim(B)
        for name, ts in zip("ab", stats):
            rec[f"{tag}.trim.{name}"] = np.array([ts[k] for k in TRIM_FIELDS])
            rec[f"{tag}.trim.{name}.cut"] = np.array([ts["cut"]])
        rec[tag + ".trim.shared"] = np.array([shared[k] for k in SR.STATS])
        put_state(tag + ".s2", s)
        put_path(tag + ".p2", s)
        rec[tag + ".counters2"] = np.array([s.half, s.status["ext_counter"]])
        h0 = s.half
        s.search(1e9, H2)
        st = s.status
        put_state(tag + ".s3", s)
        rec[tag + ".counters3"] = np.array([s.half - h0, st["n_shared"], st["stat_rewires"], s.half,
                                            st["ext_counter"]])
        s.end()
    T2 = engine.Terrain.from_data(data, storage=L.STORAGE_F64)
    Ls, Ms = planner.ReplanSession(T), planner.ReplanSession(T2)
    refused = 0
    for bad in ((LIMIT, LIMIT + 1), (LIMIT, 0)):
        try:
            Ls.tree_limit = bad
        except ValueError:
            refused += 1
    rec["L.refused"] = np.array([int(refused == 2), Ls.tree_limit[0]])
    Ls.tree_limit = (LIMIT, TRIM_TO)
    Ls.begin(start, goal, **kw)
    Ms.begin(start, goal, **kw)
    sizes_l, sizes_m, trims_m = [], [], 0
    for _ in range(CALLS):
        Ls.search(1e9, 2)
        Ms.search(1e9, 2)
        if max(Ms.known) > LIMIT:
            Ms.trim(TRIM_TO)
            trims_m += 1
        sizes_l += list(Ls.known)
        sizes_m += list(Ms.known)
    put_state("L", Ls)
    put_state("M", Ms)
    put_path("L.path", Ls)
    put_path("M.path", Ms)
    rec["L.sizes"], rec["M.sizes"] = np.array(sizes_l), np.array(sizes_m)
    rec["L.counters"] = np.array([Ls.trims_by_search, Ls.half, Ls.status["ext_counter"]])
    rec["M.counters"] = np.array([trims_m, Ms.half, Ms.status["ext_counter"]])
    return rec


@pytest.fixture(scope="module", params=["cpp", "python"])
def scenario(request, gpu, tmp_path_factory):
    if request.param == "python":
        return py_scenario()
    from tests.test_abi import build_node_callsite
    d = tmp_path_factory.mktemp("replan_trim")
    exe = build_node_callsite(d / "replan_trim_node", src="replan_trim_node.cpp")
    data, _ = R.terrain(None)
    start, goal = R.start_goal()
    nx, ny = data.z.shape
    slopes = data.dx is not None
    with open(d / "input.bin", "wb") as f:
        f.write(np.array([nx, ny, int(slopes)], np.int32).tobytes())
        for arr in (data.x, data.y, data.z) + ((data.dx, data.dy, data.dz) if slopes else ()):
            f.write(np.ascontiguousarray(arr, np.float64).tobytes())
        f.write(np.ascontiguousarray(np.r_[start, goal], np.float64).tobytes())
        f.write(np.array([BATCH, H, H2, CALLS, LIMIT, TRIM_TO, len(BUDGETS)], np.int32).tobytes())
        f.write(np.array(BUDGETS, np.int32).tobytes())
        f.write(np.array([SEED], np.uint64).tobytes())
    out = subprocess.run(["timeout", "-k", "10", "120", exe, str(d / "input.bin"), str(d / "output.bin")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return read_records(d / "output.bin")


@pytest.fixture(scope="module")
def ref():
    """The oracle's search and, per budget, the restatement's trim of it."""
    r1 = TR.session_search()
    return dict(r1=r1, met=TR.met_pairs(r1), trimmed={})


def trimmed(scenario, ref, B):
    """The restatement's session_trim of the oracle's trees under the session's
    own list (its order is the device's) and the oracle's best."""
    if B not in ref["trimmed"]:
        r1 = ref["r1"]
        pairs = list_of(scenario, f"t{B}.s1")[0]
        best = (r1["best_a"], r1["best_b"], r1["best_cost"])
        ref["trimmed"][B] = TR.session_trim(r1["a"], r1["b"], pairs, best, B)
    return ref["trimmed"][B]


# ---- 1: begin + search + trim = the restatement ----------------------------------------------------
@pytest.mark.parametrize("B", BUDGETS)
def test_trim_equals_the_restatement(scenario, ref, B):
    r1 = ref["r1"]
    for name in "ab":
        assert_same_tree(tree_of(scenario, f"t{B}.s1", name), r1[name], ("searched", name))
    pairs1, best1, cost1 = list_of(scenario, f"t{B}.s1")
    assert {tuple(p) for p in pairs1.tolist()} == ref["met"]
    assert best1 == (r1["best_a"], r1["best_b"]) and bits(cost1) == bits(r1["best_cost"])
    ta, tb, pairs, best, stats, shared = trimmed(scenario, ref, B)
    for name, t, st in zip("ab", (ta, tb), stats):
        got = [int(x) for x in scenario[f"t{B}.trim.{name}"]]
        assert got == [st[k] for k in TRIM_FIELDS], (name, got, st)
        assert bits(scenario[f"t{B}.trim.{name}.cut"][0]) == bits(st["cut"])
        assert_same_tree(tree_of(scenario, f"t{B}.s2", name), t, ("trimmed", name))
    assert [int(x) for x in scenario[f"t{B}.trim.shared"]] == [shared[k] for k in SR.STATS]
    assert_list(list_of(scenario, f"t{B}.s2"), pairs, best, "carried")
    assert list(scenario[f"t{B}.counters2"]) == [H, r1["ext_counter"]]
    if B == 0:
        assert [s["n_kept"] for s in stats] == [36, 40] and all(s["n_inherited"] == 0 for s in stats)
    if B == 24:
        assert all(s["n_over_budget"] > 0 for s in stats)
        assert stats[0]["n_kept"] <= 24 + 4 and stats[1]["n_kept"] <= 24 + 6


# ---- 2: the guarantee -------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BUDGETS)
def test_best_path_and_cost_are_bit_identical(scenario, B):
    f1, s1, a1, lyc1 = path_of(scenario, f"t{B}.p1")
    f2, s2, a2, lyc2 = path_of(scenario, f"t{B}.p2")
    assert f1 and f2 and len(s1) >= 3
    assert s1.shape == s2.shape and np.array_equal(bits(s1), bits(s2))
    assert a1.shape == a2.shape and np.array_equal(bits(a1), bits(a2))
    assert np.array_equal(bits(lyc1), bits(lyc2))
    c1, c2 = list_of(scenario, f"t{B}.s1")[2], list_of(scenario, f"t{B}.s2")[2]
    assert bits(c1) == bits(c2) == bits(lyc2[3])


# ---- 3: the search goes on ----------------------------------------------------------------------------
@pytest.mark.parametrize("B", BUDGETS)
def test_resumed_search_equals_the_oracles_continuation(scenario, ref, B):
    import oracle
    ta, tb, pairs, best, stats, shared = trimmed(scenario, ref, B)
    _, O = R.terrain(None)
    oracle.set_scan_mode(1)
    start, goal = R.start_goal()
    init = tuple({k: t[k] for k in ("v", "act", "parent")} for t in (ta, tb))
    r3 = O.plan(start, goal, init_trees=init, max_halves=H2, first_half=H,
                extend_base=ref["r1"]["ext_counter"], **TR.SESSION)
    for name in "ab":
        assert_same_tree(tree_of(scenario, f"t{B}.s3", name), r3[name], ("continued", name))
    pairs3, best3, cost3 = list_of(scenario, f"t{B}.s3")
    assert np.array_equal(pairs3[:len(pairs)], pairs)            # the carried ones, unchanged
    assert len(pairs3) == len(pairs) + r3["solutions"]           # carried + new
    halves, solutions, rewires, half, ext = (int(x) for x in scenario[f"t{B}.counters3"])
    assert (halves, solutions, half) == (H2, len(pairs3), H + H2)
    assert rewires == ref["r1"]["rewires"] + r3["rewires"] and ext == r3["ext_counter"]
    assert cost3 <= best[2]
    assert bits(cost3) == bits(SR.rank(pairs3, r3["a"]["g"], r3["b"]["g"])[2])
    print(f"budget {B}: continued from {len(ta['parent'])}+{len(tb['parent'])} vertices to "
          f"{len(r3['a']['parent'])}+{len(r3['b']['parent'])}, {len(pairs)} carried + {r3['solutions']} new "
          f"connections, best {best[2]!r} -> {cost3!r}")


# ---- 4: the limit inside search ------------------------------------------------------------------------
def test_tree_limit_equals_the_same_trims_from_outside(scenario):
    assert list(scenario["L.refused"]) == [1, 0]
    trims_l, half_l, ext_l = (int(x) for x in scenario["L.counters"])
    trims_m, half_m, ext_m = (int(x) for x in scenario["M.counters"])
    assert trims_l == trims_m and trims_l >= 2
    assert (half_l, ext_l) == (half_m, ext_m) and half_l == 2 * CALLS
    assert np.array_equal(scenario["L.sizes"], scenario["M.sizes"])
    sizes = scenario["L.sizes"].reshape(-1, 2)
    for name in "ab":
        assert_same_tree(tree_of(scenario, "L", name), tree_of(scenario, "M", name), ("limit", name))
    lm = list_of(scenario, "M")
    assert_list(list_of(scenario, "L"), lm[0], lm[1] + (lm[2],), "limit")
    for x, y in zip(path_of(scenario, "L.path"), path_of(scenario, "M.path")):
        assert np.array_equal(bits(np.asarray(x, np.float64)), bits(np.asarray(y, np.float64)))
    print(f"limit {LIMIT} -> {TRIM_TO}: {trims_l} trims in {CALLS} calls, sizes at the end {sizes[-1]}")
