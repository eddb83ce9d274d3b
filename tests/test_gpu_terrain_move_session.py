"""A ReplanSession carried across a moved terrain window (moveFromGridMap /
engine.Terrain.move, then mapChanged / map_changed), on the C++ class and the
Python class.

The map is synth-rough-256 with box 1 of tests/prune_ref.py, rounded to float
(a grid_map layer is float), as the window at (0, 0) of the same map of 384
cells a side.  begin + search(200 halves of the device RRT*), the window moved
by SHIFT, mapChanged, 100 more halves: every tree equals the oracle's, bit for
bit, and the terrain handle is the same one throughout.

SHIFT was chosen on the CPU with the oracle alone so that both roots stay
inside the window, each tree loses at least one vertex to the window's edge
and each keeps at least half; test_the_shift_meets_its_conditions states that.
The new positions are recomputed from the new origin (origin + i * res, what
grid_map does), not displaced copies of the old ones.
"""
import dataclasses
import functools
import subprocess

import numpy as np
import pytest

import oracle
from global_body_planner_amd import _lib as L
from global_body_planner_amd import terrain_data as td
from tests import prune_ref as R
from tests.test_gpu_replan_session import read_records, tree_of
from tests.test_gpu_tree_prune import assert_same_tree

pytestmark = pytest.mark.gpu

N, BIG, RES = 256, 384, 0.02
SHIFT = (30, 60)
BATCH, SEED, H, H2 = 1024, 11, 200, 100
STAR = dict(star=True, stream_a=401, stream_b=402, batch=BATCH, seed=SEED, nthreads=16)


@functools.lru_cache(maxsize=None)
def big_map():
    big = td.synth_rough(BIG)
    dz, x0, x1, y0, y1 = R.BOXES["box1"]
    z = np.array(big.z, np.float64)
    z[np.ix_((big.x >= x0) & (big.x <= x1), (big.y >= y0) & (big.y <= y1))] += dz
    return dataclasses.replace(big, z=z.astype(np.float32).astype(np.float64))


def window(ox, oy):
    """(x, y, z, dx, dy, dz) of the window at cell (ox, oy): positions from the
    window's origin, origin + i * res."""
    big = big_map()
    c = lambda a: np.ascontiguousarray(a[ox:ox + N, oy:oy + N])
    x = ox * RES + np.arange(N, dtype=np.float64) * RES
    y = oy * RES + np.arange(N, dtype=np.float64) * RES
    return (x, y, c(big.z), c(big.dx), c(big.dy), c(big.dz))


@pytest.fixture(scope="module")
def ref():
    """The oracle's side of every step."""
    oracle.set_scan_mode(1)
    start, goal = R.start_goal()
    w0, w1 = window(0, 0), window(*SHIFT)
    O0, O1 = oracle.OracleTerrain(*w0), oracle.OracleTerrain(*w1)
    r1 = O0.plan(start, goal, max_halves=H, **STAR)
    pruned = [R.prune(r1[n], R.edge_valid(O1, r1[n], d)) for n, d in (("a", 0), ("b", 1))]
    init = tuple({k: p[0][k] for k in ("v", "act", "parent")} for p in pruned)
    r3 = O1.plan(start, goal, init_trees=init, max_halves=H2, first_half=H,
                 extend_base=r1["ext_counter"], **STAR)
    oracle.set_scan_mode(0)
    return dict(r1=r1, pruned=pruned, r3=r3, start=start, goal=goal, w0=w0, w1=w1)


def py_scenario():
    from global_body_planner_amd import engine, planner
    start, goal = R.start_goal()
    rec = {}

    def put_trees(tag, trees):
        for name, t in zip("ab", trees):
            rec[f"{tag}.{name}.v"], rec[f"{tag}.{name}.act"] = t["v"].ravel(), t["act"].ravel()
            rec[f"{tag}.{name}.parent"], rec[f"{tag}.{name}.g"] = t["parent"], t["g"]

    w0, w1 = window(0, 0), window(*SHIFT)
    T = engine.Terrain(*w0)
    h0 = T._h.value
    s = planner.ReplanSession(T).begin(start, goal, batch=BATCH, seed=SEED)
    s.search(1e9, H)
    put_trees("s1", s.dump())
    rec["s1.counters"] = np.array([H, s.half, s.status["ext_counter"]])
    T.move(SHIFT[0], SHIFT[1], *w1)
    rec["move"] = np.array([1, int(T._h.value == h0)])
    rec["move.x"], rec["move.y"] = w1[0], w1[1]
    pruned, _ = s.map_changed()
    for name, ps in zip("ab", pruned):
        rec[f"s2.prune.{name}"] = np.array([ps[k] for k in ("n_before", "n_kept", "n_edge_invalid",
                                                            "n_inherited")])
    put_trees("s2", s.dump())
    h = s.half
    s.search(1e9, H2)
    put_trees("s3", s.dump())
    rec["s3.counters"] = np.array([s.half - h, s.half, s.status["ext_counter"], int(T._h.value == h0)])
    s.end()
    return rec


@pytest.fixture(scope="module", params=["cpp", "python"])
def scenario(request, gpu, tmp_path_factory):
    if request.param == "python":
        return py_scenario()
    from tests.test_abi import build_node_callsite
    d = tmp_path_factory.mktemp("move")
    exe = build_node_callsite(d / "terrain_move_node", src="terrain_move_node.cpp")
    start, goal = R.start_goal()
    with open(d / "input.bin", "wb") as f:
        f.write(np.array([N, N], np.int32).tobytes())
        f.write(np.array([RES], np.float64).tobytes())
        for off in ((0, 0), SHIFT):
            f.write(np.array([off[0] * RES, off[1] * RES], np.float64).tobytes())
            for arr in window(*off)[2:]:
                f.write(np.ascontiguousarray(arr, np.float64).tobytes())
        f.write(np.ascontiguousarray(np.r_[start, goal], np.float64).tobytes())
        f.write(np.array([BATCH, H, H2], np.int32).tobytes())
        f.write(np.array([SEED], np.uint64).tobytes())
    out = subprocess.run(["timeout", "-k", "10", "120", exe, str(d / "input.bin"), str(d / "output.bin")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rec = read_records(d / "output.bin")
    # a third of a cell and another size reload (false); then in place again
    assert list(rec["reload"]) == [0, 0, N + 1, 1]
    assert list(rec["again"]) == [1, 1, 1]
    return rec


def test_the_shift_meets_its_conditions(ref):
    """On the CPU, from the oracle alone."""
    x, y = ref["w1"][:2]
    for root in (ref["start"], ref["goal"]):
        assert x[0] < root[0] < x[-1] and y[0] < root[1] < y[-1]
    for (tree, remap, st), name in zip(ref["pruned"], "ab"):
        print(f"tree {name}: {st['n_kept']} of {st['n_before']} vertices kept")
        assert st["n_kept"] <= st["n_before"] - 1 and 2 * st["n_kept"] >= st["n_before"]
    # the new positions are not the displaced old ones bit for bit everywhere
    old = ref["w0"][0]
    assert np.any(ref["w1"][0][:N - SHIFT[0]] != old[SHIFT[0]:])


def test_begin_and_search(scenario, ref):
    for name in "ab":
        assert_same_tree(tree_of(scenario, "s1", name), ref["r1"][name], ("s1", name))
    assert list(scenario["s1.counters"]) == [H, H, ref["r1"]["ext_counter"]]


def test_the_move_keeps_the_handle_and_the_prune_equals_the_restatement(scenario, ref):
    assert list(scenario["move"]) == [1, 1]
    assert np.array_equal(scenario["move.x"], ref["w1"][0]) and np.array_equal(scenario["move.y"], ref["w1"][1])
    for name, (t, remap, st) in zip("ab", ref["pruned"]):
        got = [int(v) for v in scenario[f"s2.prune.{name}"]]
        assert got == [st["n_before"], st["n_kept"], st["n_edge_invalid"], st["n_inherited"]], name
        assert_same_tree(tree_of(scenario, "s2", name), t, ("pruned", name))


def test_the_search_goes_on_in_the_new_window(scenario, ref):
    r3 = ref["r3"]
    for name in "ab":
        got = tree_of(scenario, "s3", name)
        assert len(got["parent"]) > len(ref["pruned"]["ab".index(name)][0]["parent"])
        assert_same_tree(got, r3[name], ("continued", name))
    halves, half, ext, same = (int(v) for v in scenario["s3.counters"])
    assert (halves, half, ext, same) == (H2, H + H2, r3["ext_counter"], 1)
