"""RRTClass::set_informed_cost (include/gbp_planner.h) through a C++ node
(tests/integration/informed_plan_node.cpp, built against the drop-in as the
other node tests are): on the session pair of synth-rough-256, batch 512,
seed 5, informed cost 4.0 (as test_device_loop_with_direction_sampling_equals_
host_batched compares the two planners),

  * the host-batched search (targets from gbp_sample_states_informed_host) and
    the device-resident one (k_targets_informed) return the same path, trees and
    counters, bit for bit;
  * their `targets` count differs from a plain run's;
  * the device run's path passes the oracle's pair checks;
  * the handle's own ellipse (off) is back after the runs.
"""
import subprocess

import numpy as np
import pytest

import oracle
from global_body_planner_amd import terrain_data as td
from tests import informed_ref as R
from tests.test_gpu_planner import _start_goal, check_path

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BATCH, SEED, COST = 512, 5, 4.0


def read_runs(path):
    buf = open(path, "rb").read()
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(buf, dtype, n, pos)
        pos += a.nbytes
        return a
    runs = []
    for _ in range(3):
        head = take(np.int64, 9)
        r = dict(zip(("found", "targets", "extends", "attempts_checked", "connects", "vertices_a",
                      "vertices_b"), (int(v) for v in head[:7])))
        r["states"] = take(np.float64, 8 * int(head[7])).reshape(-1, 8)
        r["actions"] = take(np.float64, 10 * int(head[8])).reshape(-1, 10)
        r["trees"] = []
        for _k in range(2):
            nv = int(take(np.int64, 1)[0])
            r["trees"].append((take(np.uint64, 8 * nv), take(np.uint64, 10 * nv), take(np.uint64, nv),
                               take(np.int32, nv)))
        runs.append(r)
    active = int(take(np.int64, 1)[0])
    assert pos == len(buf)
    return runs, active


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    from tests.test_abi import build_node_callsite
    d = tmp_path_factory.mktemp("informed_plan")
    exe = build_node_callsite(d / "informed_plan_node", src="informed_plan_node.cpp")
    data = td.by_name("synth-rough-256")
    O = oracle.OracleTerrain.from_data(data)
    start, goal = _start_goal(O, *R.SESSION_START, *R.SESSION_GOAL)
    nx, ny = data.z.shape
    slopes = data.dx is not None
    with open(d / "input.bin", "wb") as f:
        f.write(np.array([nx, ny, int(slopes)], np.int32).tobytes())
        for arr in (data.x, data.y, data.z) + ((data.dx, data.dy, data.dz) if slopes else ()):
            f.write(np.ascontiguousarray(arr, np.float64).tobytes())
        f.write(np.ascontiguousarray(np.r_[start, goal], np.float64).tobytes())
        f.write(np.array([BATCH], np.int32).tobytes())
        f.write(np.array([SEED], np.uint64).tobytes())
        f.write(np.array([COST], np.float64).tobytes())
    out = subprocess.run(["timeout", "-k", "10", "120", exe, str(d / "input.bin"),
                          str(d / "output.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    r, active = read_runs(d / "output.bin")
    return dict(host=r[0], dev=r[1], plain=r[2], active=active, O=O, start=start, goal=goal)


def test_device_loop_with_informed_cost_equals_host_batched(runs):
    host, dev = runs["host"], runs["dev"]
    assert host["found"] == 1 and dev["found"] == 1
    # (the node does not record the planner's own duration figure: the sum stands in for it)
    dur = float(np.sum(dev["actions"][:, 6] + dev["actions"][:, 7]))
    check_path(runs["O"], dict(dev, path_duration=dur), runs["start"], runs["goal"])
    assert np.array_equal(dev["states"].view(np.uint64), host["states"].view(np.uint64))
    assert np.array_equal(dev["actions"].view(np.uint64), host["actions"].view(np.uint64))
    for k in ("vertices_a", "vertices_b", "targets", "extends", "attempts_checked", "connects"):
        assert dev[k] == host[k], (k, dev[k], host[k])
    for th, tdv in zip(host["trees"], dev["trees"]):
        assert len(th[3]) > 1
        for a, b in zip(th, tdv):
            assert np.array_equal(a, b)
    print(f"informed: {dev['vertices_a']}+{dev['vertices_b']} vertices, {dev['targets']} targets; "
          f"plain: {runs['plain']['vertices_a']}+{runs['plain']['vertices_b']} vertices, "
          f"{runs['plain']['targets']} targets")


def test_informed_cost_changes_the_targets(runs):
    assert runs["plain"]["found"] == 1
    assert runs["plain"]["targets"] != runs["host"]["targets"]


def test_handle_keeps_its_own_setting(runs):
    assert runs["active"] == 0
