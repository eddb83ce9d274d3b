"""The path join of two half trees (csrc/host/gbp_tree_path.cpp), without a device.

The join is built into a stand-alone program (tests/native/tree_path_probe.cpp)
with AddressSanitizer and UBSan and the host planner's flags
(-ffp-contract=off), from the join's own sources only: it links no engine.
Hand-made trees pin the order of the joined path (rrt_connect.cpp:386-401:
Ta's root -> ia, then Tb's ib -> root without ib, Tb's actions reversed); the
oracle's searches pin states, actions, length and yaw bit for bit.
"""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import shortcut_cases as C
from tests.helpers import bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "global_body_planner_amd", "csrc", "host")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("join")
    exe = str(d / "tree_path_probe")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe,
                    os.path.join(HERE, "native", "tree_path_probe.cpp"),
                    os.path.join(HOST, "gbp_tree_path.cpp"),
                    os.path.join(HOST, "gbp_planning_math.cpp")], check=True)
    count = [0]

    def run(ta, tb, ia, ib):
        """ta / tb: dicts of v [n][8], act [n][10], parent [n], g [n] ->
        (states, actions, length, yaw, duration)."""
        count[0] += 1
        path = str(d / f"in{count[0]}.txt")
        with open(path, "w") as f:
            f.write(f"{len(ta['parent'])} {len(tb['parent'])} {int(ia)} {int(ib)}\n")
            for t in (ta, tb):
                n = len(t["parent"])
                assert np.shape(t["v"]) == (n, 8) and np.shape(t["act"]) == (n, 10) and len(t["g"]) == n
                for key in ("v", "act"):
                    for x in np.asarray(t[key], np.float64).ravel():
                        f.write(float(x).hex() + "\n")
                f.write(" ".join(str(int(p)) for p in t["parent"]) + "\n")
                for x in np.asarray(t["g"], np.float64).ravel():
                    f.write(float(x).hex() + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        tok = r.stdout.split()
        m = int(tok[0])
        vals = np.array([float.fromhex(t) for t in tok[1:]])
        assert vals.size == 8 * m + 10 * (m - 1) + 3
        return (vals[:8 * m].reshape(m, 8), vals[8 * m:8 * m + 10 * (m - 1)].reshape(m - 1, 10),
                vals[-3], vals[-2], vals[-1])
    return run


def same(x, y):
    return np.array_equal(bits(x), bits(y))


# ---- hand-made trees ---------------------------------------------------------
Q, H = math.atan2(1.0, 1.0), math.atan2(1.0, 0.0)  # the yaws of velocities (1, 1) and (0, 1)


def state(x, y, vx, vy):
    return [x, y, 0.3, vx, vy, 0.0, 0.0, 0.0]


def action(tag, t_s, t_f):
    return [tag, 0, 0, 0, 0, 0, t_s, t_f, 0, 0]


def duration(actions):
    d = 0.0
    for a in actions:
        d += a[6] + a[7]
    return d


def tree(rows):
    """rows of (state, action, parent, g)."""
    return dict(v=np.array([r[0] for r in rows], float), act=np.array([r[1] for r in rows], float),
                parent=np.array([r[2] for r in rows], np.int32), g=np.array([r[3] for r in rows], float))


A0, A1 = state(0, 0, 1, 0), state(1, 0, 1, 1)      # yaw 0 -> Q
B0, B1 = state(5, 0, 1, 0), state(4, 0, 1, 1)      # yaw 0 -> Q
ROOT_ACTION = action(-1, 9.0, 9.0)                 # a root's action is never on a path
TA2 = tree([(A0, ROOT_ACTION, -1, 0.0), (A1, action(11, 0.3, 0.125), 0, 1.25)])
TB2 = tree([(B0, ROOT_ACTION, -1, 0.0), (B1, action(21, 0.25, 0.0), 0, 2.5)])


def test_smallest_tree_pair(probe):
    """Two trees of two vertices, joined at their leaves: [a0, a1, b0] and
    [A.a[1], B.a[1]].  Tb's joined vertex b1 is dropped, its action kept."""
    S, A, length, yaw, dur = probe(TA2, TB2, 1, 1)
    assert same(S, [A0, A1, B0])
    assert same(A, [TA2["act"][1], TB2["act"][1]])
    assert length == 1.25 + 2.5
    assert bits(yaw) == bits((0.0 + (Q - 0.0)) + (0.0 + (Q - 0.0)))
    assert bits(dur) == bits(duration(A)) and dur == (0.3 + 0.125) + (0.25 + 0.0)


def test_joined_at_the_roots(probe):
    """ia = ib = 0: Ta's root alone (Tb's root is the dropped vertex), no action."""
    S, A, length, yaw, dur = probe(TA2, TB2, 0, 0)
    assert same(S, [A0]) and A.shape == (0, 10) and (length, yaw, dur) == (0.0, 0.0, 0.0)


def test_deeper_on_one_side(probe):
    """One tree three vertices deep, with a branch beside the path so that the
    path's vertices are not the tree's first ones."""
    a2, a3 = state(9, 9, 1, 0), state(2, 1, 0, 1)  # a2: a branch off the root; a3 (yaw H) under a1
    ta = tree([(A0, ROOT_ACTION, -1, 0.0), (A1, action(11, 0.3, 0.125), 0, 1.25),
               (a2, action(12, 0.3, 0.5), 0, 7.0), (a3, action(13, 0.3, 0.25), 1, 2.75)])
    S, A, length, yaw, dur = probe(ta, TB2, 3, 1)
    assert same(S, [A0, A1, a3, B0])
    assert same(A, [ta["act"][1], ta["act"][3], TB2["act"][1]])
    assert length == 2.75 + 2.5
    assert bits(yaw) == bits(((0.0 + (Q - 0.0)) + (H - Q)) + (0.0 + (Q - 0.0)))
    assert bits(dur) == bits(duration(A))
    # the same depth on Tb's side only: its chain is walked leaf -> root
    b2, b3 = state(9, -9, 1, 0), state(3, 1, 0, 1)
    tb = tree([(B0, ROOT_ACTION, -1, 0.0), (B1, action(21, 0.25, 0.0), 0, 2.5),
               (b2, action(22, 0.3, 0.5), 0, 7.0), (b3, action(23, 0.3, 0.375), 1, 4.0)])
    S, A, length, yaw, dur = probe(TA2, tb, 1, 3)
    assert same(S, [A0, A1, B1, B0])
    assert same(A, [TA2["act"][1], tb["act"][3], tb["act"][1]])
    assert length == 1.25 + 4.0
    assert bits(yaw) == bits((0.0 + (Q - 0.0)) + ((0.0 + (Q - 0.0)) + (H - Q)))
    assert bits(dur) == bits(duration(A))


# ---- the oracle's searches on the config-2 pair ------------------------------
@functools.lru_cache(maxsize=None)
def oracle_plan(**kw):
    _, O = C.terrain(C.SYNTH[0])
    oracle.set_scan_mode(1)
    start, goal = C.start_goal(O, *C.SYNTH[1])
    return start, goal, O.plan(start, goal, **kw)


@pytest.mark.parametrize("batch,seed", [(64, 11), (1, 11), (64, 5)])
def test_join_equals_oracle_search(probe, batch, seed):
    _, _, r = oracle_plan(batch=batch, seed=seed)
    assert r["found"]
    ia, ib = r["meet_a"], r["meet_b"]
    # the trees meet at two different states, so dropping the wrong end shows
    assert not same(r["a"]["v"][ia], r["b"]["v"][ib])
    S, A, length, yaw, dur = probe(r["a"], r["b"], ia, ib)
    assert S.shape == r["states"].shape and same(S, r["states"])
    assert same(A, r["actions"])
    assert bits(length) == bits(r["path_length"])
    assert bits(yaw) == bits(r["path_yaw"])
    assert bits(dur) == bits(duration(r["actions"]))
    print(f"batch {batch} seed {seed}: {len(r['a']['parent'])} + {len(r['b']['parent'])} vertices, "
          f"path of {len(S)} states, length {length!r} yaw {yaw!r}")


def test_join_of_rewired_trees(probe):
    """RRT*'s trees: rewiring leaves parents with a larger index than their
    child, and g / y are the rewired chains' sums."""
    start, goal, r = oracle_plan(star=True, batch=1024, seed=3, max_halves=300, stream_a=401,
                                 stream_b=402)
    a, b, ia, ib = r["a"], r["b"], r["best_a"], r["best_b"]
    later = [int(np.count_nonzero(t["parent"] > np.arange(len(t["parent"])))) for t in (a, b)]
    assert r["rewires"] == 25 and later == [4, 19]
    assert ia >= 0 and ib >= 0
    S, A, length, yaw, dur = probe(a, b, ia, ib)
    assert bits(length) == bits(r["best_cost"])
    assert same(S[0], start) and same(S[-1], goal) and len(A) == len(S) - 1
    assert bits(yaw) == bits(a["y"][ia] + b["y"][ib])
    assert bits(dur) == bits(duration(A))
