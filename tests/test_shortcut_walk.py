"""postProcessPath's walk over a connect table (csrc/host/gbp_shortcut_walk.cpp)
and the shortcut entries' argument checks, without a device.

The walk is built into a stand-alone program (tests/native/shortcut_walk_probe.cpp)
with AddressSanitizer and UBSan and the engine's host flags (-ffp-contract=off);
its table is filled from the oracle's attemptConnect decisions and its output
must equal orc_post_process_path (rrt_connect.cpp:139-227) bit for bit: kept
states, kept actions, path_length_, path_yaw_, path_cost_.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from global_body_planner_amd import _lib
from tests import shortcut_cases as C
from tests.helpers import bits

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "global_body_planner_amd", "csrc", "host")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk")
    exe = str(d / "shortcut_walk_probe")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(ROOT, "include"), "-I", HOST, "-o", exe,
                    os.path.join(HERE, "native", "shortcut_walk_probe.cpp"),
                    os.path.join(HOST, "gbp_shortcut_walk.cpp"),
                    os.path.join(HOST, "gbp_host_check.cpp")], check=True)
    count = [0]

    def run(states, actions, table, add_yaw=0, lw=1.0, yw=1.0):
        n = len(states)
        assert len(actions) == n - 1 and len(table) == n * (n - 1) // 2
        count[0] += 1
        path = str(d / f"in{count[0]}.txt")
        with open(path, "w") as f:
            f.write(f"{n} {int(add_yaw)} {float(lw).hex()} {float(yw).hex()}\n")
            for v in np.asarray(states, np.float64).ravel():
                f.write(float(v).hex() + "\n")
            for v in np.asarray(actions, np.float64).ravel():
                f.write(float(v).hex() + "\n")
            f.write(" ".join(str(int(b)) for b in table) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        tok = r.stdout.split()
        m = int(tok[0])
        vals = np.array([float.fromhex(t) for t in tok[1:]])
        assert vals.size == 8 * m + 10 * (m - 1) + 3
        return (vals[:8 * m].reshape(m, 8), vals[8 * m:8 * m + 10 * (m - 1)].reshape(m - 1, 10),
                vals[-3], vals[-2], vals[-1])
    return run


def assert_walk_equal(got, want, label=""):
    gs, ga, gl, gy, gc = got
    ws, wa, wl, wy, wc = want
    assert gs.shape == ws.shape, (label, gs.shape, ws.shape)
    assert np.array_equal(bits(gs), bits(ws)), (label, "states")
    assert np.array_equal(bits(ga), bits(wa)), (label, "actions")
    assert bits(gl) == bits(wl) and bits(gy) == bits(wy) and bits(gc) == bits(wc), \
        (label, (gl, gy, gc), (wl, wy, wc))


# (terrain, batch, seed, adaptive): edges the oracle's walk keeps through the
# fallback branch; every other found path takes none
FALLBACK_EDGES = {
    ("slope-gridmap", 256, 7, False): 5, ("slope-gridmap", 256, 7, True): 9,
    ("slope-gridmap", 256, 2, False): 2, ("slope-gridmap", 256, 2, True): 5,
    ("synth-rough-256", 64, 5, False): 1, ("synth-rough-256", 1, 11, False): 2,
}


def test_walk_equals_oracle_on_found_paths(probe):
    fallbacks = []
    for case, batch, seed in C.FOUND:
        for adaptive in (False, True):
            S, A = C.found_path(case, batch, seed, adaptive)
            n = len(S)
            assert 4 <= n <= 31 and len({s.tobytes() for s in S}) == n
            want = C.oracle_walk(case[0], S, A, adaptive)
            got = probe(S, A, C.oracle_table(case[0], S, adaptive))
            assert_walk_equal(got, want, (case[0], batch, seed, adaptive))
            # the fallback branch keeps an original action (a[7] != 0 here) and
            # adds to path_cost_ only (rrt_connect.cpp:210-215); the counts are
            # the oracle's own walk's
            fb = C.fallback_edges(want[1])
            assert fb == FALLBACK_EDGES.get((case[0], batch, seed, adaptive), 0)
            assert (want[2] < want[4]) == (fb > 0)
            fallbacks.append(fb)
            print(f"{case[0]} batch {batch} seed {seed} adaptive {adaptive}: {n} -> "
                  f"{len(got[0])} states, {fb} fallback edges")
    assert any(f > 0 for f in fallbacks) and any(f == 0 for f in fallbacks)


def test_recorded_paths_are_the_oracles():
    """tests/golden/shortcut_paths.npz against the search run now, for the
    cases the oracle finishes in about a second (the synth ones and slope seed 7
    plain; the other slope searches take it 3 to 25 s each)."""
    for case, batch, seed in C.FOUND:
        for adaptive in (False, True):
            if case is C.SLOPE and (seed, adaptive) != (7, False):
                continue
            S, A = C.plan_path(case, batch, seed, adaptive)
            gs, ga = C.found_path(case, batch, seed, adaptive)
            assert np.array_equal(bits(S), bits(gs)) and np.array_equal(bits(A), bits(ga))


def test_walk_two_state_path(probe):
    """A path of one edge: kept through the connect when REACHED, through the
    fallback (its own action) when not."""
    S, A = C.found_path(C.SYNTH, 64, 11)
    for k in range(len(A)):
        s2, a2 = S[k:k + 2], A[k:k + 1]
        table = C.oracle_table(C.SYNTH[0], s2, False)
        want = C.oracle_walk(C.SYNTH[0], s2, a2, False)
        got = probe(s2, a2, table)
        assert_walk_equal(got, want, k)
        assert len(got[0]) == 2
        if not table[0]:
            assert np.array_equal(bits(got[1][0]), bits(a2[0])) and got[2] == 0 < got[4]


def test_walk_compares_states_by_value(probe):
    """A path that holds one state twice: the reference's `s != s_next` is a
    comparison of values, so the walk stops popping at the later copy."""
    S, A = C.found_path(C.SLOPE, 256, 7)
    k = len(S) // 2
    # ... S[k-1], S[k], S[k+1], S[k], S[k+1], ... : S[k] and S[k+1] twice
    s2 = np.concatenate([S[:k + 2], S[k:]])
    a2 = np.concatenate([A[:k + 1], A[k - 1:]])
    assert len(s2) == len(S) + 2 and len(a2) == len(s2) - 1
    want = C.oracle_walk(C.SLOPE[0], s2, a2, False)
    got = probe(s2, a2, C.oracle_table(C.SLOPE[0], s2, False))
    assert_walk_equal(got, want)
    assert len(got[0]) <= len(s2)


def test_walk_cost_weights(probe):
    """cost_add_yaw: path_cost_ is the per-edge weighted sum (gbp_planner.h
    weightedCost); with weights (1, 0) it is the oracle's plain cost again."""
    S, A = C.found_path(C.SLOPE, 256, 2)
    table = C.oracle_table(C.SLOPE[0], S, False)
    want = C.oracle_walk(C.SLOPE[0], S, A, False)
    assert_walk_equal(probe(S, A, table, add_yaw=1, lw=1.0, yw=0.0), want)
    got = probe(S, A, table, add_yaw=1, lw=0.0, yw=1.0)
    assert np.array_equal(bits(got[0]), bits(want[0])) and got[2] == want[2]
    assert got[4] >= got[3] > 0  # the yaw of every kept edge, the fallback edges' included


def test_shortcut_argument_validation_without_device():
    lib = _lib.load()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.create_string_buffer(4096)  # never read before the checks below fail the call
    H = ctypes.cast(h, ctypes.c_void_p)
    off = np.array([0, 3], np.int64)
    st, ac = np.zeros((3, 8)), np.zeros((2, 10))
    oo, os_, oa = np.zeros(2, np.int64), np.zeros((3, 8)), np.zeros((2, 10))
    l, y, c = np.zeros(1), np.zeros(1), np.zeros(1)
    rch, fl = np.zeros(3, np.uint8), np.zeros(3, np.uint32)

    def host(handle=H, n=1, off=off, st=st, ac=ac, oo=oo):
        return lib.gbp_shortcut_paths_host(handle, n, None if off is None else P(off),
                                           None if st is None else P(st),
                                           None if ac is None else P(ac), 0, 0, 1.0, 1.0,
                                           None if oo is None else P(oo), P(os_), P(oa), P(l), P(y),
                                           P(c), None)

    def dev(handle=H, n=1, off=off, st=st, rch=rch):
        return lib.gbp_shortcut_table_dev(handle, n, None if off is None else P(off),
                                          None if st is None else P(st), 0,
                                          None if rch is None else P(rch), P(fl), None)

    for f in (host, dev):
        assert f(handle=None) == -2                           # GBP_E_BAD_HANDLE
        assert f(n=-1) == -1                                  # GBP_E_INVALID_ARG
        assert f(off=np.array([0, 1], np.int64)) == -1        # a path of one state
        assert f(n=2, off=np.array([0, 3, 2], np.int64)) == -1  # non-monotone
        assert f(off=np.array([1, 4], np.int64)) == -1        # does not start at 0
        assert f(off=None) == -1
        assert f(st=None) == -1
        assert f(n=0, off=None, st=None) == 0                 # nothing to do
    assert host(ac=None) == -1 and host(oo=None) == -1
    assert dev(rch=None) == -1
    import torch
    if not torch.cuda.is_available():
        assert host() == -6 and dev() == -6                   # GBP_E_NO_DEVICE
