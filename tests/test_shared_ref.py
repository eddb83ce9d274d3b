"""tests/shared_ref.py on its own, without a device: the remap of a pair list
and the ranking on hand-made lists, and the numpy join against joinTreePaths
itself (csrc/host/gbp_tree_path.cpp) through the stand-alone sanitizer build of
tests/native/tree_path_probe.cpp, as tests/test_tree_path.py runs it.  Also
pathFromRows (the session's yaw and duration over rows the device gathered)
against joinTreePaths, in a stand-alone sanitizer build of its own
(tests/native/path_rows_probe.cpp)."""
import numpy as np
import pytest

from tests import shared_ref as SR
from tests.helpers import bits
from tests.test_tree_path import probe  # noqa: F401  (the fixture: builds and runs the probe)


def test_remap_keeps_order_and_counts_each_loss_once():
    pairs = [[0, 0], [1, 2], [2, 1], [3, 3], [1, 2], [2, 2]]
    ra = np.array([0, 1, -1, 2], np.int32)      # a's vertex 2 is gone
    rb = np.array([0, -1, 1, -1], np.int32)     # b's vertices 1 and 3 are gone
    out, st = SR.remap_pairs(pairs, ra, rb)
    assert out.tolist() == [[0, 0], [1, 1], [1, 1]] and out.dtype == np.int32
    # (2, 1) is lost on both sides: counted under a; (2, 2) under a; (3, 3) under b
    assert st == dict(n_before=6, n_kept=3, n_dropped_a=2, n_dropped_b=1, error=0)
    out, st = SR.remap_pairs(pairs, None, rb)
    assert out.tolist() == [[0, 0], [1, 1], [1, 1], [2, 1]] and st["n_dropped_b"] == 2
    out, st = SR.remap_pairs(pairs, None, None)
    assert out.tolist() == pairs and st["n_kept"] == 6
    out, st = SR.remap_pairs(np.empty((0, 2), np.int32), ra, rb)
    assert out.shape == (0, 2) and st["n_before"] == 0


def test_rank_is_strict_and_skips_nan():
    ga = np.array([0.0, 1.0, 2.0, np.nan])
    gb = np.array([0.5, 1.5, 0.5])
    assert SR.rank([], ga, gb) == (-1, -1, np.inf)
    assert SR.rank([[3, 0]], ga, gb) == (-1, -1, np.inf)                  # NaN alone: none
    assert SR.rank([[2, 0], [1, 1], [3, 0], [1, 1]], ga, gb) == (2, 0, 2.5)  # ties: the earliest
    assert SR.rank([[1, 1], [2, 0]], ga, gb) == (1, 1, 2.5)
    assert SR.rank([[2, 1], [0, 2], [0, 0]], ga, gb) == (0, 2, 0.5)


def test_small_trees_have_exact_equal_costs():
    A, B = SR.small_tree(11), SR.small_tree(12)
    for t in (A, B):
        assert np.all(t["g"] * 4 == np.round(t["g"] * 4)) and t["g"][0] == 0 and np.all(t["g"][1:] > 0)
        assert np.all(t["parent"][1:] < np.arange(1, 300))
    cost = A["g"][:, None] + B["g"][None, :]
    assert np.count_nonzero(cost == cost[1, 1]) > 2       # pairs of exactly equal cost exist


@pytest.mark.parametrize("ia,ib", [(299, 298), (0, 298), (299, 0), (0, 0), (17, 170)])
def test_join_equals_the_host_join(probe, ia, ib):  # noqa: F811
    A, B = SR.small_tree(11), SR.small_tree(12)
    s, a, length, na, nb = SR.join(A, ia, B, ib)
    if (ia, ib) == (0, 0):   # the probe refuses nothing here, but prints no action
        assert s.shape == (1, 8) and a.shape == (0, 10) and (na, nb) == (1, 0)
    S, Ac, plen, _, _ = probe(A, B, ia, ib)
    assert S.shape == s.shape and np.array_equal(bits(S), bits(s))
    assert Ac.shape == a.shape and np.array_equal(bits(Ac), bits(a))
    assert bits(plen) == bits(length) and na + nb == len(s)


def test_join_of_a_chain_against_the_index_order(probe):  # noqa: F811
    A, B = SR.chain_against_the_index_order(40), SR.chain_against_the_index_order(33)
    s, a, length, na, nb = SR.join(A, 1, B, 1)
    assert (na, nb) == (40, 32)
    S, Ac, plen, _, _ = probe(A, B, 1, 1)
    assert np.array_equal(bits(S), bits(s)) and np.array_equal(bits(Ac), bits(a))
    assert bits(plen) == bits(length)


# ---- pathFromRows (csrc/host/gbp_tree_path.cpp): the session's yaw and duration ---------------
@pytest.fixture(scope="module")
def rows_probe(tmp_path_factory):
    """tests/native/path_rows_probe.cpp, stand-alone with AddressSanitizer and
    UBSan and the host planner's flags, from the join's own sources only."""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    host = os.path.join(root, "global_body_planner_amd", "csrc", "host")
    d = tmp_path_factory.mktemp("rows")
    exe = str(d / "path_rows_probe")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(root, "include"), "-I", host, "-o", exe,
                    os.path.join(here, "native", "path_rows_probe.cpp"),
                    os.path.join(host, "gbp_tree_path.cpp"),
                    os.path.join(host, "gbp_planning_math.cpp")], check=True)
    count = [0]

    def run(ta, tb, ia, ib):
        count[0] += 1
        path = str(d / f"in{count[0]}.txt")
        with open(path, "w") as f:
            f.write(f"{len(ta['parent'])} {len(tb['parent'])} {int(ia)} {int(ib)}\n")
            for t in (ta, tb):
                for key in ("v", "act"):
                    for x in np.asarray(t[key], np.float64).ravel():
                        f.write(float(x).hex() + "\n")
                f.write(" ".join(str(int(p)) for p in t["parent"]) + "\n")
                for x in np.asarray(t["g"], np.float64).ravel():
                    f.write(float(x).hex() + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
        return r.stdout.split()
    return run


@pytest.mark.parametrize("ia,ib", [(299, 298), (0, 298), (299, 0), (0, 0), (17, 170)])
def test_path_from_rows_equals_the_join(rows_probe, ia, ib):
    A, B = SR.small_tree(11), SR.small_tree(12)
    _, _, _, na, nb = SR.join(A, ia, B, ib)
    assert rows_probe(A, B, ia, ib) == ["ok", str(na + nb), str(na)]


def test_path_from_rows_on_a_deep_chain(rows_probe):
    A, B = SR.chain_against_the_index_order(40), SR.chain_against_the_index_order(33)
    assert rows_probe(A, B, 1, 1) == ["ok", "72", "40"]
