"""The inputs of the scale tests (tests/scale_cases.py), without a device: that
they cross the grid caps they are meant to cross, that the tiled edge decisions
are the oracle's, that the key-range tree makes every round of the trim's radix
select choose, that a window's table is the dense path's sub-block, and that
the numpy restatements stay quick at 70,031 vertices.
"""
import time

import numpy as np
import pytest

from tests import graft_ref as G
from tests import prune_ref as R
from tests import reroot_ref as RR
from tests import scale_cases as X
from tests import shared_ref as SR
from tests import shortcut_cases as C
from tests import trim_ref as TR
from tests.helpers import bits


# ---- the sizes against the caps -------------------------------------------------------------
def test_sizes_cross_the_caps():
    n = X.N_BIG
    assert n == 70031 == len(X.big_tree()[0]["parent"])
    # k_prune_gather strides over (n - 1) x 9 pieces, k_prune_move_rows over n x 9
    for cap in (X.CAP_GATHER, X.CAP_MOVE_ROWS):
        assert n - 1 > cap * X.TB / X.PRUNE_PIECES
    assert X.CAP_MOVE_ROWS * X.TB // X.PRUNE_PIECES == 58254
    # k_trim_hist strides over the n - 1 non-root vertices: three turns, the last one short
    per_turn = X.TRIM_HIST_GRID * X.TB
    assert per_turn == 32768 and n - 1 > per_turn + 1
    assert (n - 1) // per_turn == 2 and (n - 1) % per_turn % 64 != 0   # lanes past n in the last wave
    assert sorted(X.BIG_BUDGETS) == [1, per_turn + 1, 40000, n - 1]
    # the batched entries
    bn = X.batch_n(X.CUS)
    assert bn == 1048869 and bn > 16 * X.CUS * 256 > 4096 * 256 - 1 and bn > 2 * 8 * X.CUS * 256
    assert bn % 256 != 0 and bn > 4 * X.CHUNK
    assert 6 * 174762 <= 16 * X.CUS * 256 < 6 * 174763 <= 6 * X.N_EXTEND_PREP
    assert X.N_EXTEND_PREP < 16 * X.CUS * 256       # k_extend_select's one turn: the cap is k_extend_prep's
    for count in X.WINDOW_CALLS:
        assert count > 64                            # SC_MAXP paths per shortcut launch
    assert X.WINDOW_CALLS[1] == 2 * 64 and X.WINDOW_CALLS[2] == X.N_WINDOWS


# ---- the big tree -------------------------------------------------------------------------------
@pytest.mark.parametrize("permute", [False, True])
def test_big_tree_edge_decisions_are_the_oracles(permute):
    tree, rb, cost = X.big_tree(permute)
    ok = X.big_edge_valid(permute)
    n = X.N_BIG
    assert len(ok) == n and ok[0] == 1
    if permute:
        assert np.any(tree["parent"] > np.arange(n))
        plain = X.big_tree(False)[0]
        new = X.renumbering(n, X.PERMUTE_SEED)
        assert np.array_equal(bits(tree["v"][new]), bits(plain["v"]))
    idx = X.sample_of(n, 7)
    idx = idx[idx > 0]
    assert 2000 <= len(idx) <= 2600
    _, O = R.terrain("box1")
    got = O.validate_pairs(tree["v"][tree["parent"][idx]], tree["act"][idx], R.FORWARD, nthreads=8)[0]
    assert np.array_equal(got, ok[idx])
    assert 0.1 < 1.0 - ok.mean() < 0.5
    ref = R.prune(tree, ok)
    assert 0 < ref[2]["n_kept"] < n and ref[2]["n_inherited"] > 0
    assert np.any(np.diff(np.flatnonzero(ref[1] < 0)) > 1)     # not one contiguous run
    # g as a load derives it is the oracle's own
    assert np.array_equal(bits(SR.pose_g(tree["v"], tree["parent"])), bits(tree["g"]))


@pytest.mark.parametrize("permute", [False, True])
def test_big_tree_budgets_and_ties(permute):
    tree, rb, cost = X.big_tree(permute)
    n = X.N_BIG
    f = TR.f_values(tree, rb)
    _, counts = np.unique(f[1:], return_counts=True)
    assert counts.min() >= X.COPIES                      # 745-way ties in f
    kept = {}
    for max_keep in X.BIG_BUDGETS:
        x = TR.trim(tree, rb, np.inf, max_keep, -1)
        kept[max_keep] = x[2]["n_kept"]
        assert x[2]["n_kept"] <= max_keep and (x[2]["n_kept"] - 1) % X.COPIES == 0
        assert x[2]["n_over_budget"] == n - x[2]["n_kept"] and np.isfinite(x[2]["cut"])
    assert kept[1] == 1 and kept[n - 1] == n - X.COPIES and kept[32769] < kept[40000]
    x = TR.trim(tree, rb, cost, 0, -1)
    assert x[2]["n_kept"] == 1 + 23 * X.COPIES
    # the bound between the two budgets' cuts, the smaller budget, the deepest leaf protected
    leaf = X.deepest(tree, f)
    assert X.depths(tree["parent"])[leaf] == len(SR.chain(tree["parent"], leaf)) - 1 >= 5
    bound = X.big_bound()
    x = TR.trim(tree, rb, bound, 32769, leaf)
    assert x[2]["n_over_bound"] > 0 and x[2]["n_over_budget"] > 0 and x[2]["n_protected"] > 0


# ---- the random recursive tree --------------------------------------------------------------------
def test_random_tree():
    tree, k, ok, attach, actions, size = X.random_tree()
    n = X.N_BIG
    assert len(tree["parent"]) == n and np.any(tree["parent"] > np.arange(n))
    assert 0.2 * n < size < 0.9 * n
    assert 0.015 < 1.0 - ok.mean() < 0.025 and 600 <= attach.sum() <= 800
    ref = RR.reroot(tree, k)
    assert ref[2]["n_kept"] == size and ref[2]["depth"] >= 15
    ref = RR.reroot(tree, k, ok)
    assert ref[2]["n_edge_invalid"] > 0 and ref[2]["n_inherited"] > 0 and 1 < ref[2]["n_kept"] < size
    ref = G.graft(tree, X.NEW_ROOT, attach, actions, ok)
    assert ref[2]["n_attached"] == attach.sum() and ref[2]["n_edge_invalid"] > 0
    assert 1000 < ref[2]["n_kept"] < n and ref[2]["depth"] > 2


# ---- the restatements stay quick ------------------------------------------------------------------
def test_restatements_take_seconds_at_this_size():
    tree, rb, cost = X.big_tree(True)
    rtree, k, ok, attach, actions, _ = X.random_tree()
    took = {}

    def timed(name, fn):
        t0 = time.perf_counter()
        fn()
        took[name] = time.perf_counter() - t0

    timed("TR.flags", lambda: TR.flags(tree, rb, cost, 40000, 5))
    timed("TR.trim", lambda: TR.trim(tree, rb, cost, 40000, 5))
    timed("R.prune", lambda: R.prune(tree, X.big_edge_valid(True)))
    timed("SR.pose_g", lambda: SR.pose_g(tree["v"], tree["parent"]))
    timed("RR.reroot", lambda: RR.reroot(rtree, k, ok))
    timed("G.graft", lambda: G.graft(rtree, X.NEW_ROOT, attach, actions, ok))
    timed("children", lambda: R.children(tree["parent"]))
    print({name: round(t, 2) for name, t in took.items()})
    assert max(took.values()) < 10.0, took


# ---- the key-range tree ---------------------------------------------------------------------------
def test_key_tree_values():
    """f = g + poseDistance is +0, any positive double from about 1e-162 up,
    +inf or NaN; a negative f is not reachable and not among the inputs."""
    tree, root, x = X.key_tree()
    f = X.key_f()
    n = len(f)
    assert 1400 <= n <= 1600 and np.all(tree["parent"][1:] == 0)
    assert not np.any(f < 0) and not np.any(np.signbit(f[f == 0]))
    finite = np.isfinite(x) & (np.abs(x) < 1e150)
    assert np.array_equal(bits(f[1:][finite]), bits(2.0 * np.abs(x[finite])))
    assert (f == 0).sum() == 9 and np.any(np.signbit(x[x == 0]))          # the root and eight zeros, two of them -0
    assert np.isnan(f).sum() == 40 and np.isinf(f).sum() == 72
    assert np.all(f[1:][np.abs(x) == 1e200] == np.inf)                    # the square overflowed
    mags = f[np.isfinite(f) & (f > 0) & ((f < 2.0) | (f > 2.02))]
    assert mags.min() < 1e-140 and mags.max() > 1e140
    for lo, hi in ((2.0, 2.0 + 2.0 ** -31), (2.0 + 2.0 ** -31, 2.0 + 2.0 ** -7)):
        run = f[(f >= lo) & (f < hi)]
        assert len(run) > 300 and len(np.unique(run)) < len(run)          # duplicates inside the run
        assert len(np.unique(bits(run) >> np.uint64(48))) == 1            # the high bytes shared
    assert len(np.unique(mags)) < len(mags)


def test_key_order_is_the_order_of_the_values():
    f = X.key_f()[1:]
    keys = X.trim_keys(f)
    order = np.argsort(keys, kind="stable")
    s, ks = f[order], keys[order]
    nan = np.isnan(s)
    first_nan = int(np.argmax(nan))
    assert nan[first_nan:].all() and not nan[:first_nan].any() and s[first_nan - 1] == np.inf
    assert np.all(s[1:first_nan] >= s[:first_nan - 1])
    same_value = (s[1:] == s[:-1]) | (nan[1:] & nan[:-1])
    assert np.array_equal(ks[1:] == ks[:-1], same_value)
    assert X.trim_keys(np.array([-0.0]))[0] == X.trim_keys(np.array([0.0]))[0] == np.uint64(1 << 63)
    assert X.trim_keys(np.array([np.nan, -np.nan])).tolist() == [2 ** 64 - 1] * 2


def test_every_round_of_the_select_chooses():
    """For each of the eight rounds some tested budget meets two or more
    occupied byte values among the keys that share the bytes fixed before."""
    f = X.key_f()
    keys = X.trim_keys(f[1:])
    budgets = X.key_budgets()
    n = len(f)
    assert all(1 <= mk < n for mk in budgets.values()) and len(set(budgets.values())) == len(budgets)
    chose = np.zeros(8, int)
    srt = np.sort(f[1:])
    for name, mk in budgets.items():
        occ, key = X.select_rounds(keys, mk)
        chose += np.array(occ) >= 2
        cut = X.quiet(TR.flags, X.key_tree()[0], np.zeros(8), np.inf, mk, -1)[2]["cut"]
        assert X.trim_keys(np.array([cut]))[0] == key, name        # the select's key is np.sort's element
        assert bits(cut) == bits(X.key_cut(mk)) or np.isnan(cut) and np.isnan(X.key_cut(mk))
    print("budgets whose select chooses, per round:", chose.tolist())
    assert np.all(chose >= 1), chose
    assert np.all(chose[[0, 1, 2, 5, 6]] >= 8)
    # where the named budgets put the cut
    cut = {name: X.key_cut(mk) for name, mk in budgets.items()}
    assert bits(cut["zero"]) == bits(cut["zero-tie"]) == 0
    assert cut["inf"] == np.inf and np.isnan(cut["nan"]) and np.isnan(cut["n-1"])
    t = budgets["tie"]
    assert srt[t - 1] == srt[t] and 2.0 < cut["tie"] < 2.0 + 2.0 ** -31
    for j in range(1, 5):
        assert 2.0 < cut[f"run20-{j}"] < 2.0 + 2.0 ** -31 < cut[f"run44-{j}"] < 2.0 + 2.0 ** -7
    assert 0 < cut["low"] < 1e-50 and 1e50 < cut["high"] < np.inf
    # a cut of 0, of NaN: nothing is below it; of +inf: the finite values are
    tree, root, _ = X.key_tree()
    for name, kept in (("zero", 1), ("nan", 1), ("n-1", 1), ("inf", 1 + int(np.isfinite(f[1:]).sum()))):
        assert X.quiet(TR.trim, tree, root, np.inf, budgets[name], -1)[2]["n_kept"] == kept, name


# ---- path windows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [0, 1])
def test_window_tables_are_sub_blocks(dense):
    case = C.DENSE[dense]
    S, A = C.dense_path(*case)
    w = X.windows(dense)
    assert len(w) == X.N_WINDOWS and {m for _, m in w} == set(range(2, 13))
    assert all(0 <= o and o + m <= len(S) for o, m in w) and len({o for o, _ in w}) > 60
    paths, acts = X.window_paths(dense)
    assert all(len(p) == m and len(a) == m - 1 for p, a, (_, m) in zip(paths, acts, w))
    # the pairs of three windows decided on their own: the dense table's sub-block
    n = len(S)
    picks = [2, 3, next(i for i, (o, m) in enumerate(w) if i > 3 and m >= 8 and 0 < o < n - m)]
    rows = {}
    _, O = C.terrain(case[0][0])
    import oracle
    oracle.set_scan_mode(1)
    for i, j in {(o + a, o + b) for o, m in (w[p] for p in picks) for a, b in C.pairs(m)}:
        rows[(i, j)] = O.attempt_connect(S[i], S[j], C.FORWARD)[0] == C.REACHED
    table = np.zeros(n * (n - 1) // 2, np.uint8)
    for (i, j), r in rows.items():
        table[i * (2 * n - i - 1) // 2 + (j - i - 1)] = r
    for p in picks:
        o, m = w[p]
        assert np.array_equal(X.window_block(table, n, o, m), C.oracle_table(case[0][0], paths[p], False))
    assert np.array_equal(X.window_block(np.arange(n * (n - 1) // 2), n, 0, n), np.arange(n * (n - 1) // 2))
