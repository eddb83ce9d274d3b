"""Trimming a tree by cost (gbp_tree_trim_flags_dev + gbp_tree_prune_dev,
DESIGN §5.13), restated in numpy: the expected values of
test_tree_trim_ref.py, test_gpu_tree_trim.py and test_gpu_replan_trim.py, and
the inputs they share.  Nothing here is the engine's: f is three squares summed
left to right, the cut an element of np.sort, the protected chain a parent
walk, the keep rule and the compaction tests/prune_ref.py's."""
import functools

import numpy as np

from tests import prune_ref as R
from tests import shared_ref as SR

STATS = ("n_before", "n_kept", "n_over_bound", "n_over_budget", "n_protected", "n_inherited")
# the session test's search (tests/test_gpu_replan_session.py) on synth-rough-256
SESSION = dict(star=True, stream_a=401, stream_b=402, batch=1024, seed=11, nthreads=16)
SESSION_HALVES = 200
# (max_keep, vertices kept) of _copies(S.a, 64): 6,017 vertices, 64-way ties
BUDGETS = ((1024, 961), (1025, 1025), (2048, 1985), (3000, 2945), (6016, 5953), (6017, 6017))


# ---- the restatement --------------------------------------------------------------
def f_values(tree, other_root):
    """f[i] = g[i] + poseDistance(v[i], r): the squares of the three
    differences summed in coordinate order from zero, then the root."""
    v = np.asarray(tree["v"], np.float64)
    r = np.asarray(other_root, np.float64)
    d0, d1, d2 = (r[k] - v[:, k] for k in range(3))
    s = ((0.0 + d0 * d0) + d1 * d1) + d2 * d2
    return np.asarray(tree["g"], np.float64) + np.sqrt(s)


def flags(tree, other_root, bound=np.inf, max_keep=0, protect=-1):
    """(keep [n] uint8, f [n], stats) of stage A: the bound test, the budget's
    cut and the protected chain.  stats holds cut and the four counts."""
    f = f_values(tree, other_root)
    n = len(f)
    over_bound = f > bound
    over_bound[0] = False
    over_budget = np.zeros(n, bool)
    cut = np.inf
    if max_keep >= 1 and n > max_keep:
        cut = np.sort(f[1:])[max_keep - 1]     # (np.sort puts NaN last, above +inf)
        over_budget = ~over_bound & ~(f < cut)
        over_budget[0] = False
    prot = np.zeros(n, bool)
    if protect >= 0:
        prot[SR.chain(tree["parent"], protect)] = True
    fail = over_bound | over_budget
    keep = ~fail | prot
    keep[0] = True
    stats = dict(n_before=n, n_over_bound=int(over_bound.sum()), n_over_budget=int(over_budget.sum()),
                 n_protected=int((fail & prot).sum()), cut=float(cut))
    return keep.astype(np.uint8), f, stats


def trim(tree, other_root, bound=np.inf, max_keep=0, protect=-1):
    """(trimmed tree, remap, stats, keep, f): stage A's flags through
    prune_ref's keep rule and compaction."""
    keep, f, stats = flags(tree, other_root, bound, max_keep, protect)
    out, remap, ps = R.prune(tree, keep)
    stats["n_kept"], stats["n_inherited"] = ps["n_kept"], ps["n_inherited"]
    assert ps["n_edge_invalid"] == stats["n_over_bound"] + stats["n_over_budget"] - stats["n_protected"]
    return out, remap, stats, keep, f


def session_trim(ta, tb, pairs, best, max_vertices=0):
    """ReplanSession.trim on the host: both trees trimmed toward the other's
    root (tree b toward the root tree a had before: a trim keeps the root),
    bound = the held best cost, the best connection's vertices protected, the
    list carried through both remaps and ranked again.  best = (best_a, best_b,
    best_cost), (-1, -1, inf) when none is held.
    -> (ta', tb', pairs', best', (stats a, stats b), shared stats)"""
    bound = best[2] if best[0] >= 0 else np.inf
    ra, rb = ta["v"][0], tb["v"][0]
    xa = trim(ta, rb, bound, max_vertices, best[0])
    xb = trim(tb, ra, bound, max_vertices, best[1])
    kept, shared = SR.remap_pairs(pairs, xa[1], xb[1])
    return xa[0], xb[0], kept, SR.rank(kept, xa[0]["g"], xb[0]["g"]), (xa[2], xb[2]), shared


# ---- the shared inputs ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def session_search():
    """The oracle's run of the session test: 200 halves, seed 11."""
    import oracle
    _, O = R.terrain()
    oracle.set_scan_mode(1)
    start, goal = R.start_goal()
    return O.plan(start, goal, max_halves=SESSION_HALVES, **SESSION)


def met_pairs(r):
    """The kept connections of an oracle run r as a set: the pairs of a
    start-tree and a goal-tree vertex at the same state."""
    same = np.abs(r["a"]["v"][:, None, :] - r["b"]["v"][None, :, :]).max(axis=2) < 1e-9
    return {(int(a), int(b)) for a, b in np.argwhere(same)}


@functools.lru_cache(maxsize=None)
def big(permute=False):
    """(tree of 6,017 vertices, the goal root its f is taken toward, set S's
    best cost)."""
    r = R.search("S")
    from tests.test_gpu_tree_prune import _copies, _permuted   # the prune test's many-tile tree
    t = _copies(r["a"], 64)
    if permute:
        t = _permuted(t, 20251020)
    return t, r["b"]["v"][0], r["best_cost"]
