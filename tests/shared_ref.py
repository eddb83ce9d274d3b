"""RRT*'s kept connections through a remap, their ranking, and the joined path
of two trees, restated in numpy: the expected values of
test_gpu_shared_remap.py, test_gpu_tree_path.py and test_gpu_replan_session.py
(checked on their own in test_shared_ref.py).  Nothing here is the engine's:
the remap is boolean indexing, the ranking the first minimum in list order
(vectorised: the lists reach a million pairs), the join two parent walks.  Also the small trees and pair lists those tests share."""
import functools

import numpy as np

STATS = ("n_before", "n_kept", "n_dropped_a", "n_dropped_b")


# ---- the restatement --------------------------------------------------------------
def remap_pairs(pairs, remap_a=None, remap_b=None):
    """(kept pairs [k][2] int32 in list order, stats) of the list `pairs`
    ([n][2], vertices of tree a / tree b) under the remaps of the two trees
    (old index -> new index or -1; None: the identity).  A pair lost on both
    sides counts under a."""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    ra = pairs[:, 0] if remap_a is None else np.asarray(remap_a, np.int32)[pairs[:, 0]]
    rb = pairs[:, 1] if remap_b is None else np.asarray(remap_b, np.int32)[pairs[:, 1]]
    lost_a = ra < 0
    lost_b = ~lost_a & (rb < 0)
    keep = ~lost_a & ~lost_b
    out = np.stack([ra[keep], rb[keep]], axis=1).astype(np.int32).reshape(-1, 2)
    stats = dict(n_before=len(pairs), n_kept=int(keep.sum()), n_dropped_a=int(lost_a.sum()),
                 n_dropped_b=int(lost_b.sum()), error=0)
    return out, stats


def rank(pairs, ga, gb):
    """(best_a, best_b, best_cost) of a list ranked from no best at all
    (rrt_star_connect.cpp:181-193): in list order, a NaN cost skipped, a pair
    taken only when strictly cheaper, so ties stay with the earliest; (-1, -1,
    inf) when nothing is taken."""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    c = np.asarray(ga, np.float64)[p[:, 0]] + np.asarray(gb, np.float64)[p[:, 1]]
    c = np.where(c < np.inf, c, np.inf)   # NaN < x is False: skipped, like a cost of inf
    if len(c) == 0 or not c.min() < np.inf:
        return (-1, -1, np.inf)
    i = int(np.argmin(c))                 # the first of equal minima: the earliest
    return (int(p[i, 0]), int(p[i, 1]), float(c[i]))


def chain(parent, i):
    """root -> i along the parents (the root is vertex 0)."""
    path = [int(i)]
    while path[-1] != 0:
        path.append(int(parent[path[-1]]))
        assert len(path) <= len(parent), "not a tree"
    return path[::-1]


def join(ta, ia, tb, ib):
    """The joined path (rrt_connect.cpp:386-401) of tree dicts (v, act, parent,
    g): a's root -> ia, then b's ib -> root without ib, b's edges carrying the
    child's action.  (states [m][8], actions [m - 1][10], length, vertices from
    a, vertices from b)."""
    pa, rb = chain(ta["parent"], ia), chain(tb["parent"], ib)[::-1]
    va, vb = np.asarray(ta["v"], np.float64), np.asarray(tb["v"], np.float64)
    aa, ab = np.asarray(ta["act"], np.float64), np.asarray(tb["act"], np.float64)
    states = np.concatenate([va[pa], vb[rb[1:]]]).reshape(-1, 8)
    actions = np.concatenate([aa[pa[1:]], ab[rb[:-1]]]).reshape(-1, 10)
    return states, actions, ta["g"][ia] + tb["g"][ib], len(pa), len(rb) - 1


# ---- the shared inputs ------------------------------------------------------------
def pose_g(v, parent):
    """g as gbp_tree_load_host derives it: g[c] = g[parent[c]] + |xyz[c] -
    xyz[parent[c]]|, the squares summed in coordinate order."""
    n = len(parent)
    g = np.full(n, np.nan)
    g[0] = 0.0
    kids = {}
    for i in range(1, n):
        kids.setdefault(int(parent[i]), []).append(i)
    todo = [0]
    while todo:
        u = todo.pop()
        for c in kids.get(u, ()):
            d = v[c, :3] - v[u, :3]
            g[c] = g[u] + np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            todo.append(c)
    return g


@functools.lru_cache(maxsize=None)
def small_tree(seed, n=300):
    """A random recursive tree of n vertices whose edges run along x in steps
    of k / 4, k = 1 .. 4 (y = z = 0): every g is a multiple of 1 / 4, exact in
    binary whatever the order of the sums, and many vertices share a g.  The
    other state values and the actions are random and distinct per vertex."""
    rng = np.random.default_rng(seed)
    parent = np.r_[-1, [rng.integers(0, i) for i in range(1, n)]].astype(np.int32)
    v = rng.uniform(-1, 1, (n, 8))
    v[:, :3] = 0.0
    for i in range(1, n):
        v[i, 0] = v[parent[i], 0] + rng.integers(1, 5) * rng.choice([-0.25, 0.25])
    act = rng.uniform(-1, 1, (n, 10))
    act[0] = 0.0
    return dict(v=v, act=act, parent=parent, g=pose_g(v, parent))


def random_pairs(rng, n, na, nb):
    return np.stack([rng.integers(0, na, n), rng.integers(0, nb, n)], axis=1).astype(np.int32)


def random_remap(rng, n, keep=0.5):
    """A remap as a prune writes it: about `keep` of the n vertices kept (the
    root always), numbered in order."""
    k = rng.random(n) < keep
    k[0] = True
    return np.where(k, np.cumsum(k) - 1, -1).astype(np.int32)


def chain_against_the_index_order(n):
    """Vertex i's parent is i + 1, vertex n - 1 hangs under the root: vertex 1
    is n - 1 edges deep, every step of its walk to a larger index."""
    parent = np.r_[-1, np.arange(2, n), 0].astype(np.int32)
    rng = np.random.default_rng(n)
    v = rng.uniform(-1, 1, (n, 8))
    act = rng.uniform(-1, 1, (n, 10))
    act[0] = 0.0
    return dict(v=v, act=act, parent=parent, g=pose_g(v, parent))
