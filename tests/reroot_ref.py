"""Re-rooting a tree at one of its vertices, restated in numpy (the expected
values of test_tree_reroot_ref.py and test_gpu_tree_reroot.py).  Nothing here
is the engine's: the descendants are a fixed-point loop, the order is
[k] + sorted(rest), g is a walk from the new root with oracle.pose_distance,
the stats are counted, and edge decisions are prune_ref.edge_valid's."""
import functools

import numpy as np

import oracle
from tests import prune_ref as R

FORWARD, REVERSE = R.FORWARD, R.REVERSE
STATS = ("n_before", "n_kept", "n_outside", "n_edge_invalid", "n_inherited", "depth")


def below(parent, k):
    """below[i]: k lies on i's parent chain (i = k included)."""
    parent = np.asarray(parent)
    out = np.zeros(len(parent), bool)
    out[k] = True
    while True:
        nxt = out.copy()
        has = parent >= 0
        nxt[has] |= out[parent[has]]
        if np.array_equal(nxt, out):
            return out
        out = nxt


def keep_rule(parent, k, ok=None):
    """keep[i]: i is below k and every edge from i up to (excluding) k has ok = 1."""
    parent = np.asarray(parent)
    keep = below(parent, k)
    if ok is not None:
        keep &= np.asarray(ok).astype(bool)
        keep[k] = True
    idx = np.array([i for i in range(len(parent)) if i != k and parent[i] >= 0], np.int64)
    while True:
        nxt = keep.copy()
        nxt[idx] &= keep[parent[idx]]
        if np.array_equal(nxt, keep):
            return keep
        keep = nxt


def derive_g(v, parent):
    """g[0] = 0, g[c] = g[parent[c]] + poseDistance(v[parent[c]], v[c]): one
    addition per edge, from the root down."""
    n = len(parent)
    kids = R.children(parent)
    g = np.zeros(n)
    todo = [0]
    while todo:
        u = todo.pop()
        for c in kids.get(u, []):
            g[c] = g[u] + oracle.pose_distance(v[u], v[c])
            todo.append(c)
    return g


def reroot(tree, k, ok=None):
    """(re-rooted tree with g, remap, stats) of a tree dict (v, act, parent)
    at vertex k, under edge decisions ok (None: every edge holds)."""
    parent = np.asarray(tree["parent"])
    n = len(parent)
    under = below(parent, k)
    keep = keep_rule(parent, k, ok)
    rest = sorted(int(i) for i in np.flatnonzero(keep) if i != k)
    order = np.array([k] + rest, np.int64)
    remap = np.full(n, -1, np.int32)
    remap[order] = np.arange(len(order), dtype=np.int32)
    out = dict(v=np.asarray(tree["v"])[order].copy(), act=np.asarray(tree["act"])[order].copy())
    out["act"][0] = 0.0
    p = np.where(parent[order] >= 0, remap[np.maximum(parent[order], 0)], -1).astype(np.int32)
    p[0] = -1
    out["parent"] = p
    out["g"] = derive_g(out["v"], p)
    depth = np.zeros(len(order), np.int64)
    while True:   # a fixed point again: one more edge than the parent
        nxt = depth.copy()
        nxt[1:] = depth[p[1:]] + 1
        if np.array_equal(nxt, depth):
            break
        depth = nxt
    bad = np.zeros(n, bool) if ok is None else ~np.asarray(ok).astype(bool)
    bad &= under
    bad[k] = False
    stats = dict(n_before=n, n_kept=len(order), n_outside=int((~under).sum()),
                 n_edge_invalid=int(bad.sum()), n_inherited=int((under & ~keep & ~bad).sum()),
                 depth=int(depth.max()))
    return out, remap, stats


@functools.lru_cache(maxsize=None)
def expected(which, name, k, box=None, adaptive=False):
    """(re-rooted tree, remap, stats) of tree `name` ("a" / "b") of set `which`
    at vertex k, on the terrain with `box` (None: no edge is tested)."""
    tree = R.search(which)[name]
    ok = None
    if box is not None:
        _, O = R.terrain(box)
        oracle.set_scan_mode(1)
        ok = R.edge_valid(O, tree, FORWARD if name == "a" else REVERSE, adaptive)
    return reroot(tree, k, ok)


def random_recursive_tree(n=6017, seed=20261020):
    """parent[i] = integers(0, i), random states and actions."""
    rng = np.random.default_rng(seed)
    parent = np.r_[-1, [rng.integers(0, i) for i in range(1, n)]].astype(np.int32)
    v = rng.uniform(-3.0, 3.0, (n, 8))
    act = rng.uniform(-1.0, 1.0, (n, 10))
    act[0] = 0.0
    return dict(v=v, act=act, parent=parent)


def permuted(tree, k, seed):
    """The same tree with its non-root vertices renumbered at random, and k's
    new number."""
    n = len(tree["parent"])
    new = np.r_[0, 1 + np.random.default_rng(seed).permutation(n - 1)]   # old index -> new index
    out = {key: np.empty_like(tree[key]) for key in ("v", "act", "parent")}
    for key in ("v", "act"):
        out[key][new] = tree[key]
    out["parent"][new] = np.where(tree["parent"] >= 0, new[np.maximum(tree["parent"], 0)], -1)
    return out, int(new[k])


def chain_against_the_index_order(n, seed=5):
    """Vertex i's parent is i + 1, vertex n - 1 hangs under the root; distinct
    random states."""
    rng = np.random.default_rng(seed)
    act = rng.uniform(-1.0, 1.0, (n, 10))
    act[0] = 0.0
    return dict(v=rng.uniform(-3.0, 3.0, (n, 8)), act=act,
                parent=np.r_[-1, np.arange(2, n), 0].astype(np.int32))
