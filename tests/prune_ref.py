"""Pruning a tree against a changed terrain, restated in numpy (the expected
values of test_tree_prune_ref.py and test_gpu_tree_prune.py), and the inputs
those tests share: the oracle's trees on synth-rough-256 and the three changed
maps.  Nothing here is the engine's: edge decisions are the oracle's pair
checks, the keep rule a fixed-point loop, the compaction boolean indexing."""
import dataclasses
import functools

import numpy as np

import oracle
from global_body_planner_amd import planner
from global_body_planner_amd import terrain_data as td

FORWARD, REVERSE = 0, 1
XY = (1.0, 2.55, 4.02, 2.55)
# name -> (amount added to z, x0, x1, y0, y1)
BOXES = {
    "box1": (0.5, 1.6, 2.0, 2.2, 2.9),
    "box2": (0.3, 1.2, 1.5, 2.3, 2.8),
    "box3": (np.nan, 3.4, 3.8, 2.2, 2.9),
}
# tree set -> the oracle search that grows it (streams 101 / 102, star_delta 3.0)
SETS = {
    "S": dict(batch=1024, seed=3, max_halves=300, star=True),
    "C": dict(batch=256, seed=7, max_halves=200),
}


# ---- the restatement --------------------------------------------------------------
def edge_valid(O, tree, direction, adaptive=False):
    """[n] uint8: the pair check of (v[parent[i]], act[i], direction) on O's
    terrain; the root's entry is 1 (never tested)."""
    v, act, parent = tree["v"], tree["act"], np.asarray(tree["parent"])
    ok = np.ones(len(parent), np.uint8)
    if len(parent) > 1:
        ok[1:] = O.validate_pairs(v[parent[1:]], act[1:], direction, adaptive=adaptive)[0]
    return ok


def keep_rule(parent, ok):
    """keep[i]: every edge between i and the root has ok = 1."""
    parent = np.asarray(parent)
    keep = np.asarray(ok).astype(bool).copy()
    keep[0] = True
    while True:
        nxt = keep.copy()
        nxt[1:] &= keep[parent[1:]]
        if np.array_equal(nxt, keep):
            return keep
        keep = nxt


def prune(tree, ok):
    """(pruned tree, remap, stats) of a tree dict (v, act, parent and, if it
    has one, g) under edge decisions ok."""
    parent = np.asarray(tree["parent"])
    keep = keep_rule(parent, ok)
    remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    out = {k: np.asarray(tree[k])[keep] for k in ("v", "act", "g") if k in tree}
    out["parent"] = np.where(parent[keep] >= 0, remap[parent[keep]], -1).astype(np.int32)
    bad = ~np.asarray(ok).astype(bool)
    bad[0] = False
    stats = dict(n_before=len(parent), n_kept=int(keep.sum()), n_edge_invalid=int(bad.sum()),
                 n_inherited=int((~keep & ~bad).sum()))
    return out, remap, stats


def children(parent):
    """vertex -> the sorted list of its children."""
    out = {}
    for i, p in enumerate(np.asarray(parent)):
        if p >= 0:
            out.setdefault(int(p), []).append(i)
    return out


# ---- the shared inputs ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def terrain(box=None):
    """(TerrainData, OracleTerrain) of synth-rough-256, unchanged or with a box."""
    data = td.synth_rough(256)
    if box is not None:
        dz, x0, x1, y0, y1 = BOXES[box]
        z = np.array(data.z, np.float64)
        ix = (data.x >= x0) & (data.x <= x1)
        iy = (data.y >= y0) & (data.y <= y1)
        z[np.ix_(ix, iy)] += dz
        data = dataclasses.replace(data, z=z, name=f"{data.name}-{box}")
    return data, oracle.OracleTerrain.from_data(data)


def start_goal():
    _, O = terrain()
    hs, _ = O.ground_height(XY[0], XY[1])
    hg, _ = O.ground_height(XY[2], XY[3])
    return planner.start_goal_state(hs, XY[0], XY[1]), planner.start_goal_state(hg, XY[2], XY[3])


@functools.lru_cache(maxsize=None)
def search(which):
    """The oracle's search for tree set S or C on the unchanged terrain."""
    _, O = terrain()
    oracle.set_scan_mode(1)  # bisection: the reference's brackets, quickly
    start, goal = start_goal()
    return O.plan(start, goal, nthreads=16, **SETS[which])


@functools.lru_cache(maxsize=None)
def expected(which, box, adaptive=False):
    """Per tree (a, b): (pruned tree, remap, stats, ok) of set `which` on the
    terrain with `box` (None: unchanged)."""
    _, O = terrain(box)
    oracle.set_scan_mode(1)
    r = search(which)
    out = []
    for name, direction in (("a", FORWARD), ("b", REVERSE)):
        ok = edge_valid(O, r[name], direction, adaptive)
        out.append(prune(r[name], ok) + (ok,))
    return tuple(out)


def counts(entry):
    """(own edge failed, all pruned, through an ancestor only) of an expected() entry."""
    st = entry[2]
    return st["n_edge_invalid"], st["n_before"] - st["n_kept"], st["n_inherited"]
