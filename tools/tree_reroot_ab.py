"""A/B of re-rooting a device tree at one of its vertices, on one GPU, in one process.

A  gbp_tree_reroot_host with no terrain: the keep rule and the depth by pointer
   jumping, the compaction with the new root first, the move, g derived again
   level by level, all in HBM.
B  the route without it: gbp_tree_read, the subtree and the renumbering in
   numpy (pointer doubling, boolean indexing), gbp_tree_load_host, which
   writes the tree and derives g with one lane.

Two trees:
  small  the random recursive tree of tests/reroot_ref.py (6,017 vertices),
         re-rooted at vertex 1
  large  tree a of config 5's search (synth-fractal-4096, 4096 draws per half)
         grown on the device to roughly 50k vertices, re-rooted at the second
         vertex of its best path
Both forms start from the same loaded tree (loading it is not timed) and must
leave the same tree.  They alternate, REPS times each after a warm-up of
both; host clock around calls that end synchronised.  Form A's three parts
come from the stream events the entry records (gbp_tree_reroot_last), with
the number of kernels it launched.

    python tools/tree_reroot_ab.py --out profiles/tree_reroot_ab.txt
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from global_body_planner_amd import _lib as L  # noqa: E402
from global_body_planner_amd import engine, planner  # noqa: E402
from global_body_planner_amd import terrain_data as td  # noqa: E402

REPS = 6


def ms(xs, scale=1e3):
    return (f"median {scale * statistics.median(xs):9.3f} ms  min {scale * min(xs):9.3f}  "
            f"max {scale * max(xs):9.3f}")


def numpy_reroot(v, a, parent, k):
    """the subtree of k by pointer doubling, [k] + the rest in ascending index."""
    n = len(parent)
    anc = np.where(parent >= 0, parent, 0).astype(np.int64)
    anc[k] = k
    reach = 1
    while reach < n:
        anc = anc[anc]
        reach *= 2
    keep = anc == k
    keep[k] = False
    order = np.r_[k, np.flatnonzero(keep)]
    remap = np.full(n, -1, np.int32)
    remap[order] = np.arange(len(order), dtype=np.int32)
    p = remap[np.maximum(parent[order], 0)]
    p[0] = -1
    a2 = a[order]
    a2[0] = 0.0
    return v[order], a2, p.astype(np.int32), remap


def form_b(tree, k):
    v, a, p, _ = tree.read()
    v2, a2, p2, remap = numpy_reroot(v, a, p, k)
    tree.load(v2, a2, p2)
    return remap


def loaded(arrs):
    t = engine.DeviceTree(arrs["v"][0], capacity=len(arrs["parent"]))
    t.load(arrs["v"], arrs["act"], arrs["parent"])
    return t


def last_call():
    parts = (ctypes.c_double * 3)()
    launches = ctypes.c_int64(0)
    L.check(L.load().gbp_tree_reroot_last(parts, ctypes.byref(launches)), "reroot_last")
    return list(parts), launches.value


def measure(label, arrs, k, lines):
    ta, tb, parts = [], [], []
    for rep in range(REPS + 1):  # the first round warms both forms up and compares them
        tree = loaded(arrs)
        t0 = time.perf_counter()
        remap_a, stats = tree.reroot(k)
        da = time.perf_counter() - t0
        split, launches = last_call()
        out_a = tree.read()
        tree = loaded(arrs)
        t0 = time.perf_counter()
        remap_b = form_b(tree, k)
        db = time.perf_counter() - t0
        out_b = tree.read()
        if rep == 0:
            assert np.array_equal(remap_a, remap_b), label
            for x, y in zip(out_a, out_b):
                assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), label
            continue
        ta.append(da)
        tb.append(db)
        parts.append(split)
    lines += [f"{label}: {stats['n_before']} vertices, re-rooted at {k} -> {stats['n_kept']} kept "
              f"({stats['n_outside']} not below it), depth {stats['depth']}, {launches} kernel launches",
              f"  A gbp_tree_reroot_host                       {ms(ta)}",
              f"  B read, numpy, gbp_tree_load_host            {ms(tb)}   "
              f"B / A of medians {statistics.median(tb) / statistics.median(ta):.2f}x",
              f"  A's keep rule and depth (events)             {ms([p[0] for p in parts], 1.0)}",
              f"  A's compaction, move, sort by depth (events) {ms([p[1] for p in parts], 1.0)}",
              f"  A's g by levels, sizes read first (events)   {ms([p[2] for p in parts], 1.0)}"]
    print("\n".join(lines[-6:]), flush=True)


def small_case():
    from tests import reroot_ref as RR
    return RR.random_recursive_tree(), 1


def large_case(halves):
    from tools.config5 import first_valid
    data = td.by_name("synth-fractal-4096")
    T = engine.Terrain.from_data(data, device=0)
    mid = data.x[-1] / 2
    start, goal = first_valid(T, 1.0, mid, 0.02), first_valid(T, 9.0, mid, -0.02)
    T.close()
    grown = planner.plan_rrt_star_connect(data, start, goal, batch=4096, max_time=300.0,
                                          seed=20251020, max_halves=halves, trees=True,
                                          tree_capacity=1 << 17, device_loop=True)
    arrs = {k: grown["a"][k] for k in ("v", "act", "parent")}
    chain, i = [], int(grown["meet_a"])
    while i >= 0:
        chain.append(i)
        i = int(arrs["parent"][i])
    if len(chain) < 2:
        raise SystemExit("the best path leaves tree a at its root: nothing to re-root at")
    return arrs, chain[-2], len(chain)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_reroot_ab.txt"))
    ap.add_argument("--grow-halves", type=int, default=21000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tree_reroot_ab.py measures on the GPU: no device found")
    lines = [f"re-rooting a device tree at one of its vertices, {torch.cuda.get_device_name(0)}, "
             f"{REPS} alternating repetitions of each form after a warm-up"]
    arrs, k = small_case()
    measure("small (random recursive tree)", arrs, k, lines)
    arrs, k, on_path = large_case(args.grow_halves)
    measure(f"large (config 5's tree a after {args.grow_halves} halves, synth-fractal-4096, the second "
            f"of {on_path} path vertices)", arrs, k, lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
