"""A/B of pruning a device tree against a changed terrain, on one GPU, in one process.

A  gbp_tree_revalidate_host: the edges gathered and decided on the device, one
   read-back of the flags, FRAGILE edges re-decided with glibc, the prune on
   the device.
B  the route without it: gbp_tree_read, gbp_validate_pairs_host on
   (v[parent], a), the keep rule and the compaction in numpy (pointer doubling,
   boolean indexing), gbp_tree_load_host, which writes the tree with one lane.

Two trees:
  small  64 copies of the oracle's 95-vertex RRT* tree under one root (6,017
         vertices, tests/prune_ref.py), synth-rough-256 with box 1
  large  tree a of config 5's search (synth-fractal-4096, 4096 draws per half)
         grown on the device to roughly 50k vertices; the changed map raises a
         1 m wide strip across the tree by 0.5 m
Both forms start from the same loaded tree (loading it is not timed) and must
leave the same tree.  They alternate, REPS times each after a warm-up of
both; host clock around calls that end synchronised.  Then form A's two
stages on their own: stage A (gather + pair checks) from device events, stage
B (gbp_tree_prune_dev, which synchronises) from the host clock.

    python tools/tree_prune_ab.py --out profiles/tree_prune_ab.txt
"""
import argparse
import ctypes
import dataclasses
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
from global_body_planner_amd.engine import _ptr, _stream  # noqa: E402

REPS = 6


def ms(xs):
    return (f"median {1e3 * statistics.median(xs):9.3f} ms  min {1e3 * min(xs):9.3f}  "
            f"max {1e3 * max(xs):9.3f}")


def numpy_prune(v, a, parent, ok):
    """keep rule by pointer doubling, compaction by boolean indexing."""
    n = len(parent)
    anc = np.where(parent >= 0, parent, 0).astype(np.int64)
    dead = ~ok.astype(bool)
    dead[0] = False
    reach = 1
    while reach < n:
        dead = dead | dead[anc]
        anc = anc[anc]
        reach *= 2
    keep = ~dead
    remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    p = np.where(parent[keep] >= 0, remap[parent[keep]], -1).astype(np.int32)
    return v[keep], a[keep], p, remap


def form_a(T, tree, direction):
    return tree.revalidate(T, direction)


def form_b(T, tree, direction):
    v, a, p, _ = tree.read()
    ok = np.ones(len(p), np.uint8)
    ok[1:] = T.validate_pairs_host(v[p[1:]], a[1:], direction)[0]
    v2, a2, p2, remap = numpy_prune(v, a, p, ok)
    tree.load(v2, a2, p2)
    return remap


def loaded(arrs):
    t = engine.DeviceTree(arrs["v"][0], capacity=len(arrs["parent"]))
    t.load(arrs["v"], arrs["act"], arrs["parent"])
    return t


def stages(T, arrs, direction):
    """(stage A seconds from device events, stage B seconds from the host clock)."""
    lib = L.load()
    tree = loaded(arrs)
    n = len(tree)
    ev = torch.empty(n, dtype=torch.uint8, device=T.torch_device)
    fl = torch.empty(n, dtype=torch.int32, device=T.torch_device)
    remap = torch.empty(n, dtype=torch.int32, device=T.torch_device)
    st = torch.empty(4, dtype=torch.int64, device=T.torch_device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    L.check(lib.gbp_tree_revalidate_dev(T._h, tree._h, n, direction, 0, _ptr(ev), _ptr(fl),
                                        _stream(T.device)), "revalidate_dev")
    e1.record()
    e1.synchronize()
    t0 = time.perf_counter()
    L.check(lib.gbp_tree_prune_dev(tree._h, n, _ptr(ev), _ptr(remap), _ptr(st), _stream(T.device)),
            "prune_dev")
    return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0


def measure(label, T, arrs, direction, lines):
    ta, tb, sa, sb = [], [], [], []
    for rep in range(REPS + 1):  # the first round warms both forms up and compares them
        tree = loaded(arrs)
        t0 = time.perf_counter()
        remap_a, stats = form_a(T, tree, direction)
        da = time.perf_counter() - t0
        out_a = tree.read()
        tree = loaded(arrs)
        t0 = time.perf_counter()
        remap_b = form_b(T, tree, direction)
        db = time.perf_counter() - t0
        out_b = tree.read()
        if rep == 0:
            assert np.array_equal(remap_a, remap_b), label
            for x, y in zip(out_a, out_b):
                assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), label
            stages(T, arrs, direction)
            continue
        ta.append(da)
        tb.append(db)
        a, b = stages(T, arrs, direction)
        sa.append(a)
        sb.append(b)
    lines += [f"{label}: {stats['n_before']} vertices -> {stats['n_kept']} "
              f"({stats['n_edge_invalid']} own edge failed, {stats['n_inherited']} through an "
              f"ancestor, {stats['n_resolved']} re-decided with glibc)",
              f"  A gbp_tree_revalidate_host                   {ms(ta)}",
              f"  B read, validate_pairs_host, numpy, load     {ms(tb)}   "
              f"B / A of medians {statistics.median(tb) / statistics.median(ta):.2f}x",
              f"  A's stage A (gather + pair checks, events)   {ms(sa)}",
              f"  A's stage B (gbp_tree_prune_dev, host clock) {ms(sb)}"]
    print("\n".join(lines[-5:]), flush=True)


def small_case():
    from tests import prune_ref as R
    from tests.test_gpu_tree_prune import _copies
    return R.terrain("box1")[0], _copies(R.search("S")["a"], 64)


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
    xm = float(np.median(arrs["v"][:, 0]))
    z = np.array(data.z, np.float64)
    z[(data.x >= xm - 0.5) & (data.x <= xm + 0.5), :] += 0.5
    return dataclasses.replace(data, z=z, name=data.name + "-strip"), arrs, xm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_prune_ab.txt"))
    ap.add_argument("--grow-halves", type=int, default=21000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tree_prune_ab.py measures on the GPU: no device found")
    lines = [f"pruning a device tree against a changed terrain, {torch.cuda.get_device_name(0)}, "
             f"{REPS} alternating repetitions of each form after a warm-up"]
    data, arrs = small_case()
    measure("small (64 copies of the oracle's RRT* tree, synth-rough-256 box 1)",
            engine.Terrain.from_data(data, device=0), arrs, L.FORWARD, lines)
    data, arrs, xm = large_case(args.grow_halves)
    measure(f"large (config 5's tree a after {args.grow_halves} halves, synth-fractal-4096, "
            f"+0.5 m on x in [{xm - 0.5:.2f}, {xm + 0.5:.2f}])",
            engine.Terrain.from_data(data, device=0), arrs, L.FORWARD, lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
