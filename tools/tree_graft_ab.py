"""A/B of grafting a device tree onto a root state that is none of its vertices,
on one GPU, in one process.

A  gbp_tree_graft_host: the candidates, their connect actions and pair checks
   by one wave each, the keep rule on the tree with one more vertex, the
   compaction, the move, the root's list and g derived again, all in HBM
   (DESIGN 5.11).
B  the route without it, through entries that were there before:
   gbp_tree_read, the candidates and their connect actions in numpy, their
   pair checks through gbp_validate_pairs_host, the graft in numpy (pointer
   doubling, boolean indexing), gbp_tree_load_host, which writes the tree and
   derives g with one lane.

The tree: tree a of config 5's search (synth-fractal-4096, 4096 draws per
half) grown on the device; the root: the state half way along the second edge
of its best path, and the start moved by (+0.10, +0.05) on the ground; radius
3.0.  Both forms start from the same loaded tree
(loading it is not timed) and must leave the same tree.  They alternate, REPS
times each after a warm-up of both that compares them bit for bit; host clock
around calls that end synchronised.  Form A's parts: the checks from stream
events around a stage-A launch of its own on the same tree (it changes
nothing), the rest from the events the entry records (gbp_tree_graft_last),
with the number of kernels it launched.

    python tools/tree_graft_ab.py --out profiles/tree_graft_ab.txt
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
V_NOM, KINEMATICS_RES, F_MAX, M_CONST, G_CONST = 0.75, 0.05, 637.0, 13.0, 9.81


def ms(xs, scale=1e3):
    return (f"median {scale * statistics.median(xs):9.3f} ms  min {scale * min(xs):9.3f}  "
            f"max {scale * max(xs):9.3f}")


def stance(s, a, t):
    """planning_utils.cpp:237-274 for one state."""
    t_s = a[6]
    o = np.empty(8)
    for q, dq, lo, hi in ((0, 3, 0, 3), (1, 4, 1, 4), (2, 5, 2, 5), (6, 7, 8, 9)):
        o[q] = s[q] + s[dq] * t + 0.5 * a[lo] * t * t + ((a[hi] - a[lo]) * (t * t * t)) / (6.0 * t_s)
        o[dq] = s[dq] + a[lo] * t + ((a[hi] - a[lo]) * t * t) / (2.0 * t_s)
    return o


def connect_actions(root, v, t_s):
    """rrt_connect.cpp:53-63 from `root` to every row of v."""
    a = np.zeros((len(v), 10))
    t2 = t_s * t_s
    for k, (q, dq) in enumerate(((0, 3), (1, 4), (2, 5), (6, 7))):
        td_, to, dtd, dto = root[q], v[:, q], root[dq], v[:, dq]
        lo = -(2.0 * (3.0 * td_ - 3.0 * to + 2.0 * dtd * t_s + dto * t_s)) / t2
        hi = (2.0 * (3.0 * td_ - 3.0 * to + dtd * t_s + 2.0 * dto * t_s)) / t2
        if k < 3:
            a[:, k], a[:, 3 + k] = lo, hi
        else:
            a[:, 8], a[:, 9] = lo, hi
    a[:, 6] = t_s
    return a


def valid_actions(a):
    """planning_utils.cpp:519-556."""
    f_td = M_CONST * np.stack([a[:, 0], a[:, 1], a[:, 2] + G_CONST], 1)
    f_to = M_CONST * np.stack([a[:, 3], a[:, 4], a[:, 5] + G_CONST], 1)
    ok = (a[:, 6] > 0) & (a[:, 7] >= 0)
    for f in (f_td, f_to):
        ok &= np.sqrt(f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2]) < F_MAX
        ok &= (f[:, 2] >= 0) & (np.sqrt(f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) < f[:, 2])
    return ok & (a[:, 8] < F_MAX) & (a[:, 9] < F_MAX)


def form_b(tree, T, root, radius):
    v, a, parent, _ = tree.read()
    n = len(parent)
    d = v[:, :3] - root[:3]
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    t_s = dist / V_NOM
    cand = dist <= radius
    rows = np.flatnonzero(cand & (t_s > KINEMATICS_RES))
    act = connect_actions(root, v[rows], t_s[rows])
    good = valid_actions(act)
    rows, act = rows[good], act[good]
    ok = T.validate_pairs_host(np.repeat(root[None], len(rows), 0), act, L.FORWARD)[0]
    attach = np.zeros(n, bool)
    attach[rows[ok != 0]] = True
    new_a = a.copy()
    new_a[rows[ok != 0]] = act[ok != 0]
    # the tree of n + 1 vertices whose vertex n is the root; vertex n + 1 stands for "outside"
    anc = np.r_[np.where(attach, n, np.where(parent >= 0, parent, n + 1)), n, n + 1].astype(np.int64)
    reach = 1
    while reach < n + 1:
        anc = anc[anc]
        reach *= 2
    order = np.flatnonzero(anc[:n] == n)
    remap = np.full(n, -1, np.int32)
    remap[order] = 1 + np.arange(len(order), dtype=np.int32)
    p2 = np.r_[-1, np.where(attach[order], 0, remap[np.maximum(parent[order], 0)])].astype(np.int32)
    tree.load(np.r_[root[None], v[order]], np.r_[np.zeros((1, 10)), new_a[order]], p2)
    return remap, int(cand.sum()), int(attach.sum())


def loaded(arrs):
    t = engine.DeviceTree(arrs["v"][0], capacity=len(arrs["parent"]) + 1)
    t.load(arrs["v"], arrs["act"], arrs["parent"])
    return t


def last_call():
    parts = (ctypes.c_double * 3)()
    launches = ctypes.c_int64(0)
    L.check(L.load().gbp_tree_graft_last(parts, ctypes.byref(launches)), "graft_last")
    return list(parts), launches.value


def measure(label, arrs, T, root, radius, lines):
    ta, tb, parts, checks = [], [], [], []
    for rep in range(REPS + 1):  # the first round warms both forms up and compares them
        tree = loaded(arrs)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tree.graft_check(root, radius, T, L.FORWARD)
        e1.record()
        e1.synchronize()
        t0 = time.perf_counter()
        remap_a, stats = tree.graft(root, radius, T, L.FORWARD)
        da = time.perf_counter() - t0
        split, launches = last_call()
        out_a = tree.read()
        tree = loaded(arrs)
        t0 = time.perf_counter()
        remap_b, n_cand, n_att = form_b(tree, T, root, radius)
        db = time.perf_counter() - t0
        out_b = tree.read()
        if rep == 0:
            assert np.array_equal(remap_a, remap_b), label
            assert (n_cand, n_att) == (stats["n_candidates"], stats["n_attached"]), label
            for x, y in zip(out_a, out_b):
                assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), label
            continue
        ta.append(da)
        tb.append(db)
        parts.append(split)
        checks.append(e0.elapsed_time(e1))
    lines += [f"{label}: {stats['n_before']} vertices, {stats['n_candidates']} within {radius}, "
              f"{stats['n_checked']} pair checks, {stats['n_attached']} attached -> {stats['n_kept']} kept "
              f"({stats['n_outside']} under no attached vertex), depth {stats['depth']}, "
              f"{stats['n_resolved']} re-decided with glibc, 1 + {launches} kernel launches",
              f"  A gbp_tree_graft_host                          {ms(ta)}",
              f"  B read, numpy, validate_pairs_host, load_host  {ms(tb)}   "
              f"B / A of medians {statistics.median(tb) / statistics.median(ta):.2f}x",
              f"  A's checks, one wave per vertex (events)       {ms(checks, 1.0)}",
              f"  A's keep rule, compaction, move, root (events) "
              f"{ms([p[0] + p[1] for p in parts], 1.0)}",
              f"  A's g by levels, sizes read first (events)     {ms([p[2] for p in parts], 1.0)}"]
    print("\n".join(lines[-6:]), flush=True)


def large_case(halves):
    from tools.config5 import first_valid
    data = td.by_name("synth-fractal-4096")
    T = engine.Terrain.from_data(data, device=0)
    mid = data.x[-1] / 2
    start, goal = first_valid(T, 1.0, mid, 0.02), first_valid(T, 9.0, mid, -0.02)
    grown = planner.plan_rrt_star_connect(data, start, goal, batch=4096, max_time=300.0,
                                          seed=20251020, max_halves=halves, trees=True,
                                          tree_capacity=1 << 17, device_loop=True)
    arrs = {k: grown["a"][k] for k in ("v", "act", "parent")}
    chain, i = [], int(grown["meet_a"])
    while i >= 0:
        chain.append(i)
        i = int(arrs["parent"][i])
    chain = chain[::-1]
    if len(chain) < 3:
        raise SystemExit("the best path has no second edge in tree a")
    k = chain[2]
    root = stance(arrs["v"][chain[1]], arrs["act"][k], arrs["act"][k][6] / 2)
    # a second root: the start moved by (+0.10, +0.05), its height above the ground kept
    near = np.array(start, np.float64)
    h0 = T.height_host(near[None, :2])[0][0]
    near[:2] += (0.10, 0.05)
    near[2] += T.height_host(near[None, :2])[0][0] - h0
    return T, arrs, root, len(chain), near


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_graft_ab.txt"))
    ap.add_argument("--grow-halves", type=int, default=21000)
    ap.add_argument("--radius", type=float, default=3.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tree_graft_ab.py measures on the GPU: no device found")
    lines = [f"grafting a device tree onto a root state off the tree, {torch.cuda.get_device_name(0)}, "
             f"{REPS} alternating repetitions of each form after a warm-up"]
    T, arrs, root, on_path, near = large_case(args.grow_halves)
    measure(f"config 5's tree a after {args.grow_halves} halves, synth-fractal-4096, the root half way "
            f"along the second of {on_path - 1} path edges", arrs, T, root, args.radius, lines)
    measure("the same tree, the root the start moved by (+0.10, +0.05) on the ground", arrs, T, near,
            args.radius, lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
