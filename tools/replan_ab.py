"""A/B of replanning after a map change, on one GPU, in one process.

A  the session (planner.ReplanSession, the sequence the C++ class runs): the
   terrain's strip updated in place, map_changed (both trees pruned in HBM,
   the kept connections carried through the device remaps and ranked again),
   best_path (extracted on the device).
B  what a caller does without it, from the same state: the same in-place
   update, both trees dumped, planner.revalidate_trees (load, prune, read
   back), the list remapped and ranked in numpy, the path joined on the host
   from the survivors; then, timed on its own as the cost of resuming, the
   warm start's gbp_tree_load_host of both survivors.

The state: config 5's search (synth-fractal-4096, 4096 draws per half) after
--grow-halves half-iterations; the changed map raises a 1 m wide strip across
tree a by 0.5 m.  Before every timed form the strip is put back and the
session begins again from the same dumped trees and list (not timed).  The
forms alternate, REPS times each after a warm-up round that also compares
their trees, lists, best and paths.  Then the path alone, on the unchanged
state: gbp_tree_path_host against reading both trees and joining on the host.

    python tools/replan_ab.py --out profiles/replan_ab.txt
"""
import argparse
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
from tests import shared_ref as SR  # noqa: E402

REPS = 6
BATCH, SEED = 4096, 20251020


def ms(xs):
    return (f"median {1e3 * statistics.median(xs):9.3f} ms  min {1e3 * min(xs):9.3f}  "
            f"max {1e3 * max(xs):9.3f}")


def rank_numpy(pairs, ga, gb):
    if not len(pairs):
        return -1, -1, np.inf
    c = ga[pairs[:, 0]] + gb[pairs[:, 1]]
    if np.all(np.isnan(c)):
        return -1, -1, np.inf
    k = int(np.nanargmin(c))   # the first of the cheapest
    return int(pairs[k, 0]), int(pairs[k, 1]), float(c[k])


def form_a(T, s, patch, ix0):
    T.update(patch, ix0, 0)
    pruned, shared = s.map_changed()
    return pruned, shared, s.best_path()


def form_b(T, s, patch, ix0, pairs):
    T.update(patch, ix0, 0)
    trees = s.dump()
    kept, remaps, stats = planner.revalidate_trees(T, trees)
    pairs2, shared = SR.remap_pairs(pairs, remaps[0], remaps[1])
    best = rank_numpy(pairs2, kept[0]["g"], kept[1]["g"])
    path = SR.join(kept[0], best[0], kept[1], best[1]) if best[0] >= 0 else None
    return kept, pairs2, best, path


def resume_b(kept):
    """the warm start's loads of the two survivors (gbp_tree_load_host, one lane each)"""
    out = []
    for t in kept:
        dt = engine.DeviceTree(t["v"][0], capacity=max(len(t["parent"]), 1))
        dt.load(t["v"], t["act"], t["parent"])
        out.append(dt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replan_ab.txt"))
    ap.add_argument("--grow-halves", type=int, default=21000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("replan_ab.py measures on the GPU: no device found")
    from tools.config5 import first_valid
    data = td.by_name("synth-fractal-4096")
    T = engine.Terrain.from_data(data, device=0, storage=L.STORAGE_F64)  # the strip's heights are not floats
    mid = data.x[-1] / 2
    start, goal = first_valid(T, 1.0, mid, 0.02), first_valid(T, 9.0, mid, -0.02)
    s = planner.ReplanSession(T)
    t0 = time.perf_counter()
    s.begin(start, goal, batch=BATCH, seed=SEED)
    s.search(3600.0, args.grow_halves)
    grow = time.perf_counter() - t0
    trees0 = s.dump()
    pairs0, best0, cost0 = s.shared_connections()
    half0, ext0 = s.half, s.status["ext_counter"]
    xm = float(np.median(trees0[0]["v"][:, 0]))
    rows = np.flatnonzero((data.x >= xm - 0.5) & (data.x <= xm + 0.5))
    ix0 = int(rows[0])
    z0 = np.ascontiguousarray(np.asarray(data.z, np.float64)[rows[0]:rows[-1] + 1, :])
    patch = z0 + 0.5
    lines = [f"replanning after a map change, {torch.cuda.get_device_name(0)}, {REPS} alternating "
             f"repetitions of each form after a warm-up",
             f"state: config 5 (synth-fractal-4096, batch {BATCH}, seed {SEED}) after {s.half} halves "
             f"({grow:.1f} s): trees of {len(trees0[0]['parent'])} + {len(trees0[1]['parent'])} "
             f"vertices, {len(pairs0)} kept connections, best cost {cost0!r}",
             f"changed map: +0.5 m on x in [{xm - 0.5:.2f}, {xm + 0.5:.2f}] ({len(rows)} rows of {data.z.shape[1]})"]

    def restore():
        T.update(z0, ix0, 0)
        s.begin(start, goal, batch=BATCH, seed=SEED, init_trees=trees0, first_half=half0,
                extend_base=ext0, init_shared=pairs0)

    ta, tb, tr = [], [], []
    info = None
    for rep in range(REPS + 1):
        restore()
        t0 = time.perf_counter()
        pruned, shared, path_a = form_a(T, s, patch, ix0)
        da = time.perf_counter() - t0
        if rep == 0:
            got_trees, (got_pairs, got_best, got_cost) = s.dump(), s.shared_connections()
        restore()
        t0 = time.perf_counter()
        kept, pairs_b, best_b, path_b = form_b(T, s, patch, ix0, pairs0)
        db = time.perf_counter() - t0
        t0 = time.perf_counter()
        loaded = resume_b(kept)
        torch.cuda.synchronize()
        dr = time.perf_counter() - t0
        del loaded
        if rep == 0:   # the two forms agree, bit for bit
            for x, y in zip(got_trees, kept):
                for key in ("v", "act", "parent", "g"):
                    assert np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes(), key
            assert np.array_equal(got_pairs, pairs_b) and got_best == best_b[:2]
            assert got_cost == best_b[2] or (got_best[0] < 0 and best_b[0] < 0)
            if path_a is not None:
                assert path_a["states"].tobytes() == path_b[0].tobytes()
                assert path_a["actions"].tobytes() == path_b[1].tobytes()
            info = (pruned, shared, path_a)
            continue
        ta.append(da)
        tb.append(db)
        tr.append(dr)
    pruned, shared, path_a = info
    lines += [f"after it: trees {pruned[0]['n_before']} -> {pruned[0]['n_kept']} and "
              f"{pruned[1]['n_before']} -> {pruned[1]['n_kept']}; connections {shared['n_before']} -> "
              f"{shared['n_kept']} ({shared['n_dropped_a']} lost with a, {shared['n_dropped_b']} with b "
              f"alone); best path of {0 if path_a is None else len(path_a['states'])} states",
              f"  A update, map_changed, best_path (session)             {ms(ta)}",
              f"  B update, dump, revalidate_trees, numpy list, host join {ms(tb)}   "
              f"B / A of medians {statistics.median(tb) / statistics.median(ta):.2f}x",
              f"  B's resume: gbp_tree_load_host of both survivors        {ms(tr)}"]
    # the path alone, on the unchanged state
    restore()
    tp, tj = [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        p = s.ws.tree_path(s.trees[0], s.trees[1])
        dp = time.perf_counter() - t0
        t0 = time.perf_counter()
        a, b = s.dump()
        j = SR.join(a, s.status["best_a"], b, s.status["best_b"])
        dj = time.perf_counter() - t0
        if rep == 0:
            assert p[0].tobytes() == j[0].tobytes() and p[1].tobytes() == j[1].tobytes()
            continue
        tp.append(dp)
        tj.append(dj)
    lines += [f"the best path alone ({len(j[0])} states: {j[3]} from a, {j[4]} from b), unchanged state:",
              f"  gbp_tree_path_host                                      {ms(tp)}",
              f"  read both trees, join on the host                       {ms(tj)}   "
              f"ratio of medians {statistics.median(tj) / statistics.median(tp):.1f}x"]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
