"""A/B of bounding a replan session's trees, on one GPU, in one process.

A  the session's trim (planner.ReplanSession.trim, the sequence the C++ class
   runs): both trees trimmed in HBM (gbp_tree_trim_keep_host: f, the radix
   select, the flags, then gbp_tree_prune_dev), the kept connections carried
   through the device remaps and ranked again.
B  what a caller does without it, from the same state: both trees dumped, f,
   the cut (np.sort), the flags, the keep rule and the compaction in numpy, the
   list remapped in numpy, gbp_tree_load_host of both survivors and
   gbp_plan_shared_load_host of the list.

Two trims, each in both forms:
  bound   f > the held best cost goes (trim(0))
  budget  no bound, each tree cut to half its vertices (max_keep = n / 2 per
          tree: the engine's entries under the session's own carry, since
          ReplanSession.trim takes one budget for both trees and always applies
          the bound)

The state: config 5's search (synth-fractal-4096, 4096 draws per half) after
--grow-halves half-iterations.  Before every timed form the session begins
again from the same dumped trees and list (not timed).  The forms alternate,
REPS times each after a warm-up round that also compares their trees, lists
and best.  Then the search rate: --search-seconds of search continued from the
untrimmed, the bound-trimmed and the budget-trimmed state.

    python tools/tree_trim_ab.py --out profiles/tree_trim_ab.txt
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
from tests import trim_ref as TR  # noqa: E402
from tools.tree_prune_ab import numpy_prune  # noqa: E402

REPS = 6
BATCH, SEED = 4096, 20251020
INF = float("inf")


def ms(xs):
    return (f"median {1e3 * statistics.median(xs):9.3f} ms  min {1e3 * min(xs):9.3f}  "
            f"max {1e3 * max(xs):9.3f}")


def held(s):
    st = s.status
    if st["best_a"] < 0:
        return INF, (-1, -1)
    return st["best_cost"], (st["best_a"], st["best_b"])


def form_a(s, mode):
    """-> (trim stats of a and b, shared stats)"""
    if mode == "bound":
        return s.trim(0)
    _, protect = held(s)
    before = list(s.known)
    stats = []
    for k in range(2):
        buf = s._remap_buf(k, before[k])
        stats.append(s.trees[k].trim(s.trees[k ^ 1], INF, before[k] // 2, protect[k], remap_dev=buf)[1])
        s.known[k] = stats[k]["n_kept"]
    return tuple(stats), s._carry(s._remap[0], s._remap[1], before)


def form_b(s, mode, pairs):
    """-> (survivors, list, best): the trees in fresh DeviceTrees, the list loaded."""
    trees = s.dump()
    bound, protect = held(s)
    out, remaps = [], []
    for k in range(2):
        t = trees[k]
        n = len(t["parent"])
        keep = TR.flags(t, trees[k ^ 1]["v"][0], bound if mode == "bound" else INF,
                        0 if mode == "bound" else n // 2, protect[k])[0]
        v, a, p, remap = numpy_prune(t["v"], t["act"], t["parent"], keep)
        out.append(dict(v=v, act=a, parent=p, g=t["g"][remap >= 0]))
        remaps.append(remap)
    pairs2, _ = SR.remap_pairs(pairs, remaps[0], remaps[1])
    loaded = []
    for t in out:
        dt = engine.DeviceTree(t["v"][0], capacity=max(len(t["parent"]), 1))
        dt.load(t["v"], t["act"], t["parent"])
        loaded.append(dt)
    s.ws.shared_load(loaded[0], loaded[1], pairs2)
    st = s.ws.status()
    return out, pairs2, (st["best_a"], st["best_b"], st["best_cost"]), loaded


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_trim_ab.txt"))
    ap.add_argument("--grow-halves", type=int, default=21000)
    ap.add_argument("--search-seconds", type=float, default=5.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tree_trim_ab.py measures on the GPU: no device found")
    from tools.config5 import first_valid
    data = td.by_name("synth-fractal-4096")
    T = engine.Terrain.from_data(data, device=0)
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
    lines = [f"bounding a session's trees, {torch.cuda.get_device_name(0)}, {REPS} alternating repetitions "
             f"of each form after a warm-up",
             f"state: config 5 (synth-fractal-4096, batch {BATCH}, seed {SEED}) after {s.half} halves "
             f"({grow:.1f} s): trees of {len(trees0[0]['parent'])} + {len(trees0[1]['parent'])} "
             f"vertices, {len(pairs0)} kept connections, best cost {cost0!r}"]

    def restore():
        s.begin(start, goal, batch=BATCH, seed=SEED, init_trees=trees0, first_half=half0,
                extend_base=ext0, init_shared=pairs0)

    for mode in ("bound", "budget"):
        ta, tb = [], []
        info = None
        for rep in range(REPS + 1):
            restore()
            path0 = s.best_path()
            t0 = time.perf_counter()
            stats, shared = form_a(s, mode)
            da = time.perf_counter() - t0
            if rep == 0:
                got_trees, (got_pairs, got_best, got_cost) = s.dump(), s.shared_connections()
                path1 = s.best_path()
                assert path0["states"].tobytes() == path1["states"].tobytes()
                assert path0["actions"].tobytes() == path1["actions"].tobytes()
                assert got_cost == cost0
            restore()
            t0 = time.perf_counter()
            kept, pairs_b, best_b, loaded = form_b(s, mode, pairs0)
            torch.cuda.synchronize()
            db = time.perf_counter() - t0
            del loaded
            if rep == 0:   # the two forms agree, bit for bit
                for x, y in zip(got_trees, kept):
                    for key in ("v", "act", "parent", "g"):
                        assert np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes(), (mode, key)
                assert np.array_equal(got_pairs, pairs_b) and got_best == best_b[:2] and got_cost == best_b[2]
                info = (stats, shared)
                continue
            ta.append(da)
            tb.append(db)
        stats, shared = info
        what = ("bound (f > best cost)" if mode == "bound" else
                "budget (half of each tree, no bound)")
        lines += [f"{what}: trees {stats[0]['n_before']} -> {stats[0]['n_kept']} and "
                  f"{stats[1]['n_before']} -> {stats[1]['n_kept']} (over the bound {stats[0]['n_over_bound']} + "
                  f"{stats[1]['n_over_bound']}, over the budget {stats[0]['n_over_budget']} + "
                  f"{stats[1]['n_over_budget']}, protected {stats[0]['n_protected']} + "
                  f"{stats[1]['n_protected']}, through an ancestor {stats[0]['n_inherited']} + "
                  f"{stats[1]['n_inherited']}); connections {shared['n_before']} -> {shared['n_kept']}; "
                  f"best path and cost unchanged",
                  f"  A session trim (device)                                   {ms(ta)}",
                  f"  B dump, numpy, gbp_tree_load_host, gbp_plan_shared_load_host {ms(tb)}   "
                  f"B / A of medians {statistics.median(tb) / statistics.median(ta):.2f}x"]
        print("\n".join(lines[-3:]), flush=True)
    # the search rate continued from each state
    lines.append(f"search continued for {args.search_seconds:g} s from each state:")
    for mode in ("untrimmed", "bound", "budget"):
        restore()
        if mode != "untrimmed":
            form_a(s, mode)
        n0, h0 = list(s.known), s.half
        t0 = time.perf_counter()
        s.search(args.search_seconds)
        dt = time.perf_counter() - t0
        lines.append(f"  {mode:10s} from {n0[0]:6d} + {n0[1]:6d} vertices: {s.half - h0:6d} halves in {dt:.2f} s "
                     f"= {(s.half - h0) / dt:8.1f} halves/s, to {s.known[0]} + {s.known[1]} vertices, "
                     f"best cost {s.status['best_cost']!r}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
