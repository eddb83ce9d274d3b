"""A/B of postProcessPath's two forms on one GPU, in one process.

host    the walk as RRTConnectClass::postProcessPath runs it: one
        attemptConnect per popped candidate, each an engine launch per
        recursion level and a synchronous read-back.  Driven here through
        gbp_attempt_connect_batch with n = 1 (the call attemptConnect makes),
        so that any path can be fed in; the calls are counted.
device  gbp_shortcut_paths_host (planner.shortcut_paths): staging, one table
        launch for all pairs, one read-back, host re-decisions, the walk.

Inputs: the found paths of the tests (tests/shortcut_cases.py FOUND) and the
densified 106- and 109-state paths (DENSE), plain step.  Both forms get the
same path and must keep the same states; only the post-processing is timed
(host clock around calls that end synchronised).  The forms alternate, REPS
times each after a warm-up of both.  Then, for the same inputs: the table
kernel alone from device events, in both item orders, alternating
(GBP_SHORTCUT_ORDER 0 / 1).  Last, end to end: plan_rrt_connect with
post_process 0 / 1 / 2 (total_time, the search included).

    python tools/shortcut_ab.py --out profiles/shortcut_ab.txt
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

from global_body_planner_amd import engine, planner  # noqa: E402
from tests import shortcut_cases as C  # noqa: E402

REPS = 6
FORWARD, REACHED = 0, 2


def host_walk(T, S):
    """postProcessPath's loop with its attemptConnect calls; -> (kept places, calls)."""
    n, cur, kept, calls = len(S), 0, [0], 0
    same = lambda i, j: np.array_equal(S[i], S[j])
    while not same(cur, n - 1):
        last, old = n - 1, -1
        while True:
            r, _, _ = planner.attempt_connect(T, S[cur], S[last], FORWARD)
            calls += 1
            if r[0] == REACHED or same(cur, last):
                break
            old, last = last, last - 1
        cur = last if not same(cur, last) else old
        kept.append(cur)
    return kept, calls


def ms(xs):
    return (f"median {1e3 * statistics.median(xs):9.3f} ms  min {1e3 * min(xs):9.3f}  "
            f"max {1e3 * max(xs):9.3f}")


def kernel_ms(T, paths):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    T.shortcut_table(paths)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shortcut_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shortcut_ab.py measures on the GPU: no device found")
    lines = [f"postProcessPath host form vs device form, {torch.cuda.get_device_name(0)}, "
             f"{REPS} alternating repetitions each (plain step)"]
    inputs = [(f"{c[0]} batch {b} seed {s} found", c[0], C.found_path(c, b, s)[0],
               C.found_path(c, b, s)[1]) for c, b, s in C.FOUND]
    inputs += [(f"{d[0][0]} seed {d[2]} densified k={d[3]}", d[0][0]) + C.dense_path(*d)
               for d in C.DENSE]
    terrains = {}
    for label, name, S, A in inputs:
        T = terrains.setdefault(name, engine.Terrain.from_data(C.terrain(name)[0], device=0))
        kept, calls = host_walk(T, S)           # warm-up of both forms, and the check
        out = planner.shortcut_paths(T, [S], [A])
        assert np.array_equal(out["states"][0], S[kept]), label
        th, tdv = [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            host_walk(T, S)
            th.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            planner.shortcut_paths(T, [S], [A])
            tdv.append(time.perf_counter() - t0)
        k0, k1 = [], []
        for _ in range(REPS):
            for order, acc in ((0, k0), (1, k1)):
                os.environ["GBP_SHORTCUT_ORDER"] = str(order)
                acc.append(kernel_ms(T, [S]))
        os.environ.pop("GBP_SHORTCUT_ORDER")
        n = len(S)
        lines += [f"{label}: {n} states -> {len(kept)}, {n * (n - 1) // 2} pairs, "
                  f"{out['n_resolved']} re-decided",
                  f"  host   {ms(th)}   {calls} attemptConnect calls",
                  f"  device {ms(tdv)}   speed-up of medians "
                  f"{statistics.median(th) / statistics.median(tdv):.2f}x",
                  f"  kernel, packed order        {ms(k0)}",
                  f"  kernel, longest spans first {ms(k1)}"]
        print("\n".join(lines[-5:]), flush=True)
    # every found path of a terrain in one call (what a batch of restarts would pass)
    for name in terrains:
        sel = [(S, A) for _, nm, S, A in inputs[:len(C.FOUND)] if nm == name]
        planner.shortcut_paths(terrains[name], [p[0] for p in sel], [p[1] for p in sel])
        tb = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            planner.shortcut_paths(terrains[name], [p[0] for p in sel], [p[1] for p in sel])
            tb.append(time.perf_counter() - t0)
        lines.append(f"{name}: its {len(sel)} found paths in one device call  {ms(tb)}")
        print(lines[-1], flush=True)
    lines.append("end to end, plan_rrt_connect algorithm 3 total_time (search + post-processing):")
    for case, batch, seed in ((C.SYNTH, 64, 11), (C.SLOPE, 256, 7)):
        data, O = C.terrain(case[0])
        start, goal = C.start_goal(O, *case[1])
        tt = {0: [], 1: [], 2: []}
        for rep in range(REPS + 1):
            for pp in (0, 1, 2):
                r = planner.plan_rrt_connect(data, start, goal, batch=batch, max_time=300.0,
                                             seed=seed, algorithm=3, post_process=pp)
                if rep:  # the first round warms up
                    tt[pp].append(r["total_time"])
        for pp in (0, 1, 2):
            lines.append(f"  {case[0]} batch {batch} seed {seed} post_process={pp}  {ms(tt[pp])}")
        print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
