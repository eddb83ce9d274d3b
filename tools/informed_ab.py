"""A/B of informed sampling in a replan session, on one GPU, in one process.

From one state per map the search is continued with ReplanSession.informed off
and on, alternating, SEEDS seeds each, --seconds per run, the tree limit on in
both arms:

  config 5   synth-fractal-4096, 4096 draws per half, after the first group
             that ends with a held connection
  session    the session tests' search: synth-rough-256, batch 1,024, seed 11,
             after 200 halves

A run begins again from the dumped trees and list (a warm start with the run's
seed) and calls search in groups of GROUP halves, reading after each: the
half count, the best cost, the targets so far, the last half's star_pairs and
the capacity of the neighbour-pair sets (every GBP_PLAN_HALT_STAR_PAIRS doubles
it).  Reported per run: halves/s (what losing the look-ahead search costs),
targets per half, star_pairs per half (mean and largest of the groups' last
halves), the pair sets' growths, the best cost at the end and at the half count
every run of the map reached.

    python tools/informed_ab.py --out profiles/informed_ab.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from global_body_planner_amd import engine, planner  # noqa: E402
from global_body_planner_amd import terrain_data as td  # noqa: E402

SEEDS = (101, 202, 303)
GROUP = 64


def state_of(s):
    pairs, _, cost = s.shared_connections()
    return dict(trees=s.dump(), pairs=pairs, cost=cost, half=s.half, ext=s.status["ext_counter"])


def run(T, st0, start, goal, batch, seed, limit, informed, seconds):
    s = planner.ReplanSession(T)
    s.tree_limit = limit
    s.informed = informed
    s.begin(start, goal, batch=batch, seed=seed, init_trees=st0["trees"], first_half=st0["half"],
            extend_base=st0["ext"], init_shared=st0["pairs"])
    h0, t_base = s.half, s.status["stat_targets"]
    cap0 = s.pairs_cap
    trace, pairs, grows = [], [], []
    area = []
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        cap = s.pairs_cap
        s.search(1e9, GROUP)
        if s.pairs_cap != cap:
            grows.append(s.pairs_cap)
        trace.append((s.half - h0, s.status["best_cost"]))
        pairs.append(s.status["star_pairs"])
        e = s.informed_state
        area.append(3.14159 * e.a * e.b if e.active else float("nan"))
    dt = time.perf_counter() - t0
    out = dict(informed=informed, seed=seed, halves=s.half - h0, rate=(s.half - h0) / dt,
               targets_per_half=(s.status["stat_targets"] - t_base) / max(s.half - h0, 1),
               pairs_mean=statistics.mean(pairs), pairs_max=max(pairs), cap0=cap0, grows=grows,
               cost=s.status["best_cost"], trace=trace, known=list(s.known),
               trims=s.trims_by_search, area=area[-1])
    s.end()
    return out


def cost_at(trace, halves):
    best = float("inf")
    for h, c in trace:
        if h <= halves:
            best = c
    return best


def ab(name, T, st0, start, goal, batch, limit, seconds, lines):
    lines.append(f"{name}: from {st0['half']} halves, trees of {len(st0['trees'][0]['parent'])} + "
                 f"{len(st0['trees'][1]['parent'])} vertices, {len(st0['pairs'])} kept connections, "
                 f"best cost {st0['cost']!r}; tree limit {limit}, {seconds:g} s per run")
    runs = []
    for seed in SEEDS:
        for informed in (False, True):
            runs.append(run(T, st0, start, goal, batch, seed, limit, informed, seconds))
    common = min(r["halves"] for r in runs)
    for r in runs:
        lines.append(
            f"  {'informed' if r['informed'] else 'plain   '} seed {r['seed']}: {r['halves']:6d} halves, "
            f"{r['rate']:8.1f} halves/s, {r['targets_per_half']:7.1f} targets/half, star_pairs/half mean "
            f"{r['pairs_mean']:9.1f} max {r['pairs_max']:7d}, pair sets {r['cap0']}"
            f"{''.join(' -> ' + str(g) for g in r['grows'])}, best cost {r['cost']:.4f} "
            f"(at {common} halves {cost_at(r['trace'], common):.4f}), trees {r['known'][0]} + "
            f"{r['known'][1]}, {r['trims']} trims, ellipse {r['area']:.1f} m^2")
        print(lines[-1], flush=True)
    for informed in (False, True):
        rs = [r for r in runs if r["informed"] == informed]
        lines.append(
            f"  medians {'informed' if informed else 'plain   '}: "
            f"{statistics.median(r['rate'] for r in rs):8.1f} halves/s, "
            f"{statistics.median(r['targets_per_half'] for r in rs):7.1f} targets/half, star_pairs/half "
            f"{statistics.median(r['pairs_mean'] for r in rs):9.1f}, best cost "
            f"{statistics.median(r['cost'] for r in rs):.4f}, at {common} halves "
            f"{statistics.median(cost_at(r['trace'], common) for r in rs):.4f}, "
            f"{sum(len(r['grows']) for r in rs)} growths of the pair sets")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "informed_ab.txt"))
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--maps", default="session,config5")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("informed_ab.py measures on the GPU: no device found")
    lines = [f"informed sampling in a replan session, {torch.cuda.get_device_name(0)}; arms alternate, "
             f"seeds {SEEDS}, groups of {GROUP} halves"]
    if "session" in args.maps:
        from tests import prune_ref as R
        from tests import trim_ref as TR
        data, _ = R.terrain(None)
        start, goal = R.start_goal()
        T = engine.Terrain.from_data(data, device=0)
        s = planner.ReplanSession(T).begin(start, goal, batch=TR.SESSION["batch"], seed=TR.SESSION["seed"])
        s.search(1e9, TR.SESSION_HALVES)
        st0 = state_of(s)
        s.end()
        ab("session (synth-rough-256, batch 1024)", T, st0, start, goal, TR.SESSION["batch"],
           (8192, 4096), args.seconds, lines)
    if "config5" in args.maps:
        from tools.config5 import first_valid
        data = td.by_name("synth-fractal-4096")
        T = engine.Terrain.from_data(data, device=0)
        mid = data.x[-1] / 2
        start, goal = first_valid(T, 1.0, mid, 0.02), first_valid(T, 9.0, mid, -0.02)
        s = planner.ReplanSession(T).begin(start, goal, batch=4096, seed=20251020)
        t0 = time.perf_counter()
        while not s.search(1e9, GROUP) and s.half < 60000:
            pass
        lines.append(f"config 5: first held connection after {s.half} halves, {time.perf_counter() - t0:.1f} s")
        st0 = state_of(s)
        s.end()
        ab("config 5 (synth-fractal-4096, batch 4096)", T, st0, start, goal, 4096, (65536, 32768),
           args.seconds, lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
