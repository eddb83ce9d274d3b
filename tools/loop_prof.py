"""Where a persistent validate wave spends its cycles (diagnostic build):

    make -C global_body_planner_amd/csrc variant NAME=lp DEFS=-DGBP_LOOP_PROF
    python tools/loop_prof.py ab_libs/libgbp_lp.so

The -DGBP_LOOP_PROF build of k_validate_persistent reads the shader clock
(s_memtime) between the phases of each loop step and accumulates per wave:
refill, the helper plan, sample + isValidState, transition + the helpers'
consumption, outputs + s_new ring; plus the whole loop, tail steps and steps.
Config 3 (synth-rough-1024, 262,144 attempts) and config 2 (synth-rough-256,
65,536), one launch each after a warm-up launch; with --fresh-batches N the
profiled launch is the last of 2 N that cycle N distinct resident batches
(bench.py's inputs: no launch replays cache-warm rows).

From the waves' wall-clock stamps (entry, first sample, end) it also reports
what a launch's hand-over to the next one leaves on the table: per workgroup,
the time each ended wave's slot stands empty until the workgroup's last wave
ends and its LDS is released (`slot_wait_us`: mean per wave, total slot-us per
launch, and the same split by workgroup size), and the time from the kernel's
start (its first wave's entry) and from each wave's own entry to that wave's
first sample (`start_to_first_sample_us`, `entry_to_first_sample_us`: the
coordinate staging and the first fill).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import global_body_planner_amd as gbp  # noqa: E402
from global_body_planner_amd import _lib as L  # noqa: E402
from global_body_planner_amd import terrain_data as td  # noqa: E402
from global_body_planner_amd import workload as W  # noqa: E402

PHASES = ["refill", "helper_plan", "sample_isvalid", "transition_consume", "outputs_ring"]
LP_N = 14   # values per wave (gbp_engine.hip gbp_loop_prof)


def handover(raw, block):
    """The hand-over figures of one launch from the per-wave stamps (100 MHz ticks):
    raw[:, 9] end, raw[:, 12] entry, raw[:, 13] first sample; row = workgroup * nwv + wave."""
    nwv = max(1, block // 64)
    a = raw.astype(np.float64)
    ran = a[:, 12] > 0                       # (a wave with an empty slice still enters and ends)
    wg = np.arange(a.shape[0]) // nwv
    end, entry = a[:, 9] * 1e-2, a[:, 12] * 1e-2   # us
    wait = np.zeros(a.shape[0])
    for g in np.unique(wg[ran]):
        m = ran & (wg == g)
        wait[m] = end[m].max() - end[m]
    w = wait[ran]
    t0 = entry[ran].min()
    first = a[:, 13] * 1e-2
    stepped = ran & (a[:, 13] > 0)
    q = (50, 90, 100)
    return {"block": int(block), "waves_per_workgroup": nwv, "workgroups": int(np.unique(wg[ran]).size),
            "slot_wait_us": {"mean_per_wave": float(w.mean()), "total_per_launch": float(w.sum()),
                             "max": float(w.max())},
            "entry_skew_us": float(entry[ran].max() - t0),
            "start_to_first_sample_us": {str(k): float(np.percentile(first[stepped] - t0, k)) for k in q},
            "entry_to_first_sample_us": {"mean": float((first[stepped] - entry[stepped]).mean()),
                                         **{str(k): float(np.percentile(first[stepped] - entry[stepped], k))
                                            for k in q}},
            "kernel_us": float(end[ran].max() - t0)}


def run(lib, terrain, batch, seed, opts=(), waves=2048, fresh=1):
    data = td.by_name(terrain)
    T = gbp.Terrain.from_data(data, device=0, lib=lib)
    for kv in opts:
        k, v = kv.split("=")
        T.set_option(getattr(L, "OPT_" + k), int(v))
    s, act, d, _, _ = W.make_attempts(T, batch, seed)
    out = T.validate_pairs(s, act, d)
    if fresh > 1:
        # bench.py's fresh-batch protocol: distinct resident batches cycled, so the
        # profiled launch (the last one) reads rows no earlier launch left in cache
        ins = [(s, act, d)] + [W.make_attempts(T, batch, seed, index_base=k * batch)[:3]
                               for k in range(1, fresh)]
        for k in range(2 * fresh):
            T.validate_pairs(*ins[k % fresh], out=out)
    else:
        T.validate_pairs(s, act, d, out=out)
    torch.cuda.synchronize()
    buf = (ctypes.c_ulonglong * (LP_N * waves))()
    rc = lib.gbp_loop_prof_read(buf, ctypes.c_int(waves))
    assert rc == 0, rc
    raw = np.frombuffer(buf, dtype=np.uint64).reshape(waves, LP_N)
    hand = handover(raw, T.get_option(L.OPT_LAUNCH_BLOCK))
    a = raw.astype(np.float64)
    keep = a[:, 7] > 0
    a, raw = a[keep], raw[keep]
    if os.environ.get("LOOP_PROF_DUMP"):
        np.save(os.environ["LOOP_PROF_DUMP"] + f"_{terrain}.npy", raw)
    steps = a[:, 7].sum()
    tot = a[:, 5].sum()
    row = {"terrain": terrain, "batch": batch, "waves": int(a.shape[0]),
           "steps_per_wave": float(a[:, 7].mean()), "tail_steps_per_wave": float(a[:, 6].mean()),
           "loop_cycles_per_wave": float(a[:, 5].mean()),
           "loop_cycles_per_wave_max": float(a[:, 5].max()),
           "cycles_per_step": float(tot / steps)}
    for k, nm in enumerate(PHASES):
        row[nm + "_frac"] = float(a[:, k].sum() / tot)
        row[nm + "_per_step"] = float(a[:, k].sum() / steps)
    # a tail step refills nothing: the refill's cycles fall on the steps before the tail
    row["refill_per_refilling_step"] = float(a[:, 0].sum() / max(1.0, (a[:, 7] - a[:, 6]).sum()))
    row["inputs"] = f"fresh: {fresh} batches cycled" if fresh > 1 else "one batch replayed"
    # wall clock (s_memrealtime, 100 MHz): start skew, per-wave spans, the end
    t0, t1 = a[:, 8], a[:, 9]
    span = (t1 - t0) * 10.0  # ns
    row["start_skew_us"] = float((t0.max() - t0.min()) * 10.0 / 1e3)
    row["kernel_span_us"] = float((t1.max() - t0.min()) * 10.0 / 1e3)
    row["wave_span_us"] = {q: float(np.percentile(span, q) / 1e3) for q in (0, 10, 50, 90, 99, 100)}
    row["steps_quantiles"] = {q: float(np.percentile(a[:, 7], q)) for q in (0, 50, 90, 99, 100)}
    row["corr_span_steps"] = float(np.corrcoef(span, a[:, 7])[0, 1])
    # the slowest decile: its steps and its cycles per step against the rest
    slow = span >= np.percentile(span, 90)
    row["slow_decile"] = {"steps": float(a[slow, 7].mean()), "rest_steps": float(a[~slow, 7].mean()),
                          "cycles_per_step": float(a[slow, 5].sum() / a[slow, 7].sum()),
                          "rest_cycles_per_step": float(a[~slow, 5].sum() / a[~slow, 7].sum())}
    # per XCC and per CU: mean span (contention differences)
    xcc = raw[:, 11] & 0xF
    cu = (raw[:, 10] >> 8) & 0x1FF
    row["span_by_xcc_us"] = [float(span[xcc == x].mean() / 1e3) for x in range(8) if (xcc == x).any()]
    cus = {}
    for x, c, sp in zip(xcc, cu, span):
        cus.setdefault((int(x), int(c)), []).append(sp)
    cm = np.array([np.mean(v) for v in cus.values()]) / 1e3
    row["cu_mean_span_us"] = {"n": len(cus), "min": float(cm.min()), "median": float(np.median(cm)),
                              "max": float(cm.max())}
    row["handover"] = hand
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("lib")
    p.add_argument("--set", action="append", default=[], help="OPT=value on the handle")
    p.add_argument("--fresh-batches", type=int, default=1,
                   help="cycle this many distinct resident batches (bench.py's protocol: 8)")
    a = p.parse_args()
    lib = L.load(a.lib)
    lib.gbp_loop_prof_read.argtypes = [ctypes.c_void_p, ctypes.c_int]
    for terrain, batch, seed in (("synth-rough-1024", 262144, W.CONFIG_SEEDS[3]),
                                 ("synth-rough-256", 65536, W.CONFIG_SEEDS[2])):
        print(json.dumps(run(lib, terrain, batch, seed, a.set, fresh=a.fresh_batches)), flush=True)


if __name__ == "__main__":
    main()
