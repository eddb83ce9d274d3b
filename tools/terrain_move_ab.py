"""A/B of moving a terrain handle's window by whole cells in place against
creating a new handle, on one GPU, in one process.

  (a) gbp_terrain_move_host by 8 cells along x, along y and along both (the
      whole new map given, heights and slope layers; only the strips are read)
      against what there was before for the same event: gbp_terrain_create +
      gbp_terrain_destroy of the moved arrays
  (b) the shift launch alone, by the device events gbp_terrain_move_host puts
      around it (gbp_terrain_move_shift_ms), beside a device-to-device copy
      (torch copy_ of one contiguous buffer) of the bytes it writes: the
      x-pairs, 2 sizeof(ZT) (nx - 1) ny, and the three slope layers, 24 nx ny
  (c) --session: the session's event on the state of tools/replan_ab.py (config
      5 after --grow-halves halves): move + map_changed + best_path against
      end + create + begin from the dumped trees and list (then map_changed +
      best_path there as well, timed apart)

The forms of a group alternate, REPS times each after a warm-up round that
compares them bit for bit; host clock around calls that end synchronised.
The new map of a move is the old one rolled by the shift, so the overlap holds
what it held and the strips hold the rows and columns that left on the other
side.

    python tools/terrain_move_ab.py --out profiles/terrain_move_ab.txt
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
RES = 0.02
BATCH, SEED = 4096, 20251020


def ms(xs):
    return (f"median {1e3 * statistics.median(xs):10.3f} ms  min {1e3 * min(xs):10.3f}  "
            f"max {1e3 * max(xs):10.3f}")


def clock(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def rolled(arrs, sx, sy):
    return [np.ascontiguousarray(np.roll(a, (-sx, -sy), axis=(0, 1))) for a in arrs]


def shift_ms(T):
    v = ctypes.c_float()
    L.check(T._lib.gbp_terrain_move_shift_ms(T._h, ctypes.byref(v)), "move_shift_ms")
    return v.value * 1e-3


def measure(name, lines):
    data = td.by_name(name)
    nx, ny = data.z.shape
    T = engine.Terrain.from_data(data)
    zt = 4 if T.info()["storage"] == L.STORAGE_F32 else 8
    lines.append(f"{name}: {nx} x {ny}, storage {'fp32' if zt == 4 else 'fp64'}")
    written = 2 * zt * (nx - 1) * ny + 24 * nx * ny
    buf_a = torch.empty(written, dtype=torch.uint8, device="cuda")
    buf_b = torch.empty_like(buf_a)
    cur = [data.z, data.dx, data.dy, data.dz]   # what T holds, move after move
    x, y = data.x, data.y
    for sx, sy in ((8, 0), (0, 8), (8, 8)):
        tm, tc, tk, tcp = [], [], [], []
        for rep in range(REPS + 1):
            new = rolled(cur, sx, sy)
            x, y = x + sx * RES, y + sy * RES
            dm, _ = clock(lambda: T.move(sx, sy, x, y, *new))
            dk = shift_ms(T)
            dc, F = clock(lambda: engine.Terrain(x, y, *new))
            if rep == 0:   # the two forms agree, bit for bit
                for copy in (0, 1):
                    assert T.read(copy=copy).tobytes() == F.read(copy=copy).tobytes()
                assert T.info() == F.info()
            dd, _ = clock(F.close)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            buf_b.copy_(buf_a)
            e1.record()
            e1.synchronize()
            cur = new
            if rep:
                tm.append(dm)
                tc.append(dc + dd)
                tk.append(dk)
                tcp.append(e0.elapsed_time(e1) * 1e-3)
        mk, mc = statistics.median(tk), statistics.median(tcp)
        lines += [f"  shift ({sx}, {sy})",
                  f"    (a) move_host                          {ms(tm)}",
                  f"        create + destroy                   {ms(tc)}   create+destroy / move of "
                  f"medians {statistics.median(tc) / statistics.median(tm):.2f}x",
                  f"    (b) shift launch (device events)       {ms(tk)}",
                  f"        device-to-device copy of {written >> 20:4d} MiB {ms(tcp)}   shift / copy of "
                  f"medians {mk / mc:.2f}x, {written / mk / 1e9:.0f} GB/s written"]
        print("\n".join(lines[-5:]), flush=True)
    T.close()


def session(lines, grow_halves):
    from tools.config5 import first_valid
    data = td.by_name("synth-fractal-4096")
    arrs0 = [data.z, data.dx, data.dy, data.dz]
    T = engine.Terrain.from_data(data, device=0)
    mid = data.x[-1] / 2
    start, goal = first_valid(T, 1.0, mid, 0.02), first_valid(T, 9.0, mid, -0.02)
    s = planner.ReplanSession(T)
    t0 = time.perf_counter()
    s.begin(start, goal, batch=BATCH, seed=SEED)
    s.search(3600.0, grow_halves)
    grow = time.perf_counter() - t0
    trees0 = s.dump()
    pairs0, best0, cost0 = s.shared_connections()
    half0, ext0 = s.half, s.status["ext_counter"]
    # 8 cells towards -x: what the trees hold in the map's last 8 rows leaves the window
    sx, sy = -8, 0
    x1, y1 = data.x + sx * RES, data.y + sy * RES
    new = rolled(arrs0, sx, sy)
    lines += [f"(c) the session's event, state: config 5 (synth-fractal-4096, batch {BATCH}, seed {SEED}) "
              f"after {s.half} halves ({grow:.1f} s): trees of {len(trees0[0]['parent'])} + "
              f"{len(trees0[1]['parent'])} vertices, {len(pairs0)} kept connections; window moved by "
              f"({sx}, {sy}) cells"]
    kw = dict(batch=BATCH, seed=SEED, init_trees=trees0, first_half=half0, extend_base=ext0,
              init_shared=pairs0)
    ta, tb, tb2 = [], [], []
    for rep in range(REPS + 1):
        # A: the handle and the session stay
        da, out_a = clock(lambda: (T.move(sx, sy, x1, y1, *new), s.map_changed(), s.best_path()))
        if rep == 0:
            got = s.dump()
        T.move(-sx, -sy, data.x, data.y, *arrs0)   # back (not timed)
        s.begin(start, goal, **kw)

        # B: what there was before: a new handle, a new session from the dumped state
        def form_b():
            s.end()
            T2 = engine.Terrain(x1, y1, *new)
            s2 = planner.ReplanSession(T2)
            s2.begin(start, goal, **kw)
            return T2, s2
        db, (T2, s2) = clock(form_b)
        db2, out_b = clock(lambda: (s2.map_changed(), s2.best_path()))
        if rep == 0:   # the two forms agree, bit for bit
            same = all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes()
                       for a, b in zip(got, s2.dump()) for key in ("v", "act", "parent", "g"))
            pa, pb = out_a[2], out_b[1]
            same = same and (pa is None) == (pb is None) and \
                (pa is None or pa["states"].tobytes() == pb["states"].tobytes())
            lines.append(f"    warm-up: trees and best path of A and B equal bit for bit: {same}")
            info = out_a[1]
        s2.end()
        T2.close()
        s.begin(start, goal, **kw)
        if rep:
            ta.append(da)
            tb.append(db)
            tb2.append(db2)
    pruned, shared = info
    lines += [f"    after it: trees {pruned[0]['n_before']} -> {pruned[0]['n_kept']} and "
              f"{pruned[1]['n_before']} -> {pruned[1]['n_kept']}; connections {shared['n_before']} -> "
              f"{shared['n_kept']}",
              f"    A move, map_changed, best_path (the session goes on)  {ms(ta)}",
              f"    B end, create, begin from the dumped trees and list   {ms(tb)}   "
              f"B / A of medians {statistics.median(tb) / statistics.median(ta):.2f}x",
              f"      then map_changed, best_path on the new session      {ms(tb2)}"]
    print("\n".join(lines[-5:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terrain_move_ab.txt"))
    ap.add_argument("--terrains", nargs="*", default=["synth-rough-1024", "synth-fractal-4096"])
    ap.add_argument("--session", action="store_true")
    ap.add_argument("--grow-halves", type=int, default=21000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("terrain_move_ab.py measures on the GPU: no device found")
    lines = [f"moving a terrain handle's window in place against creating a new handle, "
             f"{torch.cuda.get_device_name(0)}, {REPS} alternating repetitions of each form after a "
             f"warm-up"]
    for name in args.terrains:
        measure(name, lines)
    if args.session:
        session(lines, args.grow_halves)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
