"""What deriving a terrain's slope layers on the device costs, on one GPU, in one
process.

  (a) the whole-map launch of gbp_terrain_derive_slopes_dev by device events,
      beside a device-to-device copy (torch copy_ of one contiguous buffer) of
      the bytes it writes, 24 B per node, as a ratio
  (b) a whole-map update, host clock, three forms: gbp_terrain_update_host with
      heights alone followed by gbp_terrain_derive_slopes_host; update_host with
      heights and three host layers; and the numpy derivation those host layers
      cost (terrain_data.synth_fractal's recipe)
  (c) a 64 x 64 gbp_terrain_update_host with GBP_OPT_DERIVE_SLOPES on, beside
      the same update with it off
  (d) gbp_terrain_move_host by 8 cells with the option on, beside the same move
      with it off

The forms of a group alternate, REPS times each after a warm-up round; host
clock around calls that end synchronised, device events for (a).

    python tools/slopes_ab.py --out profiles/slopes_ab.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from global_body_planner_amd import _lib as L  # noqa: E402
from global_body_planner_amd import engine  # noqa: E402
from global_body_planner_amd import terrain_data as td  # noqa: E402
from tools.terrain_update_ab import REPS, alternate, events, host_clock, ms  # noqa: E402


def numpy_layers(z, spacing):
    gx = np.gradient(z, spacing, axis=0)
    gy = np.gradient(z, spacing, axis=1)
    nrm = np.stack([-gx, -gy, np.ones_like(z)])
    nrm /= np.linalg.norm(nrm, axis=0)
    return [np.ascontiguousarray(a.astype(np.float32).astype(np.float64)) for a in nrm]


def measure(name, lines):
    data = td.by_name(name)
    nx, ny = data.z.shape
    h = float(data.x[1] - data.x[0])
    z2 = (data.z + np.float32(0.25)).astype(np.float32).astype(np.float64)
    lay = numpy_layers(z2, h)
    T = engine.Terrain.from_data(data)   # layers, option off
    D = engine.Terrain.from_data(data)   # layers, option on
    D.set_option(L.OPT_DERIVE_SLOPES, 1 | L.SLOPES_F32)
    f32 = T.info()["storage"] == L.STORAGE_F32
    lines.append(f"{name}: {nx} x {ny}, storage {'fp32' if f32 else 'fp64'}")

    # (a) the launch alone
    written = 24 * nx * ny
    buf_a = torch.empty(written, dtype=torch.uint8, device="cuda")
    buf_b = torch.empty_like(buf_a)
    stream = torch.cuda.current_stream(0)
    a = alternate({
        "derive": events(lambda: T.derive_slopes(round_f32=True, stream=stream)),
        "copy": events(lambda: buf_b.copy_(buf_a)),
    })
    md, mc = statistics.median(a["derive"]), statistics.median(a["copy"])
    lines.append("  (a) derive_slopes_dev, whole map, device events")
    lines.append(f"      {'derive launch':42s} {ms(a['derive'])}")
    lines.append(f"      {'device-to-device copy of ' + str(written >> 20) + ' MiB':42s} {ms(a['copy'])}"
                 f"   derive / copy of medians {md / mc:.2f}x, {written / md / 1e9:.0f} GB/s written")
    del buf_a, buf_b

    # (b) a whole-map update that ends with layers of the new heights
    def update_then_derive():
        T.update(z2)
        T.derive_slopes(round_f32=True)
    b = alternate({
        "update_host heights + derive_slopes_host": host_clock(update_then_derive),
        "update_host heights + three host layers": host_clock(
            lambda: T.update(z2, dx=lay[0], dy=lay[1], dz=lay[2])),
        "numpy derivation of the three host layers": host_clock(lambda: numpy_layers(z2, h)),
    })
    lines.append("  (b) whole-map update, host clock")
    for k, v in b.items():
        lines.append(f"      {k:42s} {ms(v)}")

    # (c) a 64 x 64 update, option on / off
    ix0, iy0 = nx // 2 - 32, ny // 2 - 32
    patch = np.ascontiguousarray(z2[ix0:ix0 + 64, iy0:iy0 + 64])
    c = alternate({
        "update_host 64 x 64, option on": host_clock(lambda: D.update(patch, ix0, iy0)),
        "update_host 64 x 64, option off": host_clock(lambda: T.update(patch, ix0, iy0)),
    })
    lines.append("  (c) a 64 x 64 rectangle, host clock")
    for k, v in c.items():
        lines.append(f"      {k:42s} {ms(v)}")

    # (d) a move by 8 cells (there and back), option on / off
    maps = [(data.x, z2), (data.x + 8 * h, np.ascontiguousarray(np.roll(z2, -8, axis=0)))]
    at = {id(T): 0, id(D): 0}

    def mover(H):
        def run():
            k = at[id(H)] ^ 1
            H.move(8 if k else -8, 0, maps[k][0], data.y, maps[k][1])
            at[id(H)] = k
        return run
    d = alternate({
        "move_host by 8 cells, option on": host_clock(mover(D)),
        "move_host by 8 cells, option off": host_clock(mover(T)),
    })
    lines.append("  (d) a move by 8 cells, host clock")
    for k, v in d.items():
        lines.append(f"      {k:42s} {ms(v)}")
    for H in (T, D):
        H.close()
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slopes_ab.txt"))
    ap.add_argument("--terrains", nargs="+", default=["synth-rough-1024", "synth-fractal-4096"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slopes_ab.py measures on the GPU: no device found")
    lines = [f"deriving a terrain's slope layers on the device, {torch.cuda.get_device_name(0)}, "
             f"{REPS} alternating repetitions of each form after a warm-up"]
    for name in args.terrains:
        block = []
        measure(name, block)
        lines += block
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
