"""A/B of updating a terrain handle in place against creating a new one, on one
GPU, in one process.

  (a) the whole map through gbp_terrain_update_host against gbp_terrain_create
      + gbp_terrain_destroy of the same arrays (heights and slope layers; then
      heights alone against a create without slope layers)
  (b) a 64 x 64 rectangle through gbp_terrain_update_host and through
      gbp_terrain_update_dev (enqueue + stream synchronise), against (a)'s
      create + destroy
  (c) the device entry's launches alone, whole map, by device events: source
      layout 0 (fp64 x-major: the round-trip check launch and the apply launch),
      layout 0 on an fp64-storage handle (the apply launch alone, 16-byte
      stores), layout 1 (a float grid_map layer through the LDS tile), each
      beside a device-to-device copy (torch copy_ of one contiguous buffer) of
      the bytes the patch kernel writes, 2 sizeof(ZT) (nx - 1) ny, as a ratio

The forms of a group alternate, REPS times each after a warm-up round; host
clock around calls that end synchronised, device events for (c).

    python tools/terrain_update_ab.py --out profiles/terrain_update_ab.txt
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
from global_body_planner_amd import engine  # noqa: E402
from global_body_planner_amd import terrain_data as td  # noqa: E402

REPS = 6


def ms(xs):
    return (f"median {1e3 * statistics.median(xs):10.3f} ms  min {1e3 * min(xs):10.3f}  "
            f"max {1e3 * max(xs):10.3f}")


def alternate(forms):
    """forms: name -> callable returning seconds; one warm-up round, then REPS
    rounds, the forms of a round one after the other."""
    out = {k: [] for k in forms}
    for rep in range(REPS + 1):
        for k, f in forms.items():
            t = f()
            if rep:
                out[k].append(t)
    return out


def host_clock(f):
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    return run


def events(f):
    def run():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3
    return run


def gridmap_layer(z):
    return np.ascontiguousarray(z[::-1, ::-1].T.astype(np.float32))


def measure(name, lines):
    data = td.by_name(name)
    nx, ny = data.z.shape
    lay = (data.dx, data.dy, data.dz)
    z2 = (data.z + np.float32(0.25)).astype(np.float32).astype(np.float64)
    T = engine.Terrain.from_data(data)
    N = engine.Terrain(data.x, data.y, data.z)
    f32 = T.info()["storage"] == L.STORAGE_F32
    lines.append(f"{name}: {nx} x {ny}, storage {'fp32' if f32 else 'fp64'}")

    def create_destroy(layers):
        def run():
            engine.Terrain(data.x, data.y, z2, *(lay if layers else ())).close()
        return run

    # (a) whole map
    a = alternate({
        "create+destroy, heights + slope layers": host_clock(create_destroy(True)),
        "update_host,    heights + slope layers": host_clock(
            lambda: T.update(z2, dx=lay[0], dy=lay[1], dz=lay[2])),
        "create+destroy, heights alone": host_clock(create_destroy(False)),
        "update_host,    heights alone": host_clock(lambda: N.update(z2)),
    })
    lines.append("  (a) whole map")
    for k, v in a.items():
        lines.append(f"      {k:42s} {ms(v)}")
    keys = list(a)
    for c, u in ((keys[0], keys[1]), (keys[2], keys[3])):
        lines.append(f"      create+destroy / update_host of medians ({c.split(', ')[1]}): "
                     f"{statistics.median(a[c]) / statistics.median(a[u]):.2f}x")

    # (b) a 64 x 64 rectangle
    ix0, iy0 = nx // 2 - 32, ny // 2 - 32
    patch = np.ascontiguousarray(z2[ix0:ix0 + 64, iy0:iy0 + 64])
    dpatch = torch.from_numpy(patch).cuda()
    b = alternate({
        "update_host 64 x 64": host_clock(lambda: T.update(patch, ix0, iy0)),
        "update_dev  64 x 64 (enqueue + synchronise)": host_clock(lambda: T.update(dpatch, ix0, iy0)),
    })
    lines.append("  (b) a 64 x 64 rectangle")
    ref = statistics.median(a[keys[0]])
    for k, v in b.items():
        lines.append(f"      {k:42s} {ms(v)}   create+destroy / this of medians "
                     f"{ref / statistics.median(v):.0f}x")

    # (c) the device entry's launches alone
    D = engine.Terrain(data.x, data.y, data.z, storage=L.STORAGE_F64)
    dz = torch.from_numpy(z2).cuda()
    dg = torch.from_numpy(gridmap_layer(z2)).cuda()
    lines.append("  (c) the device entry's launches, whole map, device events")
    for label, handle, src, layout, zt in (
            ("layout 0, fp32 handle (check + apply)", T, dz, L.SRC_F64_XMAJOR, 4),
            ("layout 0, fp64 handle (apply)", D, dz, L.SRC_F64_XMAJOR, 8),
            ("layout 1, fp32 handle (apply, LDS tile)", T, dg, L.SRC_F32_GRIDMAP, 4)):
        if handle is T and not f32:
            continue
        written = 2 * zt * (nx - 1) * ny
        buf_a = torch.empty(written, dtype=torch.uint8, device="cuda")
        buf_b = torch.empty_like(buf_a)
        c = alternate({
            "patch": events(lambda: handle.update(src, layout=layout)),
            "copy": events(lambda: buf_b.copy_(buf_a)),
        })
        mp, mc = statistics.median(c["patch"]), statistics.median(c["copy"])
        lines.append(f"      {label:42s} {ms(c['patch'])}")
        lines.append(f"      {'device-to-device copy of ' + str(written >> 20) + ' MiB':42s} "
                     f"{ms(c['copy'])}   patch / copy of medians {mp / mc:.2f}x, "
                     f"{written / mp / 1e9:.0f} GB/s written")
        del buf_a, buf_b
    for h in (T, N, D):
        h.close()
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terrain_update_ab.txt"))
    ap.add_argument("--terrains", nargs="+", default=["synth-rough-1024", "synth-fractal-4096"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("terrain_update_ab.py measures on the GPU: no device found")
    lines = [f"updating a terrain handle in place against creating a new one, "
             f"{torch.cuda.get_device_name(0)}, {REPS} alternating repetitions of each form "
             f"after a warm-up"]
    for name in args.terrains:
        block = []
        measure(name, block)
        lines += block
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
