// terrain_patch_probe.cpp — the engine-free part of an in-place terrain update
// (csrc/host/gbp_terrain_patch.cpp) on heap arrays of exactly the stated
// sizes, for AddressSanitizer / UBSan (tests/test_terrain_patch.py).
//
//   terrain_patch_probe NX NY storage < cases
//
// One case per line: ix0 iy0 nx ny layout ld n v_0 ... v_{n-1} (hex floats:
// the source array, n elements of double or float by the layout).  The mirror
// starts as m[ix][iy] = 100 + 10 ix + iy before every case.  Per case one
// output line: rc p0 p1 round_trips m_0 ... m_{NX NY - 1} (hex floats), where
// rc is check_patch's status and the mirror is scattered only when rc is 0,
// as gbp_terrain_update_host does.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "gbp_terrain_patch.h"

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const int NX = atoi(argv[1]), NY = atoi(argv[2]), storage = atoi(argv[3]);
  gbp_rect r;
  int layout;
  long long ld, n;
  while (scanf("%d %d %d %d %d %lld %lld", &r.ix0, &r.iy0, &r.nx, &r.ny, &layout, &ld, &n) == 7) {
    // exactly n elements on the heap: an index past the source is an ASan report
    std::unique_ptr<double[]> sd;
    std::unique_ptr<float[]> sf;
    const bool f32src = layout == GBP_SRC_F32_GRIDMAP;
    if (f32src)
      sf.reset(new float[n]);
    else
      sd.reset(new double[n]);
    for (long long i = 0; i < n; i++) {
      double v;
      if (scanf("%la", &v) != 1) return 3;
      if (f32src)
        sf[i] = (float)v;
      else
        sd[i] = v;
    }
    const void *src = f32src ? (const void *)sf.get() : (const void *)sd.get();
    std::unique_ptr<double[]> m(new double[(size_t)NX * NY]);
    for (int ix = 0; ix < NX; ix++)
      for (int iy = 0; iy < NY; iy++) m[(size_t)ix * NY + iy] = 100.0 + 10.0 * ix + iy;
    gbp_patch::Rect q;
    const int rc = gbp_patch::check_patch(NX, NY, storage, &r, layout, ld, src, &q);
    int p0 = -1, p1 = -1, rt = -1;
    gbp_patch::Rect qq;
    if (gbp_patch::resolve_rect(NX, NY, &r, &qq) == GBP_OK &&
        gbp_patch::check_source(layout, NX, qq, ld, src) == GBP_OK) {
      gbp_patch::pair_rows(NX, qq, &p0, &p1);
      rt = gbp_patch::round_trips(layout, NX, NY, qq, ld, src) ? 1 : 0;
    }
    if (rc == GBP_OK)
      gbp_patch::scatter(m.get(), NX, NY, q, layout, ld, src, storage == GBP_STORAGE_F32);
    printf("%d %d %d %d", rc, p0, p1, rt);
    for (int i = 0; i < NX * NY; i++) printf(" %a", m[i]);
    printf("\n");
  }
  return 0;
}
