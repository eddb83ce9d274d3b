// nan_free_probe.cpp — "no height of the map is NaN" as a terrain handle keeps
// it (csrc/host/gbp_terrain_patch.cpp: nan_free, the scan of
// gbp_terrain_create, and nan_free_after, the rule behind every write of the
// host mirror), on heap arrays of exactly the stated sizes, for
// AddressSanitizer / UBSan (tests/test_nan_free_host.py).
//
//   nan_free_probe NX NY storage < input
//
// First line: the NX NY heights of the map (hex floats, x-major); the mirror
// holds them rounded to float when storage is GBP_STORAGE_F32, as create does.
// Then one patch per line, applied to the same mirror in order: ix0 iy0 nx ny
// v_0 ... v_{nx ny - 1} (GBP_SRC_F64_XMAJOR, ld = ny).  Output: one line for
// the create scan, one per patch: rc fact, where rc is check_patch's status
// (a rejected patch writes nothing and keeps the fact, as
// gbp_terrain_update_host does) and fact is 0 or 1.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "gbp_terrain_patch.h"

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  const int NX = atoi(argv[1]), NY = atoi(argv[2]), storage = atoi(argv[3]);
  const bool f32 = storage == GBP_STORAGE_F32;
  const size_t cells = (size_t)NX * NY;
  std::unique_ptr<double[]> m(new double[cells]);
  for (size_t i = 0; i < cells; i++) {
    double v;
    if (scanf("%la", &v) != 1) return 3;
    m[i] = f32 ? (double)(float)v : v;
  }
  bool fact = gbp_patch::nan_free(m.get(), cells);
  printf("0 %d\n", fact ? 1 : 0);
  gbp_rect r;
  while (scanf("%d %d %d %d", &r.ix0, &r.iy0, &r.nx, &r.ny) == 4) {
    const long long n = (long long)r.nx * r.ny;
    if (n <= 0) return 4;
    // exactly n elements on the heap: an index past the source is an ASan report
    std::unique_ptr<double[]> src(new double[n]);
    for (long long i = 0; i < n; i++)
      if (scanf("%la", &src[i]) != 1) return 3;
    gbp_patch::Rect q;
    const int rc = gbp_patch::check_patch(NX, NY, storage, &r, GBP_SRC_F64_XMAJOR, r.ny, src.get(), &q);
    if (rc == GBP_OK) {
      gbp_patch::scatter(m.get(), NX, NY, q, GBP_SRC_F64_XMAJOR, r.ny, src.get(), f32);
      fact = gbp_patch::nan_free_after(m.get(), NX, NY, q, fact);
    }
    printf("%d %d\n", rc, fact ? 1 : 0);
  }
  return 0;
}
