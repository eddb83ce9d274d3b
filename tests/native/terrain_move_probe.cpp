// terrain_move_probe.cpp — the engine-free part of a terrain window moved by
// whole cells (csrc/host/gbp_terrain_patch.cpp: move_rects, shift_mirror,
// nan_free_after_move, detect_shift) on heap arrays of exactly the stated
// sizes, for AddressSanitizer / UBSan (tests/test_terrain_move_host.py).
//
//   terrain_move_probe < cases
//
// One case per line, numbers as hex floats:
//   M NX NY sx sy storage old_0 .. old_{NX NY - 1} src_0 .. src_{NX NY - 1}
//     the old mirror and the whole new map (GBP_SRC_F64_XMAJOR, ld = NY) moved
//     as gbp_terrain_move_host moves its mirror: shift_mirror, the strips
//     scattered, nan_free_after_move with `was` = the old mirror's full scan.
//     Output: ox0 oy0 onx ony nstrips (ix0 iy0 nx ny) x 2 nan_free m_0 ..
//   D N rel_tol o_0 .. o_{N-1} n_0 .. n_{N-1}
//     Output: accepted shift   (shift = 0 when refused)
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "gbp_terrain_patch.h"

static bool read_doubles(double *d, long long n) {
  for (long long i = 0; i < n; i++)
    if (scanf("%la", &d[i]) != 1) return false;
  return true;
}

int main() {
  char cmd;
  while (scanf(" %c", &cmd) == 1) {
    if (cmd == 'M') {
      int NX, NY, storage;
      long long sx, sy;
      if (scanf("%d %d %lld %lld %d", &NX, &NY, &sx, &sy, &storage) != 5) return 3;
      const size_t cells = (size_t)NX * NY;
      std::unique_ptr<double[]> m(new double[cells]), src(new double[cells]);
      if (!read_doubles(m.get(), (long long)cells) || !read_doubles(src.get(), (long long)cells))
        return 3;
      const bool was = gbp_patch::nan_free(m.get(), cells);
      const gbp_patch::MoveRects mr = gbp_patch::move_rects(NX, NY, sx, sy);
      gbp_patch::shift_mirror(m.get(), NX, NY, sx, sy, mr);
      for (int k = 0; k < mr.nstrips; k++)
        gbp_patch::scatter(m.get(), NX, NY, mr.strip[k], GBP_SRC_F64_XMAJOR, NY,
                           gbp_patch::move_src(GBP_SRC_F64_XMAJOR, NY, src.get(), mr.strip[k]),
                           storage == GBP_STORAGE_F32);
      const bool nf = gbp_patch::nan_free_after_move(m.get(), NX, NY, mr, was);
      printf("%d %d %d %d %d", mr.overlap.ix0, mr.overlap.iy0, mr.overlap.nx, mr.overlap.ny,
             mr.nstrips);
      for (int k = 0; k < 2; k++)
        printf(" %d %d %d %d", mr.strip[k].ix0, mr.strip[k].iy0, mr.strip[k].nx, mr.strip[k].ny);
      printf(" %d", nf ? 1 : 0);
      for (size_t i = 0; i < cells; i++) printf(" %a", m[i]);
      printf("\n");
    } else if (cmd == 'D') {
      int N;
      double tol;
      if (scanf("%d %la", &N, &tol) != 2 || N < 0) return 3;
      std::unique_ptr<double[]> o(new double[N]), n(new double[N]);
      if (!read_doubles(o.get(), N) || !read_doubles(n.get(), N)) return 3;
      int shift = 0;
      const bool ok = gbp_patch::detect_shift(o.get(), n.get(), N, tol, &shift);
      printf("%d %d\n", ok ? 1 : 0, ok ? shift : 0);
    } else {
      return 2;
    }
  }
  return 0;
}
