// The slope rule of csrc/gbp_slopes.h on the host, for tests/test_slopes_host.py.
// Built stand-alone with AddressSanitizer and UBSan; the arrays are heap
// allocations of exactly the stated sizes.
//
// stdin, per case:  nx ny flags, then nx + ny + nx*ny doubles as C99 hex floats
// (x, y, then z x-major).  stdout, per case: three lines (dx, dy, dz), nx*ny
// values each as the 16 hex digits of their bit pattern.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "gbp_slopes.h"

static bool read_doubles(double *d, size_t n) {
  char tok[64];
  for (size_t i = 0; i < n; i++) {
    if (scanf("%63s", tok) != 1) return false;
    d[i] = strtod(tok, nullptr);
  }
  return true;
}

int main() {
  int nx, ny, flags;
  while (scanf("%d %d %d", &nx, &ny, &flags) == 3) {
    if (nx < 2 || ny < 2) return 2;
    const size_t cells = (size_t)nx * ny;
    std::unique_ptr<double[]> x(new double[nx]), y(new double[ny]), z(new double[cells]);
    std::unique_ptr<double[]> out(new double[3 * cells]);
    if (!read_doubles(x.get(), nx) || !read_doubles(y.get(), ny) || !read_doubles(z.get(), cells))
      return 3;
    for (int ix = 0; ix < nx; ix++)
      for (int iy = 0; iy < ny; iy++) {
        double n[3];
        gbp::slope_node_xmajor(z.get(), x.get(), y.get(), nx, ny, ix, iy, flags, n);
        for (int k = 0; k < 3; k++) out[k * cells + (size_t)ix * ny + iy] = n[k];
      }
    for (int k = 0; k < 3; k++) {
      for (size_t i = 0; i < cells; i++) {
        uint64_t b;
        memcpy(&b, &out[k * cells + i], sizeof b);
        printf("%016" PRIx64 "%c", b, i + 1 == cells ? '\n' : ' ');
      }
    }
  }
  return 0;
}
