// informed_probe.cpp — runs gbp_informed_ellipse (csrc/host/gbp_informed.cpp)
// on the cases of a text file (tests/test_informed_ref.py builds this with
// -fsanitize=address,undefined; no engine, no device).
//
// input:  per line ax ay bx by cost x0 xN y0 yM (strtod: nan, inf and hex floats read)
// output: per line the return code, then active and cost cx cy ux uy a b as the
//         bit patterns of the doubles (hex); a refused case must leave *out untouched
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gbp.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char tok[9][64];
  while (std::fscanf(f, "%63s %63s %63s %63s %63s %63s %63s %63s %63s", tok[0], tok[1], tok[2],
                     tok[3], tok[4], tok[5], tok[6], tok[7], tok[8]) == 9) {
    double v[9];
    for (int k = 0; k < 9; k++) v[k] = std::strtod(tok[k], nullptr);
    const double fa[2] = {v[0], v[1]}, fb[2] = {v[2], v[3]}, bounds[4] = {v[5], v[6], v[7], v[8]};
    gbp_informed e;
    std::memset(&e, 0x5a, sizeof e);
    gbp_informed before = e;
    const int rc = gbp_informed_ellipse(fa, fb, v[4], bounds, &e);
    if (rc != GBP_OK && std::memcmp(&e, &before, sizeof e) != 0) return 6;
    if (rc == GBP_OK && e.reserved != 0) return 4;
    std::printf("%d %d", rc, rc == GBP_OK ? e.active : 0);
    const double out[7] = {e.cost, e.cx, e.cy, e.ux, e.uy, e.a, e.b};
    for (double x : out) {
      uint64_t b;
      std::memcpy(&b, &x, 8);
      std::printf(" %016" PRIx64, rc == GBP_OK ? b : (uint64_t)0);
    }
    std::printf("\n");
  }
  std::fclose(f);
  if (gbp_informed_ellipse(nullptr, nullptr, 1.0, nullptr, nullptr) != GBP_E_INVALID_ARG) return 5;
  return 0;
}
