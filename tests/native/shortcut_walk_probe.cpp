// shortcut_walk_probe.cpp — runs gbp_shortcut::walk (csrc/host/gbp_shortcut_walk.cpp)
// on one path read from a text file and prints what it keeps, every double as
// a hex float so the test compares bits (tests/test_shortcut_walk.py builds
// this with -fsanitize=address,undefined; the buffers are heap arrays of
// exactly the documented sizes so an overrun is caught).
//
// input:  n add_yaw length_weight yaw_weight
//         8 n state values, 10 (n - 1) action values, n (n - 1) / 2 table entries (0 / 1)
// output: m, then 8 m state values, 10 (m - 1) action values, length, yaw, cost
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gbp_shortcut_walk.h"

static bool read_double(FILE *f, double *v) {
  char tok[64];
  if (std::fscanf(f, "%63s", tok) != 1) return false;
  char *end = nullptr;
  *v = std::strtod(tok, &end);
  return end && *end == 0;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  long long n = 0;
  gbp_shortcut::CostWeights cw;
  if (std::fscanf(f, "%lld %d", &n, &cw.add_yaw) != 2 || n < 2) return 3;
  if (!read_double(f, &cw.length_weight) || !read_double(f, &cw.yaw_weight)) return 3;
  std::vector<double> states(8 * n), actions(10 * (n - 1));
  std::vector<uint8_t> reached(gbp_shortcut::pair_count(n));
  for (double &v : states)
    if (!read_double(f, &v)) return 3;
  for (double &v : actions)
    if (!read_double(f, &v)) return 3;
  for (uint8_t &r : reached) {
    int b = 0;
    if (std::fscanf(f, "%d", &b) != 1) return 3;
    r = (uint8_t)b;
  }
  std::fclose(f);
  double *os = new double[8 * n], *oa = new double[10 * (n - 1)];
  double len = 0, yaw = 0, cost = 0;
  const int64_t m = gbp_shortcut::walk(n, states.data(), actions.data(), reached.data(), cw, os, oa,
                                       &len, &yaw, &cost);
  if (m < 0) return 4;
  std::printf("%lld\n", (long long)m);
  for (int64_t k = 0; k < 8 * m; k++) std::printf("%a\n", os[k]);
  for (int64_t k = 0; k < 10 * (m - 1); k++) std::printf("%a\n", oa[k]);
  std::printf("%a\n%a\n%a\n", len, yaw, cost);
  delete[] os;
  delete[] oa;
  return 0;
}
