// tree_path_probe.cpp — runs gbp_amd::joinTreePaths (csrc/host/gbp_tree_path.cpp)
// on one pair of trees read from a text file and prints the joined path, every
// double as a hex float so the test compares bits (tests/test_tree_path.py
// builds this with -fsanitize=address,undefined; the tree arrays are heap
// arrays of exactly the trees' sizes so an overrun is caught).
//
// input:  na nb ia ib, then per tree (Ta first): 8 n state values, 10 n action
//         values, n parents (root -1), n g values
// output: m, then 8 m state values, 10 (m - 1) action values, length, yaw, duration
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "gbp_tree_path.h"

using gbp_amd::Action;
using gbp_amd::State;

static bool read_double(FILE *f, double *v) {
  char tok[64];
  if (std::fscanf(f, "%63s", tok) != 1) return false;
  char *end = nullptr;
  *v = std::strtod(tok, &end);
  return end && *end == 0;
}

struct Tree {
  std::unique_ptr<State[]> v;
  std::unique_ptr<Action[]> a;
  std::unique_ptr<int[]> parent;
  std::unique_ptr<double[]> g;
  bool read(FILE *f, long long n) {
    v.reset(new State[n]);
    a.reset(new Action[n]);
    parent.reset(new int[n]);
    g.reset(new double[n]);
    for (long long i = 0; i < n; i++)
      for (double &x : v[i])
        if (!read_double(f, &x)) return false;
    for (long long i = 0; i < n; i++)
      for (double &x : a[i])
        if (!read_double(f, &x)) return false;
    for (long long i = 0; i < n; i++)
      if (std::fscanf(f, "%d", &parent[i]) != 1) return false;
    for (long long i = 0; i < n; i++)
      if (!read_double(f, &g[i])) return false;
    return true;
  }
  gbp_amd::TreeView view() const { return {v.get(), a.get(), parent.get(), g.get()}; }
};

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  long long na = 0, nb = 0;
  int ia = 0, ib = 0;
  if (std::fscanf(f, "%lld %lld %d %d", &na, &nb, &ia, &ib) != 4) return 3;
  if (na < 1 || nb < 1 || ia < 0 || ia >= na || ib < 0 || ib >= nb) return 3;
  Tree A, B;
  if (!A.read(f, na) || !B.read(f, nb)) return 3;
  std::fclose(f);
  const gbp_amd::JoinedPath p = gbp_amd::joinTreePaths(A.view(), ia, B.view(), ib);
  if (p.states.empty() || p.actions.size() + 1 != p.states.size()) return 4;
  std::printf("%zu\n", p.states.size());
  for (const State &s : p.states)
    for (double x : s) std::printf("%a\n", x);
  for (const Action &a : p.actions)
    for (double x : a) std::printf("%a\n", x);
  std::printf("%a\n%a\n%a\n", p.length, p.yaw, p.duration);
  return 0;
}
