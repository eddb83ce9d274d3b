// tree_prune_probe.cpp — runs gbp_amd::applyPruneRemap
// (csrc/host/gbp_tree_prune.cpp) on one tree read from a text file and prints
// the survivors (tests/test_tree_prune_ref.py builds this with
// -fsanitize=address,undefined; the arrays are heap arrays of exactly the
// tree's size so an overrun is caught).
//
// input:  n, then n remap entries, n parents (root -1)
// output: the kept count (-1: refused), then per survivor: its parent and the
//         old index its v / a / g rows came from
// Row i of v, a and g holds i in every element, so a moved row names its origin.
#include <cstdio>
#include <memory>

#include "gbp_tree_prune.h"

using gbp_amd::Action;
using gbp_amd::State;

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  long long n = 0;
  if (std::fscanf(f, "%lld", &n) != 1 || n < 1) return 3;
  std::unique_ptr<int32_t[]> remap(new int32_t[n]), parent(new int32_t[n]);
  std::unique_ptr<State[]> v(new State[n]);
  std::unique_ptr<Action[]> a(new Action[n]);
  std::unique_ptr<double[]> g(new double[n]);
  for (long long i = 0; i < n; i++)
    if (std::fscanf(f, "%d", &remap[i]) != 1) return 3;
  for (long long i = 0; i < n; i++)
    if (std::fscanf(f, "%d", &parent[i]) != 1) return 3;
  std::fclose(f);
  for (long long i = 0; i < n; i++) {
    v[i].fill((double)i);
    a[i].fill((double)i);
    g[i] = (double)i;
  }
  const long long kept = gbp_amd::applyPruneRemap(remap.get(), n, v.get(), a.get(), parent.get(), g.get());
  std::printf("%lld\n", kept);
  for (long long j = 0; j < kept; j++) {
    for (double x : v[j])
      if (x != g[j]) return 4;
    for (double x : a[j])
      if (x != g[j]) return 4;
    std::printf("%d %lld\n", parent[j], (long long)g[j]);
  }
  return 0;
}
