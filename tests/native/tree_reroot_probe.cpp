// tree_reroot_probe.cpp — runs gbp_amd::applyRerootRemap
// (csrc/host/gbp_tree_prune.cpp) and the start-tree path helpers
// (csrc/host/gbp_tree_path.cpp) on one tree read from a text file
// (tests/test_tree_reroot_ref.py builds this with
// -fsanitize=address,undefined; the arrays are heap arrays of exactly the
// tree's size so an overrun is caught).
//
// input:  n, new_root, meet, then n remap entries, n parents (root -1)
// output: line 1: the vertices root -> meet of the tree as given (empty: none)
//         line 2: per vertex of that path, the index findStateAmong gives for
//                 its state among the path's vertices
//         then the kept count (-1: refused, and the rows must be untouched),
//         then per survivor: its parent and the old index its v / g rows came
//         from (a's too, but for the new root, whose action must be zeros)
// Row i of v, a and g holds i in every element, so a moved row names its origin.
#include <cstdio>
#include <memory>
#include <vector>

#include "gbp_tree_path.h"
#include "gbp_tree_prune.h"

using gbp_amd::Action;
using gbp_amd::State;

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  long long n = 0;
  int new_root = 0, meet = 0;
  if (std::fscanf(f, "%lld %d %d", &n, &new_root, &meet) != 3 || n < 1) return 3;
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
  const std::vector<int32_t> pv(parent.get(), parent.get() + n);
  const std::vector<State> vv(v.get(), v.get() + n);
  const std::vector<int> path = gbp_amd::startTreePath(pv, meet);
  for (int i : path) std::printf("%d ", i);
  std::printf("\n");
  for (int i : path) std::printf("%d ", gbp_amd::findStateAmong(vv, path, vv[i]));
  State nowhere;
  nowhere.fill(-1.0);
  if (gbp_amd::findStateAmong(vv, path, nowhere) != -1) return 5;
  std::printf("\n");
  const long long kept =
      gbp_amd::applyRerootRemap(remap.get(), n, new_root, v.get(), a.get(), parent.get(), g.get());
  std::printf("%lld\n", kept);
  if (kept < 0) {
    for (long long i = 0; i < n; i++)
      if (v[i][0] != (double)i || a[i][9] != (double)i || g[i] != (double)i || parent[i] != pv[i]) return 6;
    return 0;
  }
  for (long long j = 0; j < kept; j++) {
    for (double x : v[j])
      if (x != g[j]) return 4;
    for (double x : a[j])
      if (x != (j == 0 ? 0.0 : g[j])) return 4;
    std::printf("%d %lld\n", parent[j], (long long)g[j]);
  }
  return 0;
}
