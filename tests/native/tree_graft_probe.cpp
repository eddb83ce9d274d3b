// tree_graft_probe.cpp — runs gbp_amd::applyGraftRemap
// (csrc/host/gbp_tree_prune.cpp) on one tree read from a text file
// (tests/test_tree_graft_ref.py builds this with -fsanitize=address,undefined).
//
// input:  n, then n remap entries, n parents (root -1), n attach flags
// output: the kept count, the new root included (-1: refused, and the tree
//         must be untouched), then per survivor: its parent, the old index
//         its v / g rows came from (-1: the root state) and the old index its
//         action names (1000000 + i: the connect action of old vertex i; -1:
//         the root's zeros)
// Row i of v, a and g holds i in every element, the connect action of vertex
// i holds 1000000 + i and the root state -1, so a row names its origin.
#include <cstdio>
#include <vector>

#include "gbp_tree_prune.h"

using gbp_amd::Action;
using gbp_amd::State;

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  long long n = 0;
  if (std::fscanf(f, "%lld", &n) != 1 || n < 1) return 3;
  std::vector<int32_t> remap((size_t)n), parent((size_t)n);
  std::vector<uint8_t> attach((size_t)n);
  for (auto &x : remap)
    if (std::fscanf(f, "%d", &x) != 1) return 3;
  for (auto &x : parent)
    if (std::fscanf(f, "%d", &x) != 1) return 3;
  for (auto &x : attach) {
    int b = 0;
    if (std::fscanf(f, "%d", &b) != 1) return 3;
    x = (uint8_t)b;
  }
  std::fclose(f);
  gbp_amd::TreeDump trees;
  std::vector<Action> actions((size_t)n);
  trees.v[0].resize((size_t)n);
  trees.a[0].resize((size_t)n);
  trees.g[0].resize((size_t)n);
  trees.parent[0] = parent;
  for (long long i = 0; i < n; i++) {
    trees.v[0][i].fill((double)i);
    trees.a[0][i].fill((double)i);
    trees.g[0][i] = (double)i;
    actions[i].fill(1000000.0 + (double)i);
  }
  State root;
  root.fill(-1.0);
  const bool ok = gbp_amd::applyGraftRemap(remap, root, attach, actions, trees, 0);
  if (!ok) {
    if ((long long)trees.v[0].size() != n || trees.parent[0] != parent) return 6;
    for (long long i = 0; i < n; i++)
      if (trees.v[0][i][0] != (double)i || trees.a[0][i][9] != (double)i || trees.g[0][i] != (double)i)
        return 6;
    std::printf("-1\n");
    return 0;
  }
  const long long kept = (long long)trees.v[0].size();
  if ((long long)trees.a[0].size() != kept || (long long)trees.parent[0].size() != kept ||
      (long long)trees.g[0].size() != kept)
    return 4;
  std::printf("%lld\n", kept);
  for (long long j = 0; j < kept; j++) {
    const double src = j == 0 ? -1.0 : trees.g[0][j];
    if (j == 0 && trees.g[0][0] != 0.0) return 4;
    for (double x : trees.v[0][j])
      if (x != src) return 4;
    const double a0 = trees.a[0][j][0];
    for (double x : trees.a[0][j])
      if (x != a0) return 4;
    if (j == 0 && a0 != 0.0) return 4;
    std::printf("%d %lld %lld\n", trees.parent[0][j], (long long)src, j == 0 ? -1LL : (long long)a0);
  }
  return 0;
}
