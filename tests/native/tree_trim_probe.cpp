// tree_trim_probe.cpp — runs gbp_amd::applyTrimRemap
// (csrc/host/gbp_tree_prune.cpp) on one tree read from a text file
// (tests/test_tree_trim_ref.py builds this with -fsanitize=address,undefined).
//
// input:  n, then n remap entries, n parents (root -1), n keep flags
// output: 0 when the call refuses (and the tree must be untouched); else 1, the
//         record (n_before, n_kept, n_flagged, n_inherited), then per survivor
//         its parent and the old index its v / a / g rows came from
// Row i of v, a and g holds i in every element, so a row names its origin.
#include <cstdio>
#include <vector>

#include "gbp_tree_prune.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  long long n = 0;
  if (std::fscanf(f, "%lld", &n) != 1 || n < 1) return 3;
  std::vector<int32_t> remap((size_t)n), parent((size_t)n);
  std::vector<uint8_t> keep((size_t)n);
  for (auto &x : remap)
    if (std::fscanf(f, "%d", &x) != 1) return 3;
  for (auto &x : parent)
    if (std::fscanf(f, "%d", &x) != 1) return 3;
  for (auto &x : keep) {
    int b = 0;
    if (std::fscanf(f, "%d", &b) != 1) return 3;
    x = (uint8_t)b;
  }
  std::fclose(f);
  gbp_amd::TreeDump trees;
  trees.v[1].resize((size_t)n);
  trees.a[1].resize((size_t)n);
  trees.g[1].resize((size_t)n);
  trees.parent[1] = parent;
  for (long long i = 0; i < n; i++) {
    trees.v[1][i].fill((double)i);
    trees.a[1][i].fill((double)i);
    trees.g[1][i] = (double)i;
  }
  gbp_amd::TrimRemapRecord rec;
  rec.n_before = -7;
  if (!gbp_amd::applyTrimRemap(remap, keep, trees, 1, &rec)) {
    if ((long long)trees.v[1].size() != n || trees.parent[1] != parent || rec.n_before != -7) return 6;
    for (long long i = 0; i < n; i++)
      if (trees.v[1][i][0] != (double)i || trees.a[1][i][9] != (double)i || trees.g[1][i] != (double)i)
        return 6;
    std::printf("0\n");
    return 0;
  }
  const long long kept = (long long)trees.v[1].size();
  if ((long long)trees.a[1].size() != kept || (long long)trees.parent[1].size() != kept ||
      (long long)trees.g[1].size() != kept || rec.n_kept != kept || !trees.v[0].empty())
    return 4;
  std::printf("1 %lld %lld %lld %lld\n", (long long)rec.n_before, (long long)rec.n_kept,
              (long long)rec.n_flagged, (long long)rec.n_inherited);
  for (long long j = 0; j < kept; j++) {
    const double src = trees.g[1][j];
    for (double x : trees.v[1][j])
      if (x != src) return 4;
    for (double x : trees.a[1][j])
      if (x != src) return 4;
    std::printf("%d %lld\n", trees.parent[1][j], (long long)src);
  }
  return 0;
}
