// The map-changed call of a node that keeps its trees:
// RRTConnectClass::revalidateTrees on a new FastTerrainMap, through the
// reference's global names (gbp_planner_compat.h).  Built and run by
// tests/test_gpu_tree_prune.py the way node_callsite.cpp is.
//
// argv[1]: a binary file — int32 nx, ny; doubles x[nx], y[ny], then z, dx, dy,
//          dz [nx][ny] of the NEW map; per tree (Ta, Tb): int32 n, doubles
//          v[n][8], a[n][10], g[n], int32 parent[n]
// output:  per tree one line: n_before n_kept n_edge_invalid n_inherited
//          fragile_resolved, then the survivors' parents on one line
#include <cstdio>
#include <vector>

#include "gbp_planner_compat.h"

// not reference names: the drop-in's own additions stay in its namespace
using gbp_amd::PruneStats;
using gbp_amd::TreeDump;

template <class T>
static bool get(FILE *f, T *p, size_t n) {
  return std::fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t dims[2];
  if (!get(f, dims, 2) || dims[0] < 2 || dims[1] < 2) return 3;
  const size_t nx = dims[0], ny = dims[1];
  std::vector<double> x(nx), y(ny), layer[4];
  if (!get(f, x.data(), nx) || !get(f, y.data(), ny)) return 3;
  for (auto &l : layer) {
    l.resize(nx * ny);
    if (!get(f, l.data(), nx * ny)) return 3;
  }
  TreeDump trees;
  for (int k = 0; k < 2; k++) {
    int32_t n = 0;
    if (!get(f, &n, 1) || n < 1) return 3;
    trees.v[k].resize(n);
    trees.a[k].resize(n);
    trees.g[k].resize(n);
    trees.parent[k].resize(n);
    if (!get(f, trees.v[k][0].data(), 8 * (size_t)n) || !get(f, trees.a[k][0].data(), 10 * (size_t)n) ||
        !get(f, trees.g[k].data(), n) || !get(f, trees.parent[k].data(), n))
      return 3;
  }
  std::fclose(f);

  FastTerrainMap terrain_;  // the map the callback just loaded
  terrain_.loadDataFlat((int)nx, (int)ny, x.data(), y.data(), layer[0].data(), layer[1].data(),
                        layer[2].data(), layer[3].data());
  RRTConnectClass rrt_connect_obj;
  rrt_connect_obj.set_state_action_pair_check_adaptive_step_size_flag_(false);
  PruneStats stats[2];
  std::vector<int32_t> remap[2];
  rrt_connect_obj.revalidateTrees(terrain_, trees, stats, remap);
  for (int k = 0; k < 2; k++) {
    if ((int64_t)remap[k].size() != stats[k].n_before ||
        (int64_t)trees.parent[k].size() != stats[k].n_kept)
      return 4;
    std::printf("%lld %lld %lld %lld %lld\n", (long long)stats[k].n_before, (long long)stats[k].n_kept,
                (long long)stats[k].n_edge_invalid, (long long)stats[k].n_inherited,
                (long long)stats[k].fragile_resolved);
    for (int32_t p : trees.parent[k]) std::printf("%d ", p);
    std::printf("\n");
  }
  return 0;
}
