// The robot-moved sequence of a node that keeps its trees: a
// search, RRTConnectClass::rerootStartTree at the path's second state, the
// next search from that state with BatchStats::warm_*, through the reference's
// global names (gbp_planner_compat.h).  Built and run by
// tests/test_gpu_tree_reroot.py the way node_callsite.cpp is.
//
// argv[1]: a binary file — int32 nx, ny; doubles x[nx], y[ny], then z, dx, dy,
//          dz [nx][ny]; doubles start[8], goal[8]
// argv[2]: receives int32 vertex; tree a before and after the re-root, each as
//          int32 n, doubles v[n][8], a[n][10], g[n], int32 parent[n]; int32 n,
//          int32 remap[n]; int64 n_before n_kept n_outside n_edge_invalid
//          n_inherited depth
// output:  one line: the first search's vertices, the re-root's counters, the
//          second search's vertices and path states
// exit:    4 no first path, 5 the path leaves the start tree at its root,
//          6 the re-rooted tree is not what was asked for, 7 no second path
#include <cstdio>
#include <cstring>
#include <vector>

#include "gbp_planner_compat.h"

using gbp_amd::Action;
using gbp_amd::BatchStats;
using gbp_amd::RerootStats;
using gbp_amd::State;
using gbp_amd::TreeDump;

template <class T>
static bool get(FILE *f, T *p, size_t n) {
  return std::fread(p, sizeof(T), n, f) == n;
}
template <class T>
static void put(FILE *f, const T *p, size_t n) {
  std::fwrite(p, sizeof(T), n, f);
}
static void put_tree(FILE *f, const TreeDump &t) {
  const int32_t n = (int32_t)t.v[0].size();
  put(f, &n, 1);
  put(f, t.v[0][0].data(), 8 * (size_t)n);
  put(f, t.a[0][0].data(), 10 * (size_t)n);
  put(f, t.g[0].data(), n);
  put(f, t.parent[0].data(), n);
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
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
  State start, goal;
  if (!get(f, start.data(), 8) || !get(f, goal.data(), 8)) return 3;
  std::fclose(f);

  FastTerrainMap terrain_;
  terrain_.loadDataFlat((int)nx, (int)ny, x.data(), y.data(), layer[0].data(), layer[1].data(),
                        layer[2].data(), layer[3].data());
  RRTConnectClass rrt_connect_obj;
  rrt_connect_obj.set_state_action_pair_check_adaptive_step_size_flag_(false);
  const int batch = 256;

  // the search whose plan the robot starts to execute
  TreeDump trees;
  BatchStats first;
  first.dump = &trees;
  std::vector<State> state_sequence;
  std::vector<Action> action_sequence;
  if (!rrt_connect_obj.buildRRTConnectDevice(terrain_, start, goal, batch, 60.0, state_sequence,
                                             action_sequence, &first))
    return 4;
  // the path's second state is a vertex of the start tree: the second of the
  // chain root -> meet_a
  std::vector<int32_t> chain;
  for (int32_t i = first.meet_a; i >= 0 && chain.size() <= trees.parent[0].size(); i = trees.parent[0][i])
    chain.push_back(i);
  if (chain.size() < 2 || chain.back() != 0) return 5;
  const int32_t vertex = chain[chain.size() - 2];
  const State stands_on = trees.v[0][vertex];

  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  put(o, &vertex, 1);
  put_tree(o, trees);
  RerootStats rs;
  std::vector<int32_t> remap;
  rrt_connect_obj.rerootStartTree(terrain_, trees, vertex, rs, &remap);
  put_tree(o, trees);
  const int32_t n = (int32_t)remap.size();
  const int64_t counters[6] = {rs.n_before, rs.n_kept, rs.n_outside, rs.n_edge_invalid, rs.n_inherited,
                               rs.depth};
  put(o, &n, 1);
  put(o, remap.data(), n);
  put(o, counters, 6);
  std::fclose(o);
  if ((int64_t)trees.v[0].size() != rs.n_kept || rs.n_kept < (int64_t)chain.size() - 1 ||
      std::memcmp(trees.v[0][0].data(), stands_on.data(), sizeof(State)) != 0 ||
      trees.parent[0][0] != -1 || trees.g[0][0] != 0.0 || remap[vertex] != 0 || remap[0] != -1 ||
      remap[first.meet_a] < 0)
    return 6;

  // the next search, from where the robot stands, warm-started with the kept
  // start tree and the goal tree as it was
  BatchStats next;
  for (int k = 0; k < 2; k++) {
    next.warm_n[k] = (int64_t)trees.v[k].size();
    next.warm_v[k] = trees.v[k][0].data();
    next.warm_a[k] = trees.a[k][0].data();
    next.warm_parent[k] = trees.parent[k].data();
  }
  next.warm_half = 2 * ((first.iterations + 1) / 2 + 1);
  next.warm_extend = first.extends;
  state_sequence.clear();
  action_sequence.clear();
  if (!rrt_connect_obj.buildRRTConnectDevice(terrain_, trees.v[0][0], goal, batch, 60.0, state_sequence,
                                             action_sequence, &next) ||
      state_sequence.empty() ||
      std::memcmp(state_sequence.front().data(), stands_on.data(), sizeof(State)) != 0 ||
      next.vertices_a < rs.n_kept)
    return 7;
  std::printf("first %lld+%lld vertices; re-rooted at %d: %lld of %lld kept, %lld outside, depth %lld; "
              "next %lld+%lld vertices, %zu path states\n",
              (long long)first.vertices_a, (long long)first.vertices_b, vertex, (long long)rs.n_kept,
              (long long)rs.n_before, (long long)rs.n_outside, (long long)rs.depth,
              (long long)next.vertices_a, (long long)next.vertices_b, state_sequence.size());
  return 0;
}
