// ReplanSession (include/gbp_planner.h) through one replanning scenario, for
// tests/test_gpu_replan_session.py, which compares every record with the
// oracle's and the numpy restatements' values:
//   1  begin + search(H halves)            | buildRRTStarConnectDevice, same arguments
//   2  gbp_terrain_update_host(rectangle), mapChanged, bestPath
//   3  robotAt(the best path's second state), bestPath
//   4  search(H2 halves)
//   5  buildRRTStarConnectDevice warm-started from step 3's dump and list (warm_shared)
//   6  a second session whose map change (every height + 50 m) leaves no connection
//
//   replan_session_node <input.bin> <output.bin>
// input:  int32 nx ny has_slopes; x[nx] y[ny] z[nx ny] (dx dy dz [nx ny]) f64;
//         int32 ix0 iy0 pnx pny; patch z[pnx pny] f64; start[8] goal[8] f64;
//         int32 batch H H2; uint64 seed
// output: records (uint32 name length, name, char 'd' | 'i' | 'q', int64 count, data)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gbp_planner_compat.h"

using gbp_amd::BatchStats;
using gbp_amd::TreeDump;

static FILE *out_ = nullptr;

template <class T>
static void put(const std::string &name, char type, const T *data, size_t count) {
  const uint32_t len = (uint32_t)name.size();
  const int64_t n = (int64_t)count;
  std::fwrite(&len, 4, 1, out_);
  std::fwrite(name.data(), 1, len, out_);
  std::fwrite(&type, 1, 1, out_);
  std::fwrite(&n, 8, 1, out_);
  if (count) std::fwrite(data, sizeof(T), count, out_);
}
static void put_i(const std::string &name, std::vector<int64_t> v) { put(name, 'q', v.data(), v.size()); }
static void put_d(const std::string &name, std::vector<double> v) { put(name, 'd', v.data(), v.size()); }

static void put_trees(const std::string &tag, const TreeDump &d) {
  for (int k = 0; k < 2; k++) {
    const std::string t = tag + (k ? ".b." : ".a.");
    put(t + "v", 'd', d.v[k].empty() ? nullptr : d.v[k][0].data(), 8 * d.v[k].size());
    put(t + "act", 'd', d.a[k].empty() ? nullptr : d.a[k][0].data(), 10 * d.a[k].size());
    put(t + "parent", 'i', d.parent[k].data(), d.parent[k].size());
    put(t + "g", 'd', d.g[k].data(), d.g[k].size());
  }
}
static void put_list(const std::string &tag, const std::vector<std::array<int32_t, 2>> &pairs,
                     int32_t best_a, int32_t best_b, double best_cost) {
  put(tag + ".pairs", 'i', pairs.empty() ? nullptr : pairs[0].data(), 2 * pairs.size());
  put_i(tag + ".best", {best_a, best_b});
  put_d(tag + ".best_cost", {best_cost});
}
static void put_state(const std::string &tag, ReplanSession &s) {
  TreeDump d;
  s.dump(d);
  put_trees(tag, d);
  std::vector<std::array<int32_t, 2>> pairs;
  std::array<int32_t, 2> best;
  double cost = 0;
  s.sharedConnections(pairs, &best, &cost);
  put_list(tag, pairs, best[0], best[1], cost);
}
static bool put_path(const std::string &tag, ReplanSession &s, std::vector<State> &states) {
  std::vector<Action> actions;
  const bool found = s.bestPath(states, actions);
  put_i(tag + ".found", {found ? 1 : 0});
  put(tag + ".states", 'd', states.empty() ? nullptr : states[0].data(), 8 * states.size());
  put(tag + ".actions", 'd', actions.empty() ? nullptr : actions[0].data(), 10 * actions.size());
  put_d(tag + ".length_yaw_cost", {s.pathLength(), s.pathYaw(), s.pathCost(), s.bestCost()});
  return found;
}

struct Handle {  // an engine terrain handle of this program's own
  gbp_terrain *t = nullptr;
  ~Handle() {
    if (t) gbp_terrain_destroy(t);
  }
};

template <class T>
static std::vector<T> get(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
    std::fprintf(stderr, "short input\n");
    std::exit(3);
  }
  return v;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  out_ = std::fopen(argv[2], "wb");
  if (!f || !out_) return 2;
  const auto dims = get<int32_t>(f, 3);
  const int nx = dims[0], ny = dims[1];
  const bool slopes = dims[2] != 0;
  const auto x = get<double>(f, nx), y = get<double>(f, ny), z = get<double>(f, (size_t)nx * ny);
  std::vector<double> dx, dy, dz;
  if (slopes) {
    dx = get<double>(f, (size_t)nx * ny);
    dy = get<double>(f, (size_t)nx * ny);
    dz = get<double>(f, (size_t)nx * ny);
  }
  const auto rect = get<int32_t>(f, 4);
  const auto patch = get<double>(f, (size_t)rect[2] * rect[3]);
  const auto sg = get<double>(f, 16);
  const auto cfg = get<int32_t>(f, 3);
  const uint64_t seed = get<uint64_t>(f, 1)[0];
  std::fclose(f);
  State start, goal;
  for (int k = 0; k < 8; k++) {
    start[k] = sg[k];
    goal[k] = sg[8 + k];
  }
  const int batch = cfg[0], H = cfg[1], H2 = cfg[2];
  try {
    // fp64 storage: the changed heights need not round-trip through float, and
    // an update never changes a handle's storage (FastTerrainMap's own handles
    // choose it from the first map)
    Handle h0, h1;
    auto load = [&](Handle &h) {
      const int rc = gbp_terrain_create(0, nx, ny, x.data(), y.data(), z.data(),
                                        slopes ? dx.data() : nullptr, slopes ? dy.data() : nullptr,
                                        slopes ? dz.data() : nullptr, GBP_STORAGE_F64, &h.t);
      if (rc) throw gbp_amd::EngineError(rc, "gbp_terrain_create");
      return FastTerrainMap::borrow(h.t);
    };
    {  // the reference of step 1: one build call
      FastTerrainMap terrain = load(h0);
      RRTStarConnectClass planner;
      planner.setSeed(seed);
      BatchStats st;
      TreeDump d;
      std::vector<std::array<int32_t, 2>> pairs;
      st.max_halves = H;
      st.dump = &d;
      st.shared_dump = &pairs;
      std::vector<State> states;
      std::vector<Action> actions;
      planner.buildRRTStarConnectDevice(terrain, start, goal, batch, 1e9, states, actions, &st);
      put_trees("build", d);
      put_list("build", pairs, st.meet_a, st.meet_b, planner.bestCost());
      put_i("build.counters", {st.halves, st.solutions, st.rewires});
    }
    FastTerrainMap terrain = load(h1);
    ReplanSession s;
    s.begin(terrain, start, goal, batch, 3.0, seed);
    BatchStats st1;
    s.search(1e9, H, &st1);
    put_state("s1", s);
    put_i("s1.counters", {st1.halves, st1.solutions, st1.rewires, s.nextHalf(), s.extendCounter()});
    // 2: the map changes under the resident trees
    const gbp_rect box{rect[0], rect[1], rect[2], rect[3]};
    const int urc = gbp_terrain_update_host(h1.t, &box, GBP_SRC_F64_XMAJOR, rect[3], patch.data(),
                                            nullptr, nullptr, nullptr);
    if (urc) throw gbp_amd::EngineError(urc, "gbp_terrain_update_host");
    PruneStats ps[2];
    SharedStats sh;
    s.mapChanged(terrain, ps, &sh);
    for (int k = 0; k < 2; k++)
      put_i(k ? "s2.prune.b" : "s2.prune.a",
            {ps[k].n_before, ps[k].n_kept, ps[k].n_edge_invalid, ps[k].n_inherited});
    put_i("s2.shared", {sh.n_before, sh.n_kept, sh.n_dropped_a, sh.n_dropped_b});
    put_state("s2", s);
    std::vector<State> path;
    if (!put_path("s2.path", s, path) || path.size() < 3) {
      std::fprintf(stderr, "no path of three states after the map change\n");
      return 4;
    }
    // 3: the robot reaches the path's second state
    RerootStats rs;
    s.robotAt(path[1], rs, &sh);
    put_i("s3.reroot", {rs.n_before, rs.n_kept, rs.n_outside, rs.n_edge_invalid, rs.n_inherited, rs.depth});
    put_i("s3.shared", {sh.n_before, sh.n_kept, sh.n_dropped_a, sh.n_dropped_b});
    put_state("s3", s);
    std::vector<State> path3;
    put_path("s3.path", s, path3);
    put_i("s3.counters", {s.nextHalf(), s.extendCounter()});
    TreeDump d3;
    s.dump(d3);
    std::vector<std::array<int32_t, 2>> list3;
    s.sharedConnections(list3);
    const int32_t half3 = s.nextHalf();
    const int64_t ext3 = s.extendCounter();
    // 4: the search goes on
    BatchStats st4;
    s.search(1e9, H2, &st4);
    put_state("s4", s);
    put_i("s4.counters", {st4.halves, st4.solutions, st4.rewires, s.nextHalf(), s.extendCounter()});
    std::vector<State> path4;
    put_path("s4.path", s, path4);
    s.end();
    // 5: the same continuation as a warm start of the one-call build
    {
      RRTStarConnectClass planner;
      planner.setSeed(seed);
      BatchStats st;
      TreeDump d;
      std::vector<std::array<int32_t, 2>> pairs;
      st.max_halves = H2;
      st.dump = &d;
      st.shared_dump = &pairs;
      for (int k = 0; k < 2; k++) {
        st.warm_n[k] = (int64_t)d3.v[k].size();
        st.warm_v[k] = d3.v[k][0].data();
        st.warm_a[k] = d3.a[k][0].data();
        st.warm_parent[k] = d3.parent[k].data();
      }
      st.warm_half = half3;
      st.warm_extend = ext3;
      st.warm_shared = list3.empty() ? nullptr : list3[0].data();
      st.warm_shared_n = (int64_t)list3.size();
      std::vector<State> states;
      std::vector<Action> actions;
      planner.buildRRTStarConnectDevice(terrain, d3.v[0][0], goal, batch, 1e9, states, actions, &st);
      put_trees("warm", d);
      put_list("warm", pairs, st.meet_a, st.meet_b, planner.bestCost());
      put_i("warm.counters", {st.halves, st.solutions, st.rewires});
    }
    // 6: a map change that leaves nothing: every height raised by 50 m, so no
    // edge holds, both trees shrink to their roots and no connection survives
    {
      Handle h2;
      FastTerrainMap t2 = load(h2);
      ReplanSession s6;
      s6.begin(t2, start, goal, batch, 3.0, seed);
      s6.search(1e9, H);
      std::vector<double> high(z);
      for (double &v : high) v += 50.0;
      const int rc = gbp_terrain_update_host(h2.t, nullptr, GBP_SRC_F64_XMAJOR, ny, high.data(), nullptr,
                                             nullptr, nullptr);
      if (rc) throw gbp_amd::EngineError(rc, "gbp_terrain_update_host (whole map)");
      PruneStats p6[2];
      SharedStats sh6;
      s6.mapChanged(t2, p6, &sh6);
      put_i("s6.kept", {p6[0].n_kept, p6[1].n_kept});
      put_i("s6.shared", {sh6.n_before, sh6.n_kept, sh6.n_dropped_a, sh6.n_dropped_b});
      put_state("s6", s6);
      std::vector<State> none;
      put_path("s6.path", s6, none);
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "replan_session_node: %s\n", e.what());
    return 1;
  }
  std::fclose(out_);
  return 0;
}
