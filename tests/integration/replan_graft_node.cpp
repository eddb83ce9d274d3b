// ReplanSession::robotOff / goalAt (include/gbp_planner.h) through one
// scenario, for tests/test_gpu_replan_graft.py, which compares every record
// with the oracle's and the numpy restatements' values:
//   1  begin + search(H halves)
//   1b robotOff and goalAt with a state that is valid in no phase: false, nothing changed
//   2  robotOff(root_a, radius), bestPath
//   3  goalAt(root_b, radius), bestPath
//   4  search(H2 halves), bestPath
//   5  a second session: begin + search(H halves), goalAt(goal_shift, radius)
//
//   replan_graft_node <input.bin> <output.bin>
// input:  int32 nx ny has_slopes; x[nx] y[ny] z[nx ny] (dx dy dz [nx ny]) f64;
//         start[8] goal[8] root_a[8] root_b[8] goal_shift[8] bad[8] f64; radius f64;
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

static void put_state(const std::string &tag, ReplanSession &s) {
  TreeDump d;
  s.dump(d);
  for (int k = 0; k < 2; k++) {
    const std::string t = tag + (k ? ".b." : ".a.");
    put(t + "v", 'd', d.v[k].empty() ? nullptr : d.v[k][0].data(), 8 * d.v[k].size());
    put(t + "act", 'd', d.a[k].empty() ? nullptr : d.a[k][0].data(), 10 * d.a[k].size());
    put(t + "parent", 'i', d.parent[k].data(), d.parent[k].size());
    put(t + "g", 'd', d.g[k].data(), d.g[k].size());
  }
  std::vector<std::array<int32_t, 2>> pairs;
  std::array<int32_t, 2> best;
  double cost = 0;
  s.sharedConnections(pairs, &best, &cost);
  put(tag + ".pairs", 'i', pairs.empty() ? nullptr : pairs[0].data(), 2 * pairs.size());
  put_i(tag + ".best", {best[0], best[1]});
  put_d(tag + ".best_cost", {cost});
}
static void put_path(const std::string &tag, ReplanSession &s) {
  std::vector<State> states;
  std::vector<Action> actions;
  const bool found = s.bestPath(states, actions);
  put_i(tag + ".found", {found ? 1 : 0});
  put(tag + ".states", 'd', states.empty() ? nullptr : states[0].data(), 8 * states.size());
  put(tag + ".actions", 'd', actions.empty() ? nullptr : actions[0].data(), 10 * actions.size());
  put_d(tag + ".length_yaw_cost", {found ? s.pathLength() : 0.0, found ? s.pathYaw() : 0.0,
                                   found ? s.pathCost() : 0.0, s.bestCost()});
}
static void put_graft(const std::string &tag, bool ok, const GraftStats &gs, const SharedStats &sh) {
  put_i(tag + ".ok", {ok ? 1 : 0});
  put_i(tag + ".graft", {gs.n_before, gs.n_kept, gs.n_candidates, gs.n_checked, gs.n_attached,
                         gs.n_outside, gs.n_edge_invalid, gs.n_inherited, gs.depth});
  put_i(tag + ".shared", {sh.n_before, sh.n_kept, sh.n_dropped_a, sh.n_dropped_b});
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
  const auto sv = get<double>(f, 48);
  const double radius = get<double>(f, 1)[0];
  const auto cfg = get<int32_t>(f, 3);
  const uint64_t seed = get<uint64_t>(f, 1)[0];
  std::fclose(f);
  State st[6];  // start, goal, root_a, root_b, goal_shift, bad
  for (int q = 0; q < 6; q++)
    for (int k = 0; k < 8; k++) st[q][k] = sv[8 * q + k];
  const int batch = cfg[0], H = cfg[1], H2 = cfg[2];
  try {
    Handle h1, h2;
    auto load = [&](Handle &h) {
      const int rc = gbp_terrain_create(0, nx, ny, x.data(), y.data(), z.data(),
                                        slopes ? dx.data() : nullptr, slopes ? dy.data() : nullptr,
                                        slopes ? dz.data() : nullptr, GBP_STORAGE_F64, &h.t);
      if (rc) throw gbp_amd::EngineError(rc, "gbp_terrain_create");
      return FastTerrainMap::borrow(h.t);
    };
    FastTerrainMap terrain = load(h1);
    ReplanSession s;
    s.begin(terrain, st[0], st[1], batch, 3.0, seed);
    BatchStats st1;
    s.search(1e9, H, &st1);
    put_state("s1", s);
    put_i("s1.counters", {st1.halves, st1.solutions, st1.rewires, s.nextHalf(), s.extendCounter()});
    // 1b: a root that is valid in no phase
    GraftStats gs;
    SharedStats sh;
    const bool off_bad = s.robotOff(st[5], radius, gs, &sh);
    const bool goal_bad = s.goalAt(st[5], radius, gs, &sh);
    put_i("s1b.ok", {off_bad ? 1 : 0, goal_bad ? 1 : 0});
    put_state("s1b", s);
    // 2: the robot is off the tree
    const bool ok2 = s.robotOff(st[2], radius, gs, &sh);
    put_graft("s2", ok2, gs, sh);
    put_state("s2", s);
    put_path("s2.path", s);
    // 3: the goal moved
    const bool ok3 = s.goalAt(st[3], radius, gs, &sh);
    put_graft("s3", ok3, gs, sh);
    put_state("s3", s);
    put_path("s3.path", s);
    put_i("s3.counters", {s.nextHalf(), s.extendCounter()});
    // 4: the search goes on
    BatchStats st4;
    s.search(1e9, H2, &st4);
    put_state("s4", s);
    put_i("s4.counters", {st4.halves, st4.solutions, st4.rewires, s.nextHalf(), s.extendCounter()});
    put_path("s4.path", s);
    s.end();
    // 5: a goal that nothing of the goal tree connects to
    {
      FastTerrainMap t2 = load(h2);
      ReplanSession s5;
      s5.begin(t2, st[0], st[1], batch, 3.0, seed);
      s5.search(1e9, H);
      const bool ok5 = s5.goalAt(st[4], radius, gs, &sh);
      put_graft("s5", ok5, gs, sh);
      put_state("s5", s5);
      put_path("s5.path", s5);
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "replan_graft_node: %s\n", e.what());
    return 1;
  }
  std::fclose(out_);
  return 0;
}
