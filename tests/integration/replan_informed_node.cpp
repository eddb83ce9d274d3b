// ReplanSession::setInformed (include/gbp_planner.h) for
// tests/test_gpu_replan_informed.py, whose py_scenario writes the same records
// through planner.ReplanSession; the test compares the two and checks every
// record against the public entries.
//   P: a plain session, I: one with setInformed(true), a terrain handle each
//   1. both searched in calls of 2 halves until I holds a connection   first.*
//      (first.P.<c> / first.I.<c>: both states after call c)
//   2. I searched on to H halves                                       s200.*
//   3. search(1e9, 2): next half, targets so far                        nt
//   4. 50 calls of 2 halves                                            costs, stat_targets
//   5. bestPath with the property on, off, on                          p_on / p_off / p_on2
//   6. robotAt(the path's second state)                                robot.*
//   7. the map set to NaN, mapChanged                                  map.*
//   8. end                                                             inf_end
// An ellipse is recorded as 8 doubles: active cost cx cy ux uy a b.
//
//   replan_informed_node <input.bin> <output.bin>
// input:  int32 nx ny has_slopes; x[nx] y[ny] z[nx ny] (dx dy dz [nx ny]) f64;
//         start[8] goal[8] f64; int32 batch H; uint64 seed
// output: records (uint32 name length, name, char 'd' | 'i' | 'q', int64 count, data)
#include <cmath>
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
  put_d(tag + ".length_yaw_cost", {s.pathLength(), s.pathYaw(), s.pathCost(), s.bestCost()});
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

static void put_inf(const std::string &name, const gbp_informed &e) {
  put_d(name, {(double)e.active, e.cost, e.cx, e.cy, e.ux, e.uy, e.a, e.b});
}
static gbp_informed handle_inf(gbp_terrain *t) {
  gbp_informed e{};
  if (gbp_terrain_get_informed(t, &e) != GBP_OK) throw gbp_amd::EngineError(GBP_E_BAD_HANDLE, "get_informed");
  return e;
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
  const auto sg = get<double>(f, 16);
  const auto cfg = get<int32_t>(f, 2);
  const uint64_t seed = get<uint64_t>(f, 1)[0];
  std::fclose(f);
  State start, goal;
  for (int k = 0; k < 8; k++) {
    start[k] = sg[k];
    goal[k] = sg[8 + k];
  }
  const int batch = cfg[0], H = cfg[1];
  try {
    Handle h, h2;
    auto load = [&](Handle &to) {
      const int rc = gbp_terrain_create(0, nx, ny, x.data(), y.data(), z.data(),
                                        slopes ? dx.data() : nullptr, slopes ? dy.data() : nullptr,
                                        slopes ? dz.data() : nullptr, GBP_STORAGE_F64, &to.t);
      if (rc) throw gbp_amd::EngineError(rc, "gbp_terrain_create");
      return FastTerrainMap::borrow(to.t);
    };
    FastTerrainMap terrain = load(h), terrain2 = load(h2);
    // what end() has to put back: an inactive record that is not all zero
    gbp_informed mark{};
    mark.cost = 42.0;
    mark.a = 1.5;
    if (gbp_terrain_set_informed(h2.t, &mark) != GBP_OK) return 4;
    ReplanSession P, I;
    I.setInformed(true);
    put_i("flags", {P.informed() ? 1 : 0, I.informed() ? 1 : 0});
    P.begin(terrain, start, goal, batch, 3.0, seed);
    I.begin(terrain2, start, goal, batch, 3.0, seed);
    put_inf("inf_begin", I.informedState());
    // 1. until the informed session holds a connection
    std::vector<int64_t> sizes_p, sizes_i;
    bool held = false;
    int calls = 0;
    while (!held && calls < H / 2) {
      BatchStats sp, si;
      P.search(1e9, 2, &sp);
      held = I.search(1e9, 2, &si);
      calls++;
      put_state("first.P." + std::to_string(calls), P);  // every dump and list on the way
      put_state("first.I." + std::to_string(calls), I);
      sizes_p.insert(sizes_p.end(), {sp.vertices_a, sp.vertices_b, sp.solutions, P.extendCounter()});
      sizes_i.insert(sizes_i.end(), {si.vertices_a, si.vertices_b, si.solutions, I.extendCounter()});
    }
    put_i("first.calls", {calls, held ? 1 : 0});
    put_i("first.sizes_p", sizes_p);
    put_i("first.sizes_i", sizes_i);
    put_state("first.P", P);
    put_state("first.I", I);
    put_inf("first.inf", I.informedState());
    P.end();
    // 2. on to H halves
    BatchStats s2;
    if (H > 2 * calls) I.search(1e9, H - 2 * calls, &s2);
    put_state("s200", I);
    put_inf("s200.inf", I.informedState());
    put_i("s200.half", {I.nextHalf(), s2.targets});
    // 3. one more group of 2 halves under that ellipse
    {
      BatchStats st;
      I.search(1e9, 2, &st);
      put_i("nt", {I.nextHalf(), st.targets});
    }
    // 4. 100 further halves
    std::vector<double> costs;
    std::vector<int64_t> targets;
    for (int c = 0; c < 50; c++) {
      BatchStats st;
      I.search(1e9, 2, &st);
      costs.push_back(I.bestCost());
      targets.push_back(st.targets);
    }
    put_d("costs", costs);
    put_i("stat_targets", targets);
    // 5. the property toggled
    put_path("p_on", I);
    put_inf("p_on.inf", I.informedState());
    I.setInformed(false);
    put_inf("p_off.inf", I.informedState());
    put_path("p_off", I);
    I.setInformed(true);
    put_inf("p_on2.inf", I.informedState());
    put_path("p_on2", I);
    // 6. the robot on the path's second state
    {
      std::vector<State> states;
      std::vector<Action> actions;
      if (!I.bestPath(states, actions) || states.size() < 2) return 5;
      RerootStats rs;
      I.robotAt(states[1], rs);
      put_state("robot", I);
      put_inf("robot.inf", I.informedState());
    }
    // 7. a map that drops every connection
    {
      const std::vector<double> nan_z((size_t)nx * ny, std::nan(""));
      const int rc = gbp_terrain_update_host(h2.t, nullptr, GBP_SRC_F64_XMAJOR, ny, nan_z.data(),
                                             nullptr, nullptr, nullptr);
      if (rc) throw gbp_amd::EngineError(rc, "gbp_terrain_update_host");
      PruneStats ps[2];
      I.mapChanged(terrain2, ps);
      put_state("map", I);
      put_inf("map.inf", I.informedState());
    }
    // 8. end
    I.end();
    put_inf("inf_end", handle_inf(h2.t));
    put_i("flags_end", {I.informed() ? 1 : 0});
  } catch (const std::exception &e) {
    std::fprintf(stderr, "replan_informed_node: %s\n", e.what());
    return 1;
  }
  std::fclose(out_);
  return 0;
}
