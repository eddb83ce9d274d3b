// ReplanSession::trim and setTreeLimit (include/gbp_planner.h) for
// tests/test_gpu_replan_trim.py, which compares every record with the oracle's
// and the numpy restatement's values (tests/trim_ref.py):
//   per budget B:  begin + search(H halves), bestPath, trim(B), bestPath,
//                  search(H2 halves)                         records t<B>.*
//   the limit:     a session with setTreeLimit(limit, trim_to) and one without,
//                  both searched in `calls` calls of 2 halves; on the second the
//                  program itself calls trim(trim_to) after every call that
//                  leaves a tree above the limit             records L.* / M.*
//
//   replan_trim_node <input.bin> <output.bin>
// input:  int32 nx ny has_slopes; x[nx] y[ny] z[nx ny] (dx dy dz [nx ny]) f64;
//         start[8] goal[8] f64; int32 batch H H2 calls limit trim_to nb;
//         int32 budgets[nb]; uint64 seed
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
  put_d(tag + ".length_yaw_cost", {s.pathLength(), s.pathYaw(), s.pathCost(), s.bestCost()});
}
static void put_trim(const std::string &tag, const TrimStats ts[2], const SharedStats &sh) {
  for (int k = 0; k < 2; k++) {
    put_i(tag + (k ? ".b" : ".a"), {ts[k].n_before, ts[k].n_kept, ts[k].n_over_bound, ts[k].n_over_budget,
                                    ts[k].n_protected, ts[k].n_inherited});
    put_d(tag + (k ? ".b.cut" : ".a.cut"), {ts[k].cut});
  }
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
  const auto sg = get<double>(f, 16);
  const auto cfg = get<int32_t>(f, 7);
  const auto budgets = get<int32_t>(f, (size_t)cfg[6]);
  const uint64_t seed = get<uint64_t>(f, 1)[0];
  std::fclose(f);
  State start, goal;
  for (int k = 0; k < 8; k++) {
    start[k] = sg[k];
    goal[k] = sg[8 + k];
  }
  const int batch = cfg[0], H = cfg[1], H2 = cfg[2], calls = cfg[3], limit = cfg[4], trim_to = cfg[5];
  try {
    Handle h, h2;  // (the two sessions of the limit's part search in turns: a handle each)
    auto load = [&](Handle &to) {
      const int rc = gbp_terrain_create(0, nx, ny, x.data(), y.data(), z.data(),
                                        slopes ? dx.data() : nullptr, slopes ? dy.data() : nullptr,
                                        slopes ? dz.data() : nullptr, GBP_STORAGE_F64, &to.t);
      if (rc) throw gbp_amd::EngineError(rc, "gbp_terrain_create");
      return FastTerrainMap::borrow(to.t);
    };
    FastTerrainMap terrain = load(h), terrain2 = load(h2);
    for (int32_t B : budgets) {
      const std::string tag = "t" + std::to_string(B);
      ReplanSession s;
      s.begin(terrain, start, goal, batch, 3.0, seed);
      s.search(1e9, H);
      put_state(tag + ".s1", s);
      put_path(tag + ".p1", s);
      TrimStats ts[2];
      SharedStats sh;
      s.trim(B, ts, &sh);
      put_trim(tag + ".trim", ts, sh);
      put_state(tag + ".s2", s);
      put_path(tag + ".p2", s);
      put_i(tag + ".counters2", {s.nextHalf(), s.extendCounter()});
      BatchStats st;
      s.search(1e9, H2, &st);
      put_state(tag + ".s3", s);
      put_i(tag + ".counters3", {st.halves, st.solutions, st.rewires, s.nextHalf(), s.extendCounter()});
    }
    // the limit inside search against the same trims made from outside
    ReplanSession L, M;
    bool refused = false;
    try {
      L.setTreeLimit(limit, limit + 1);
    } catch (const gbp_amd::EngineError &) {
      refused = true;
    }
    try {
      L.setTreeLimit(limit, 0);
      refused = false;
    } catch (const gbp_amd::EngineError &) {
    }
    put_i("L.refused", {refused ? 1 : 0, L.treeLimit()});
    L.setTreeLimit(limit, trim_to);
    L.begin(terrain, start, goal, batch, 3.0, seed);
    M.begin(terrain2, start, goal, batch, 3.0, seed);
    std::vector<int64_t> sizes_l, sizes_m;
    int64_t trims_m = 0;
    for (int c = 0; c < calls; c++) {
      BatchStats sl, sm;
      L.search(1e9, 2, &sl);
      M.search(1e9, 2, &sm);
      if (sm.vertices_a > limit || sm.vertices_b > limit) {
        TrimStats ts[2];
        M.trim(trim_to, ts);
        trims_m++;
        sm.vertices_a = ts[0].n_kept;
        sm.vertices_b = ts[1].n_kept;
      }
      sizes_l.insert(sizes_l.end(), {sl.vertices_a, sl.vertices_b});
      sizes_m.insert(sizes_m.end(), {sm.vertices_a, sm.vertices_b});
    }
    put_state("L", L);
    put_state("M", M);
    put_path("L.path", L);
    put_path("M.path", M);
    put_i("L.sizes", sizes_l);
    put_i("M.sizes", sizes_m);
    put_i("L.counters", {L.trimsBySearch(), L.nextHalf(), L.extendCounter()});
    put_i("M.counters", {trims_m, M.nextHalf(), M.extendCounter()});
  } catch (const std::exception &e) {
    std::fprintf(stderr, "replan_trim_node: %s\n", e.what());
    return 1;
  }
  std::fclose(out_);
  return 0;
}
