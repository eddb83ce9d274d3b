// RRTClass::set_informed_cost (include/gbp_planner.h) for
// tests/test_gpu_informed_planner.py: the host-batched search and the
// device-resident one, both with the same informed cost, must draw the same
// targets and build the same trees; a third, plain host-batched run shows that
// the cost changes the draws.
//
//   informed_plan_node <input.bin> <output.bin>
// input:  int32 nx ny has_slopes; x[nx] y[ny] z[nx ny] (dx dy dz [nx ny]) f64;
//         start[8] goal[8] f64; int32 batch; uint64 seed; f64 cost
// output: per run (host informed, device informed, host plain):
//           int64 found targets extends attempts_checked connects vertices_a
//                 vertices_b n_states n_actions
//           f64 states[n_states][8] actions[n_actions][10]
//           per tree: int64 nv; f64 v[nv][8] a[nv][10] g[nv]; int32 parent[nv]
//         then int64 active: the handle's ellipse after the runs (0: restored)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gbp_planner_compat.h"

using gbp_amd::BatchStats;
using gbp_amd::TreeDump;

template <class T>
static std::vector<T> get(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
    std::fprintf(stderr, "short input\n");
    std::exit(3);
  }
  return v;
}

template <class T>
static void put(FILE *f, const T *p, size_t n) {
  if (n) std::fwrite(p, sizeof(T), n, f);
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  FILE *out = std::fopen(argv[2], "wb");
  if (!f || !out) return 2;
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
  const int batch = get<int32_t>(f, 1)[0];
  const uint64_t seed = get<uint64_t>(f, 1)[0];
  const double cost = get<double>(f, 1)[0];
  std::fclose(f);
  State s0, s1;
  std::copy(sg.begin(), sg.begin() + 8, s0.begin());
  std::copy(sg.begin() + 8, sg.end(), s1.begin());
  try {
    FastTerrainMap terrain(0);
    terrain.loadDataFlat(nx, ny, x.data(), y.data(), z.data(), slopes ? dx.data() : nullptr,
                         slopes ? dy.data() : nullptr, slopes ? dz.data() : nullptr);
    for (int run = 0; run < 3; run++) {
      RRTConnectClass planner;
      planner.setSeed(seed);
      planner.set_informed_cost(run < 2 ? cost : 0.0);
      if (planner.informedCost() != (run < 2 ? cost : 0.0)) return 4;
      std::vector<State> states;
      std::vector<Action> actions;
      BatchStats st;
      TreeDump dump;
      st.dump = &dump;
      const bool found = run == 1 ? planner.buildRRTConnectDevice(terrain, s0, s1, batch, 120.0,
                                                                  states, actions, &st)
                                  : planner.buildRRTConnectBatched(terrain, s0, s1, batch, 120.0,
                                                                   states, actions, &st);
      const int64_t head[9] = {found ? 1 : 0,       st.targets,    st.extends,
                               st.attempts_checked, st.connects,   st.vertices_a,
                               st.vertices_b,       (int64_t)states.size(), (int64_t)actions.size()};
      put(out, head, 9);
      put(out, states.empty() ? nullptr : states[0].data(), 8 * states.size());
      put(out, actions.empty() ? nullptr : actions[0].data(), 10 * actions.size());
      for (int k = 0; k < 2; k++) {
        const int64_t nv = (int64_t)dump.v[k].size();
        put(out, &nv, 1);
        put(out, nv ? dump.v[k][0].data() : nullptr, 8 * (size_t)nv);
        put(out, nv ? dump.a[k][0].data() : nullptr, 10 * (size_t)nv);
        put(out, dump.g[k].data(), (size_t)nv);
        put(out, dump.parent[k].data(), (size_t)nv);
      }
    }
    gbp_informed e{};
    if (gbp_terrain_get_informed(terrain.handle(), &e) != GBP_OK) return 5;
    const int64_t active = e.active;
    put(out, &active, 1);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "informed_plan_node: %s\n", e.what());
    return 1;
  }
  std::fclose(out);
  return 0;
}
