// closed_forms_probe.cpp — the host statement of the planner's closed forms
// through its two kept surfaces, gbp_host:: (csrc/host/gbp_host_check.h) and
// gbp_amd::planning_utils:: (include/gbp_planner.h), for
// tests/test_closed_forms.py.  No engine, no device: linked with
// gbp_host_check.cpp and gbp_planning_math.cpp alone.
//
//   closed_forms_probe pairs IN OUT   every pair of IN through gbp_host::pair_check,
//                                     both directions, plain and adaptive
//   closed_forms_probe forms IN OUT   every row of IN through the closed forms
//
// IN and OUT are raw little-endian binary64 / uint32 records (the layouts are
// the structs below and the dtypes of the test).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "gbp.h"
#include "gbp_host_check.h"
#include "gbp_planner.h"

namespace pu = gbp_amd::planning_utils;

namespace {

struct PairOut {
  double s_new[8], t_new;
  uint32_t valid, flags, counts, pad;
};

struct FormRow {  // one input row
  double s[8], s2[8], a[10], t;
};

struct FormOut {
  double stance[8], flight[8], stance_rev[8];
  double sd_host, sd_pu, pd_host, pd_pu, yaw_pu;
  double connect[10];      // gbp_host::connect_action(s, s2, a[6])
  double ac_s_new[8], ac_a_new[10];
  int32_t va_host, va_pu, ac_result, pad;
};

bool read_all(FILE *f, void *p, size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }

bool read_terrain(FILE *f, gbp_host::Terrain &T) {
  double dims[2];
  if (!read_all(f, dims, sizeof dims)) return false;
  T.nx = (int)dims[0];
  T.ny = (int)dims[1];
  T.x.resize(T.nx);
  T.y.resize(T.ny);
  T.z.resize((size_t)T.nx * T.ny);
  return read_all(f, T.x.data(), 8 * T.x.size()) && read_all(f, T.y.data(), 8 * T.y.size()) &&
         read_all(f, T.z.data(), 8 * T.z.size());
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  FILE *in = std::fopen(argv[2], "rb"), *out = std::fopen(argv[3], "wb");
  if (!in || !out) return 2;
  gbp_host::Terrain T;
  double count;
  if (!read_terrain(in, T) || !read_all(in, &count, 8)) return 3;
  const size_t n = (size_t)count;
  if (!std::strcmp(argv[1], "pairs")) {
    std::vector<double> s(8 * n), a(10 * n);
    if (!read_all(in, s.data(), 8 * s.size()) || !read_all(in, a.data(), 8 * a.size())) return 3;
    std::vector<PairOut> o(n);
    for (int dir = 0; dir < 2; dir++)
      for (int adaptive = 0; adaptive < 2; adaptive++) {
        for (size_t k = 0; k < n; k++) {
          PairOut &r = o[k];
          std::memset(&r, 0x55, sizeof r);  // an unassigned output stays this pattern
          r.t_new = -7.0;
          r.pad = 0;
          r.valid = gbp_host::pair_check(T, &s[8 * k], &a[10 * k], dir, adaptive, r.s_new, &r.t_new,
                                         &r.flags, &r.counts);
        }
        if (std::fwrite(o.data(), sizeof(PairOut), n, out) != n) return 4;
      }
  } else if (!std::strcmp(argv[1], "forms")) {
    std::vector<FormRow> rows(n);
    if (!read_all(in, rows.data(), sizeof(FormRow) * n)) return 3;
    std::vector<FormOut> o(n);
    for (size_t k = 0; k < n; k++) {
      const FormRow &q = rows[k];
      FormOut &r = o[k];
      std::memset(&r, 0, sizeof r);
      pu::State s, s2;
      pu::Action a;
      std::memcpy(s.data(), q.s, sizeof q.s);
      std::memcpy(s2.data(), q.s2, sizeof q.s2);
      std::memcpy(a.data(), q.a, sizeof q.a);
      const pu::State st = pu::applyStance(s, a, q.t), fl = pu::applyFlight(s, q.t),
                      sr = pu::applyStanceReverse(s, a, q.t);
      std::memcpy(r.stance, st.data(), sizeof r.stance);
      std::memcpy(r.flight, fl.data(), sizeof r.flight);
      std::memcpy(r.stance_rev, sr.data(), sizeof r.stance_rev);
      r.sd_host = gbp_host::state_distance(q.s, q.s2);
      r.sd_pu = pu::stateDistance(s, s2);
      r.pd_host = gbp_host::pose_distance(q.s, q.s2);
      r.pd_pu = pu::poseDistance(s, s2);
      r.yaw_pu = pu::stateYawDistance(s, s2);
      r.va_host = gbp_host::is_valid_action(q.a);
      r.va_pu = pu::isValidAction(a);
      gbp_host::connect_action(q.s, q.s2, q.a[6], r.connect);
      // attemptConnect(s_existing = s, s = s2), t_s as rrt_connect.cpp:89 forms it;
      // direction and step size by row
      for (double &v : r.ac_s_new) v = std::numeric_limits<double>::quiet_NaN();  // unassigned
      for (double &v : r.ac_a_new) v = std::numeric_limits<double>::quiet_NaN();
      const double t_s = gbp_host::pose_distance(q.s2, q.s) / pu::V_NOM;
      r.ac_result = gbp_host::attempt_connect(T, q.s, q.s2, t_s, r.ac_s_new, r.ac_a_new, (int)(k & 1),
                                              (int)((k >> 1) & 1), GBP_CONNECT_MAX_DEPTH, nullptr);
    }
    if (std::fwrite(o.data(), sizeof(FormOut), n, out) != n) return 4;
  } else {
    return 2;
  }
  return std::fclose(out) == 0 ? 0 : 4;
}
