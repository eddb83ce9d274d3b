// planning_utils_probe.cpp — the closed forms and the path interpolation of the
// planner's public surface, gbp_amd::planning_utils:: (include/gbp_planner.h:
// csrc/host/gbp_planning_math.cpp and csrc/host/gbp_planner.cpp), for
// tests/test_reference_parity.py.  Linked against libgbp_planner.so; nothing
// here touches a device.
//
//   planning_utils_probe forms IN OUT   every row of IN through interp, applyAction, the
//                                       two-argument applyStance / applyStanceReverse, the
//                                       weighted stateDistance, isWithinBounds, rotate_grf
//   planning_utils_probe path IN OUT    getInterpPath of the path in IN
//
// IN and OUT are raw little-endian binary64 records (the layouts are the
// structs below and the dtypes of the test).
#include <cstdio>
#include <cstring>
#include <vector>

#include "gbp_planner.h"

namespace pu = gbp_amd::planning_utils;

namespace {

struct FormRow {
  double s[8], s2[8], a[10], t, n[3], f[3], lw, yw;
};

struct FormOut {
  double interp[8], action[8], stance[8], stance_rev[8];
  double sd_yaw, sd_plain, within;
  double grf[3];
};

bool read_all(FILE *f, void *p, size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }

template <class T>
T load(const double *p) {
  T v;
  std::memcpy(v.data(), p, sizeof(double) * v.size());
  return v;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 4) return 2;
  FILE *in = std::fopen(argv[2], "rb"), *out = std::fopen(argv[3], "wb");
  if (!in || !out) return 2;
  double count;
  if (!read_all(in, &count, 8)) return 3;
  const size_t n = (size_t)count;
  if (!std::strcmp(argv[1], "forms")) {
    std::vector<FormRow> rows(n);
    if (!read_all(in, rows.data(), sizeof(FormRow) * n)) return 3;
    std::vector<FormOut> o(n);
    for (size_t k = 0; k < n; k++) {
      const FormRow &q = rows[k];
      FormOut &r = o[k];
      const pu::State s = load<pu::State>(q.s), s2 = load<pu::State>(q.s2);
      const pu::Action a = load<pu::Action>(q.a);
      const pu::State ip = pu::interp(s, s2, q.t), ac = pu::applyAction(s, a),
                      st = pu::applyStance(s, a), sr = pu::applyStanceReverse(s, a);
      std::memcpy(r.interp, ip.data(), sizeof r.interp);
      std::memcpy(r.action, ac.data(), sizeof r.action);
      std::memcpy(r.stance, st.data(), sizeof r.stance);
      std::memcpy(r.stance_rev, sr.data(), sizeof r.stance_rev);
      r.sd_yaw = pu::stateDistance(s, s2, true, q.lw, q.yw);
      r.sd_plain = pu::stateDistance(s, s2, false, q.lw, q.yw);
      r.within = pu::isWithinBounds(s, s2) ? 1.0 : 0.0;
      const std::array<double, 3> g = pu::rotate_grf({q.n[0], q.n[1], q.n[2]}, {q.f[0], q.f[1], q.f[2]});
      std::memcpy(r.grf, g.data(), sizeof r.grf);
    }
    if (std::fwrite(o.data(), sizeof(FormOut), n, out) != n) return 4;
  } else if (!std::strcmp(argv[1], "path")) {
    // count = states n; then dt, 8 n state values, 10 (n - 1) action values
    double dt;
    std::vector<double> sv(8 * n), av(10 * (n - 1));
    if (n < 2 || !read_all(in, &dt, 8) || !read_all(in, sv.data(), 8 * sv.size()) ||
        !read_all(in, av.data(), 8 * av.size()))
      return 3;
    std::vector<pu::State> states, path;
    std::vector<pu::Action> actions;
    std::vector<double> ts;
    std::vector<int> phase;
    for (size_t k = 0; k < n; k++) states.push_back(load<pu::State>(&sv[8 * k]));
    for (size_t k = 0; k + 1 < n; k++) actions.push_back(load<pu::Action>(&av[10 * k]));
    pu::getInterpPath(states, actions, dt, path, ts, phase);
    // output: m, phases' count, then m rows of 8, m times, the phases as doubles
    const double head[2] = {(double)path.size(), (double)phase.size()};
    if (ts.size() != path.size() || std::fwrite(head, 8, 2, out) != 2) return 4;
    for (const pu::State &p : path)
      if (std::fwrite(p.data(), 8, 8, out) != 8) return 4;
    if (std::fwrite(ts.data(), 8, ts.size(), out) != ts.size()) return 4;
    for (int p : phase) {
      const double v = p;
      if (std::fwrite(&v, 8, 1, out) != 1) return 4;
    }
  } else {
    return 2;
  }
  std::fclose(in);
  return std::fclose(out) == 0 ? 0 : 4;
}
