// gbp_host_check.cpp — glibc re-decision of FRAGILE attempts (see the header).
// Built with g++ -O3 -ffp-contract=off: the reference's x86-64 arithmetic, the
// reference's libm.  The terrain lookups and isValidState are stated here, with
// glibc's atan2 / cos / sin; the closed forms and the pair checks' sample loops
// are the one statement of gbp_closed_forms.h, compiled here by g++ and handed
// out through the out-of-line functions of the header.  Every function
// follows the reference source line by line;
// the only departures are the engine conventions every engine path shares
// (gbp.h): an undefined out-of-map lookup makes the state invalid (GBP_F_OOD),
// a check is stopped after GBP_MAX_SAMPLES states (GBP_F_LIMIT).
#include "gbp_host_check.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../gbp_closed_forms.h"
#include "gbp.h"

namespace gbp_host {

// planning_utils.h:21-66, stated once in gbp_closed_forms.h
using gbp::H_MAX, gbp::H_MIN, gbp::V_MAX, gbp::P_MAX, gbp::ROBOT_L, gbp::ROBOT_W, gbp::ROBOT_H,
    gbp::KINEMATICS_RES;

namespace {

constexpr int NO_BRACKET_LOW = -1;   // v < d[0] or NaN: the scan never matches, index 0
constexpr int NO_BRACKET_HIGH = -2;  // v >= d[n-1]: the scan reads d[n] (undefined)

// fast_terrain_map.cpp:101-117: the first i with d[i] <= v < d[i+1]; for an
// ascending vector that is the last i with d[i] <= v, if v < d[n-1]
int bracket(const std::vector<double> &d, double v) {
  const int n = (int)d.size();
  if (!(v >= d[0])) return NO_BRACKET_LOW;
  if (v >= d[n - 1]) return NO_BRACKET_HIGH;
  return (int)(std::upper_bound(d.begin(), d.end(), v) - d.begin()) - 1;
}

double zc(const Terrain &T, int ix, int iy) { return T.z[(size_t)ix * T.ny + iy]; }

// fast_terrain_map.cpp:135-157; -1 = undefined (a scan read past the end)
int height_is_nan(const Terrain &T, double x, double y) {
  const int ix = bracket(T.x, x), iy = bracket(T.y, y);
  if (ix == NO_BRACKET_HIGH || iy == NO_BRACKET_HIGH) return -1;
  const int cx = ix < 0 ? 0 : ix, cy = iy < 0 ? 0 : iy;
  return (std::isnan(zc(T, cx, cy)) || std::isnan(zc(T, cx, cy + 1)) ||
          std::isnan(zc(T, cx + 1, cy)) || std::isnan(zc(T, cx + 1, cy + 1)))
             ? 1
             : 0;
}

// fast_terrain_map.cpp:94-132; false = undefined (finite point with no bracket)
bool ground_height(const Terrain &T, double x, double y, double &h) {
  if (std::isnan(x) || std::isnan(y)) {  // every term is NaN whatever x1..y2 hold
    h = NAN;
    return true;
  }
  const int ix = bracket(T.x, x), iy = bracket(T.y, y);
  if (ix < 0 || iy < 0) return false;
  const double x1 = T.x[ix], x2 = T.x[ix + 1], y1 = T.y[iy], y2 = T.y[iy + 1];
  const double fx1y1 = zc(T, ix, iy), fx1y2 = zc(T, ix, iy + 1);
  const double fx2y1 = zc(T, ix + 1, iy), fx2y2 = zc(T, ix + 1, iy + 1);
  h = 1.0 / ((x2 - x1) * (y2 - y1)) *
      (fx1y1 * (x2 - x) * (y2 - y) + fx2y1 * (x - x1) * (y2 - y) + fx1y2 * (x2 - x) * (y - y1) +
       fx2y2 * (x - x1) * (y - y1));
  return true;
}

}  // namespace

bool is_valid_state(const Terrain &T, const double s[8], int phase, Acc &acc) {
  if (acc.V >= GBP_MAX_SAMPLES) {  // engine guard (gbp.h GBP_F_LIMIT)
    acc.flags |= GBP_F_LIMIT;
    return false;
  }
  acc.V++;
  const double x0 = T.x.front(), xN = T.x.back(), y0 = T.y.front(), yN = T.y.back();
  // :564 heightIsNan(centre); an undefined read matters only where (2) passes
  const int r = height_is_nan(T, s[0], s[1]);
  if (r < 0) {
    if (!(s[0] < x0 || s[0] > xN || s[1] < y0 || s[1] > yN)) acc.flags |= GBP_F_OOD;
    return false;
  }
  if (r) {
    acc.flags |= GBP_F_NAN;
    return false;
  }
  // :568-571 (abs resolves to the double overload)
  if ((s[0] < x0) || (s[0] > xN) || (s[1] < y0) || (s[1] > yN) || (std::fabs(s[6]) >= P_MAX))
    return false;
  // :574
  if (std::sqrt(s[3] * s[3] + s[4] * s[4]) > V_MAX) return false;
  // :578-594
  const double yaw = std::atan2(s[4], s[3]);
  const double cy = std::cos(yaw);
  const double sy = std::sin(yaw);
  const double pitch = s[6];
  const double cp = std::cos(pitch);
  const double sp = std::sin(pitch);
  const double R_11 = cy * cp, R_12 = -sy, R_13 = cy * sp;
  const double R_21 = sy * cp, R_22 = cy, R_23 = sy * sp;
  const double R_31 = -sp, R_32 = 0, R_33 = cp;
  const double test_x[2] = {-0.5 * ROBOT_L, 0.5 * ROBOT_L};
  const double test_y[2] = {-0.5 * ROBOT_W, 0.5 * ROBOT_W};
  const double z_body = -ROBOT_H;
  // :601-627
  for (double x_body : test_x) {
    for (double y_body : test_y) {
      const double x_leg = s[0] + R_11 * x_body + R_12 * y_body;
      const double y_leg = s[1] + R_21 * x_body + R_22 * y_body;
      const double z_leg = s[2] + R_31 * x_body + R_32 * y_body;
      const double x_corner = x_leg + R_13 * z_body;
      const double y_corner = y_leg + R_23 * z_body;
      const double z_corner = z_leg + R_33 * z_body;
      const int rl = height_is_nan(T, x_leg, y_leg);
      if (rl < 0) {
        acc.flags |= GBP_F_OOD;
        return false;
      }
      if (rl) {
        acc.flags |= GBP_F_NAN;
        return false;
      }
      acc.G += 2;  // both heights are computed before the test (:618-619)
      double gl, gc;
      if (!ground_height(T, x_leg, y_leg, gl) || !ground_height(T, x_corner, y_corner, gc)) {
        acc.flags |= GBP_F_OOD;
        return false;
      }
      const double leg_height = z_leg - gl;
      const double corner_height = z_corner - gc;
      if ((corner_height < H_MIN) || ((phase == GBP_STANCE) && (leg_height > H_MAX))) return false;
    }
  }
  // :630-632
  acc.G++;
  double gu;
  if (!ground_height(T, s[0] + R_13 * z_body, s[1] + R_23 * z_body, gu)) {
    acc.flags |= GBP_F_OOD;
    return false;
  }
  const double height = (s[2] + R_33 * z_body) - gu;
  if (height < H_MIN) return false;
  return true;
}

bool pair_check(const Terrain &T, const double s[8], const double a[10], int direction,
                int adaptive, double s_new[8], double *t_new, uint32_t *flags, uint32_t *counts) {
  Acc acc;
  uint32_t f = 0;
  bool v;  // the shared loops (gbp_closed_forms.h) over is_valid_state above
  if (direction == GBP_FORWARD)
    v = adaptive ? gbp::pair_forward<true>(T, s, a, s_new, *t_new, acc, f)
                 : gbp::pair_forward<false>(T, s, a, s_new, *t_new, acc, f);
  else
    v = adaptive ? gbp::pair_reverse<true>(T, s, a, s_new, *t_new, acc, f)
                 : gbp::pair_reverse<false>(T, s, a, s_new, *t_new, acc, f);
  f |= acc.flags | (v ? GBP_F_VALID : 0u);
  if (flags) *flags = f;
  if (counts) *counts = (acc.G & 0xFFFFu) | (acc.V << 16);
  return v;
}

// the closed forms of gbp_closed_forms.h, out of line: what the host code of
// the .hip units calls, so that g++ and glibc form every value of a re-decision
double state_distance(const double *q1, const double *q2) { return gbp::state_distance(q1, q2); }

double pose_distance(const double *q1, const double *q2) { return gbp::pose_distance(q1, q2); }

bool is_valid_action(const double a[10]) { return gbp::is_valid_action(a); }

void connect_action(const double *s_start, const double *s_goal, double t_s, double a[10]) {
  gbp::connect_action(s_start, s_goal, t_s, a);
}

int attempt_connect(const Terrain &T, const double *s_existing, const double *s0, double t_s,
                    double s_new[8], double a_new[10], int direction, int adaptive, int max_depth,
                    uint32_t *flags) {
  double s[8];
  std::memcpy(s, s0, sizeof s);
  uint32_t fl = 0;
  int result = GBP_TRAPPED;
  for (int depth = 0;; depth++) {
    if (depth > max_depth) {  // engine convention: the reference recursion is unbounded
      fl |= GBP_F_DEPTH_CAPPED;
      break;
    }
    if (t_s <= KINEMATICS_RES) break;  // :23-24
    const double *s_start = direction == GBP_FORWARD ? s_existing : s;
    const double *s_goal = direction == GBP_FORWARD ? s : s_existing;
    connect_action(s_start, s_goal, t_s, a_new);
    if (!is_valid_action(a_new)) break;  // :66, :83
    double sn[8], tn = 0;
    uint32_t f = 0;
    const bool ok = pair_check(T, direction == GBP_FORWARD ? s_start : s_goal, a_new, direction,
                               adaptive, sn, &tn, &f, nullptr);
    fl |= f & (GBP_F_OOD | GBP_F_NAN | GBP_F_LIMIT);
    if (f & GBP_F_SNEW_SET) std::memcpy(s_new, sn, sizeof sn);
    if (ok) {
      result = depth == 0 ? GBP_REACHED : GBP_ADVANCED;  // :74-75, :79-80
      break;
    }
    // :77 recurse toward the returned state; unassigned t_new / s_new: TRAPPED
    if (!(f & GBP_F_TNEW_SET) || !(f & GBP_F_SNEW_SET)) break;
    std::memcpy(s, sn, sizeof s);
    t_s = tn;
  }
  if (flags) *flags = fl;
  return result;
}

}  // namespace gbp_host

// the reference's yaw of a state with glibc (planning_utils.h:135-136), for the
// device's yaw-weighted k-nearest (gbp_knn_yaw_batch_dev takes the yaws)
extern "C" __attribute__((visibility("default"))) double gbp_host_yaw(const double *s) {
  return std::atan2(s[4], s[3]);
}
