// gbp_closed_forms.h — the planner's closed forms, stated once for the device
// and the host: the constants, the propagation, isValidAction, the distances,
// the connect action and the sample loops of the pair checks.
//
// Plain C++17 on const double * / double *.  hipcc compiles it into the kernels
// (gbp_device.h, gbp_plan_dev.h); g++ compiles the same text into the host
// files under host/ (gbp_host_check.cpp, gbp_planning_math.cpp,
// gbp_shortcut_walk.cpp, gbp_planner.cpp), which include it by relative path.
// Everything is FP64 in the reference's operation order and must be built
// without FMA contraction: the pragma below does that for clang, and for g++
// the build flags give -ffp-contract=off (csrc/Makefile HCFLAGS / PFLAGS and
// every stand-alone build line).
//
// The rule of the FRAGILE re-decision: its arithmetic is compiled
// by g++ against glibc, never by hipcc's host pass.  The host code of the .hip
// units therefore keeps calling gbp_host::… (gbp_host_check.h, out of line in
// gbp_host_check.cpp) and nothing of this header, although hipcc would accept
// these functions on the host.
//
// Reference citations are given per function (paths relative to the reference
// repository root).
#pragma once
#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <cmath>
#include <stdint.h>

#include "gbp.h"

// GBP_HD: every function here.  GBP_HD_LOOP: the two pair loops, which the
// kernels call out of line (a forced inline would move the validate kernel's
// instructions).
#ifdef __HIPCC__
#define GBP_HD __host__ __device__ __forceinline__
#define GBP_HD_LOOP __host__ __device__
#else
#define GBP_HD inline
#define GBP_HD_LOOP inline
#endif
#ifdef __clang__
#define GBP_UNROLL _Pragma("unroll")
#else
#define GBP_UNROLL
#endif

namespace gbp {

// ---- constants: include/global_body_planner/planning_utils.h:21-66 --------
constexpr double H_MAX = 0.4;
constexpr double H_MIN = 0.075;
constexpr double V_MAX = 2.0;
constexpr double V_NOM = 0.75;
constexpr double P_MAX = 1.0;
constexpr double ANG_ACC_MAX = 7.0;
constexpr double ROBOT_L = 0.3;
constexpr double ROBOT_W = 0.3;
constexpr double ROBOT_H = 0.05;
constexpr double M_CONST = 13;
constexpr double G_CONST = 9.81;
constexpr double F_MAX = 637;
constexpr double MU = 1.0;
constexpr double T_F_MAX = 0.5;
constexpr double T_F_MIN = 0.0;
constexpr double KINEMATICS_RES = 0.05;
constexpr double BACKUP_RATIO = 0.5;
constexpr double GOAL_BOUNDS = 0.5;
constexpr double MY_PI = 3.14159;

GBP_HD double std_min(double a, double b) { return (b < a) ? b : a; }
GBP_HD double std_max(double a, double b) { return (a < b) ? b : a; }

// stance divisions x / (6 t_s), x / (2 t_s) (Markstein with a constant
// reciprocal was measured: no faster than the hardware-assisted sequence)
GBP_HD double pdiv(double x, double d) {
  return x / d;
}
#define PDIV6(x) pdiv((x), 6.0 * t_s)
#define PDIV2(x) pdiv((x), 2.0 * t_s)
// ---- propagation --------------------------------------------------------------
// The forms write o[k] as they go: o must not alias s (no caller passes it).
// planning_utils.cpp:237-274
GBP_HD void apply_stance(const double *s, const double *a, double t, double *o) {
  const double a_x_td = a[0], a_y_td = a[1], a_z_td = a[2];
  const double a_x_to = a[3], a_y_to = a[4], a_z_to = a[5];
  const double t_s = a[6], a_p_td = a[8], a_p_to = a[9];
  o[0] = s[0] + s[3] * t + 0.5 * a_x_td * t * t + PDIV6((a_x_to - a_x_td) * (t * t * t));
  o[1] = s[1] + s[4] * t + 0.5 * a_y_td * t * t + PDIV6((a_y_to - a_y_td) * (t * t * t));
  o[2] = s[2] + s[5] * t + 0.5 * a_z_td * t * t + PDIV6((a_z_to - a_z_td) * (t * t * t));
  o[3] = s[3] + a_x_td * t + PDIV2((a_x_to - a_x_td) * t * t);
  o[4] = s[4] + a_y_td * t + PDIV2((a_y_to - a_y_td) * t * t);
  o[5] = s[5] + a_z_td * t + PDIV2((a_z_to - a_z_td) * t * t);
  o[6] = s[6] + s[7] * t + 0.5 * a_p_td * t * t + PDIV6((a_p_to - a_p_td) * (t * t * t));
  o[7] = s[7] + a_p_td * t + PDIV2((a_p_to - a_p_td) * t * t);
}

// planning_utils.cpp:282-306 (g is the literal 9.81)
GBP_HD void apply_flight(const double *s, double t_f, double *o) {
  const double g = 9.81;
  o[0] = s[0] + s[3] * t_f;
  o[1] = s[1] + s[4] * t_f;
  o[2] = s[2] + s[5] * t_f - 0.5 * g * t_f * t_f;
  o[3] = s[3];
  o[4] = s[4];
  o[5] = s[5] - g * t_f;
  o[6] = s[6] + s[7] * t_f;
  o[7] = s[7];
}

// planning_utils.cpp:324-367 (s_new[7] before s_new[6], as written)
GBP_HD void apply_stance_reverse(const double *s, const double *a, double t, double *o) {
  const double a_x_td = a[0], a_y_td = a[1], a_z_td = a[2];
  const double a_x_to = a[3], a_y_to = a[4], a_z_to = a[5];
  const double t_s = a[6], a_p_td = a[8], a_p_to = a[9];
  const double cx = s[3] - a_x_td * t_s - 0.5 * (a_x_to - a_x_td) * t_s;
  const double cy = s[4] - a_y_td * t_s - 0.5 * (a_y_to - a_y_td) * t_s;
  const double cz = s[5] - a_z_td * t_s - 0.5 * (a_z_to - a_z_td) * t_s;
  const double cp = s[7] - a_p_td * t_s - 0.5 * (a_p_to - a_p_td) * t_s;
  const double d1 = t_s - t, d2 = t_s * t_s - t * t, d3 = t_s * t_s * t_s - t * t * t;
  o[0] = s[0] - cx * d1 - 0.5 * a_x_td * d2 - PDIV6((a_x_to - a_x_td) * d3);
  o[1] = s[1] - cy * d1 - 0.5 * a_y_td * d2 - PDIV6((a_y_to - a_y_td) * d3);
  o[2] = s[2] - cz * d1 - 0.5 * a_z_td * d2 - PDIV6((a_z_to - a_z_td) * d3);
  o[3] = s[3] - a_x_td * d1 - PDIV2((a_x_to - a_x_td) * d2);
  o[4] = s[4] - a_y_td * d1 - PDIV2((a_y_to - a_y_td) * d2);
  o[5] = s[5] - a_z_td * d1 - PDIV2((a_z_to - a_z_td) * d2);
  o[7] = s[7] - a_p_td * d1 - PDIV2((a_p_to - a_p_td) * d2);
  o[6] = s[6] - cp * d1 - 0.5 * a_p_td * d2 - PDIV6((a_p_to - a_p_td) * d3);
}

// planning_utils.cpp:519-556
GBP_HD bool is_valid_action(const double *a) {
  if ((a[6] <= 0) || (a[7] < 0)) return false;
  const double m = M_CONST, g = G_CONST, mu = MU;
  const double f_x_td = m * a[0], f_y_td = m * a[1], f_z_td = m * (a[2] + g);
  const double f_x_to = m * a[3], f_y_to = m * a[4], f_z_to = m * (a[5] + g);
  if ((sqrt(f_x_td * f_x_td + f_y_td * f_y_td + f_z_td * f_z_td) >= F_MAX) ||
      (sqrt(f_x_to * f_x_to + f_y_to * f_y_to + f_z_to * f_z_to) >= F_MAX) || (f_z_td < 0) ||
      (f_z_to < 0) || (a[8] >= F_MAX) || (a[9] >= F_MAX))
    return false;
  if ((sqrt(f_x_td * f_x_td + f_y_td * f_y_td) >= mu * f_z_td) ||
      (sqrt(f_x_to * f_x_to + f_y_to * f_y_to) >= mu * f_z_to))
    return false;
  return true;
}

// rrt_connect.cpp:53-63 (the cubic-Hermite stance action, t_f = 0)
GBP_HD void connect_action(const double *s_start, const double *s_goal, double t_s, double *a) {
  const double x_td = s_start[0], y_td = s_start[1], z_td = s_start[2];
  const double dx_td = s_start[3], dy_td = s_start[4], dz_td = s_start[5];
  const double x_to = s_goal[0], y_to = s_goal[1], z_to = s_goal[2];
  const double dx_to = s_goal[3], dy_to = s_goal[4], dz_to = s_goal[5];
  const double p_td = s_start[6], dp_td = s_start[7], p_to = s_goal[6], dp_to = s_goal[7];
  a[0] = -(2.0 * (3.0 * x_td - 3.0 * x_to + 2.0 * dx_td * t_s + dx_to * t_s)) / (t_s * t_s);
  a[1] = -(2.0 * (3.0 * y_td - 3.0 * y_to + 2.0 * dy_td * t_s + dy_to * t_s)) / (t_s * t_s);
  a[2] = -(2.0 * (3.0 * z_td - 3.0 * z_to + 2.0 * dz_td * t_s + dz_to * t_s)) / (t_s * t_s);
  a[3] = (2.0 * (3.0 * x_td - 3.0 * x_to + dx_td * t_s + 2.0 * dx_to * t_s)) / (t_s * t_s);
  a[4] = (2.0 * (3.0 * y_td - 3.0 * y_to + dy_td * t_s + 2.0 * dy_to * t_s)) / (t_s * t_s);
  a[5] = (2.0 * (3.0 * z_td - 3.0 * z_to + dz_td * t_s + 2.0 * dz_to * t_s)) / (t_s * t_s);
  a[6] = t_s;
  a[7] = 0;
  a[8] = -(2.0 * (3.0 * p_td - 3.0 * p_to + 2.0 * dp_td * t_s + dp_to * t_s)) / (t_s * t_s);
  a[9] = (2.0 * (3.0 * p_td - 3.0 * p_to + dp_td * t_s + 2.0 * dp_to * t_s)) / (t_s * t_s);
}

GBP_HD uint32_t stage_bits(uint32_t k) { return k << GBP_F_STAGE_SHIFT; }

// ---- pair checks, one sample after the other (the "direct" form) -------------
// TV is the terrain and ACC the counters (G, V, flags) of the caller's
// is_valid_state(T, sc, phase, acc), found by argument-dependent lookup: the
// kernels' branch-free check for TerrainView<ZT> (gbp_device.h), glibc's for
// gbp_host::Terrain (gbp_host_check.cpp).  The plain loop is the adaptive one
// with the step pinned to KINEMATICS_RES.
// planning_utils.cpp:713-753 (plain) and :651-712 (adaptive)
template <bool ADAPTIVE, class TV, class ACC>
GBP_HD_LOOP bool pair_forward(const TV &T, const double *s, const double *a, double *s_new,
                              double &t_new, ACC &acc, uint32_t &f) {
  const double t_s = a[6], t_f = a[7];
  double sc[8];
  double time_step = KINEMATICS_RES, t_pre_success = 0;
  f = (f & ~GBP_F_STAGE_MASK) | stage_bits(GBP_STAGE_FWD_STANCE);
  for (double t = 0; t <= t_s; t += (ADAPTIVE ? time_step : KINEMATICS_RES)) {
    apply_stance(s, a, t, sc);
    if (!is_valid_state(T, sc, GBP_STANCE, acc)) {
      if (acc.flags & GBP_F_LIMIT) return false;
      if (!ADAPTIVE || (KINEMATICS_RES - 0.01 <= time_step && time_step <= KINEMATICS_RES + 0.01)) {
        apply_stance(s, a, (1.0 - BACKUP_RATIO) * t, s_new);
        f |= GBP_F_SNEW_SET;
        return false;
      }
      time_step = KINEMATICS_RES;
      t = t_pre_success;
    } else {
      GBP_UNROLL
      for (int k = 0; k < 8; k++) s_new[k] = sc[k];
      t_new = t;
      f |= GBP_F_SNEW_SET | GBP_F_TNEW_SET;
      if (ADAPTIVE) {
        time_step += KINEMATICS_RES;
        t_pre_success = t;
      }
    }
  }
  double s_takeoff[8];
  apply_stance(s, a, a[6], s_takeoff);
  time_step = KINEMATICS_RES;
  f = (f & ~GBP_F_STAGE_MASK) | stage_bits(GBP_STAGE_FWD_FLIGHT);
  for (double t = 0; t < t_f; t += (ADAPTIVE ? time_step : KINEMATICS_RES)) {
    apply_flight(s_takeoff, t, sc);
    if (!is_valid_state(T, sc, GBP_FLIGHT, acc)) return false;
    if (ADAPTIVE) time_step += KINEMATICS_RES;
  }
  f = (f & ~GBP_F_STAGE_MASK) | stage_bits(GBP_STAGE_FWD_LAND);
  apply_flight(s_takeoff, t_f, sc);
  if (!is_valid_state(T, sc, GBP_STANCE, acc)) return false;
  GBP_UNROLL
  for (int k = 0; k < 8; k++) s_new[k] = sc[k];
  t_new = t_s + t_f;
  f |= GBP_F_SNEW_SET | GBP_F_TNEW_SET;
  return true;
}

// planning_utils.cpp:837-876 (plain) and :774-836 (adaptive)
template <bool ADAPTIVE, class TV, class ACC>
GBP_HD_LOOP bool pair_reverse(const TV &T, const double *s, const double *a, double *s_new,
                              double &t_new, ACC &acc, uint32_t &f) {
  const double t_s = a[6], t_f = a[7];
  double sc[8];
  double time_step = KINEMATICS_RES, t_pre_success = 0;
  f = (f & ~GBP_F_STAGE_MASK) | stage_bits(GBP_STAGE_REV_FLIGHT);
  for (double t = 0; t < t_f; t += (ADAPTIVE ? time_step : KINEMATICS_RES)) {
    apply_flight(s, -t, sc);
    if (!is_valid_state(T, sc, GBP_FLIGHT, acc)) return false;
    if (ADAPTIVE) time_step += KINEMATICS_RES;
  }
  double s_takeoff[8];
  apply_flight(s, -t_f, s_takeoff);
  time_step = KINEMATICS_RES;
  f = (f & ~GBP_F_STAGE_MASK) | stage_bits(GBP_STAGE_REV_STANCE);
  for (double t = t_s; t >= 0; t -= (ADAPTIVE ? time_step : KINEMATICS_RES)) {
    apply_stance_reverse(s_takeoff, a, t, sc);
    if (!is_valid_state(T, sc, GBP_STANCE, acc)) {
      if (acc.flags & GBP_F_LIMIT) return false;
      if (!ADAPTIVE || (KINEMATICS_RES - 0.01 <= time_step && time_step <= KINEMATICS_RES + 0.01)) {
        apply_stance(s, a, t + BACKUP_RATIO * (t_s - t), s_new);  // forward stance, as written (:857)
        f |= GBP_F_SNEW_SET;
        return false;
      }
      time_step = KINEMATICS_RES;
      t = t_pre_success;
    } else {
      GBP_UNROLL
      for (int k = 0; k < 8; k++) s_new[k] = sc[k];
      t_new = t_s - t;
      f |= GBP_F_SNEW_SET | GBP_F_TNEW_SET;
      if (ADAPTIVE) {
        time_step += KINEMATICS_RES;
        t_pre_success = t;
      }
    }
  }
  f = (f & ~GBP_F_STAGE_MASK) | stage_bits(GBP_STAGE_REV_START);
  apply_stance_reverse(s_takeoff, a, 0, sc);
  if (!is_valid_state(T, sc, GBP_STANCE, acc)) return false;
  GBP_UNROLL
  for (int k = 0; k < 8; k++) s_new[k] = sc[k];
  t_new = t_s;
  f |= GBP_F_SNEW_SET | GBP_F_TNEW_SET;
  return true;
}

// ---- distances: planning_utils.cpp:106-127 -------------------------------------
GBP_HD double state_distance(const double *q1, const double *q2) {
  double sum = 0;
  GBP_UNROLL
  for (int i = 0; i < 8; i++) sum = sum + 1.0 * (q2[i] - q1[i]) * (q2[i] - q1[i]);
  return sqrt(sum);
}

GBP_HD double pose_distance(const double *q1, const double *q2) {
  double sum = 0;  // planning_utils.cpp:106-115
  GBP_UNROLL
  for (int i = 0; i < 3; i++) sum = sum + (q2[i] - q1[i]) * (q2[i] - q1[i]);
  return sqrt(sum);
}

// stateYawDistance (planning_utils.h:133-145) on the two states' yaws, which
// the caller forms with glibc's atan2(q[4], q[3]) as the reference does (no
// device atan2 reproduces glibc's bits); std::min / std::max as selects
GBP_HD double yaw_distance(double yaw1, double yaw2) {
  const double yaw_min = (yaw2 < yaw1) ? yaw2 : yaw1;
  const double yaw_max = (yaw1 < yaw2) ? yaw2 : yaw1;
  const double a = yaw_max - yaw_min, b = yaw_min + 2 * MY_PI - yaw_max;
  return (b < a) ? b : a;
}

// the reference's path cost (rrt_connect.cpp:193-215, :304-313): the length,
// or with cost_add_yaw the weighted sum of length and yaw
GBP_HD double weighted_cost(bool add_yaw, double lw, double yw, double length, double yaw) {
  return add_yaw ? length * lw + yaw * yw : length;
}

}  // namespace gbp
