// gbp_planning_math.cpp — the engine-free arithmetic of planning_utils:
// distances, the propagation closed forms, isValidAction.  No call into
// include/gbp.h, so the path join (gbp_tree_path.cpp) and its stand-alone test
// program link it without the engine.  Compiled without FMA contraction
// (-ffp-contract=off): the expressions are the reference's.
#include "gbp_planner.h"

#include <cmath>

namespace gbp_amd {
namespace planning_utils {

static inline double std_min(double a, double b) { return (b < a) ? b : a; }
static inline double std_max(double a, double b) { return (a < b) ? b : a; }

State interp(State q1, State q2, double x) {  // planning_utils.cpp:97-103
  State q;
  for (int d = 0; d < 8; d++) q[d] = (q2[d] - q1[d]) * x + q1[d];
  return q;
}

double poseDistance(const State &q1, const State &q2) {  // :106-115
  double sum = 0;
  for (int i = 0; i < POSEDIM; i++) sum = sum + (q2[i] - q1[i]) * (q2[i] - q1[i]);
  return std::sqrt(sum);
}

double stateDistance(const State &q1, const State &q2) {  // :116-127
  double sum = 0;
  for (int i = 0; i < 8; i++) sum = sum + 1.0 * (q2[i] - q1[i]) * (q2[i] - q1[i]);
  return std::sqrt(sum);
}

double stateYawDistance(const State &q1, const State &q2) {  // planning_utils.h:133-145
  const double yaw1 = std::atan2(q1[4], q1[3]);
  const double yaw2 = std::atan2(q2[4], q2[3]);
  const double yaw_min = std_min(yaw1, yaw2), yaw_max = std_max(yaw1, yaw2);
  return std_min(yaw_max - yaw_min, yaw_min + 2 * MY_PI - yaw_max);
}

double stateDistance(const State &q1, const State &q2, bool f, double lw, double yw) {
  if (f) return poseDistance(q1, q2) * lw + stateYawDistance(q1, q2) * yw;
  return stateDistance(q1, q2);
}

bool isWithinBounds(State s1, State s2) { return stateDistance(s1, s2) <= GOAL_BOUNDS; }

State applyStance(State s, Action a, double t) {  // :237-274
  const double a_x_td = a[0], a_y_td = a[1], a_z_td = a[2];
  const double a_x_to = a[3], a_y_to = a[4], a_z_to = a[5];
  const double t_s = a[6], a_p_td = a[8], a_p_to = a[9];
  State o;
  o[0] = s[0] + s[3] * t + 0.5 * a_x_td * t * t + (a_x_to - a_x_td) * (t * t * t) / (6.0 * t_s);
  o[1] = s[1] + s[4] * t + 0.5 * a_y_td * t * t + (a_y_to - a_y_td) * (t * t * t) / (6.0 * t_s);
  o[2] = s[2] + s[5] * t + 0.5 * a_z_td * t * t + (a_z_to - a_z_td) * (t * t * t) / (6.0 * t_s);
  o[3] = s[3] + a_x_td * t + (a_x_to - a_x_td) * t * t / (2.0 * t_s);
  o[4] = s[4] + a_y_td * t + (a_y_to - a_y_td) * t * t / (2.0 * t_s);
  o[5] = s[5] + a_z_td * t + (a_z_to - a_z_td) * t * t / (2.0 * t_s);
  o[6] = s[6] + s[7] * t + 0.5 * a_p_td * t * t + (a_p_to - a_p_td) * (t * t * t) / (6.0 * t_s);
  o[7] = s[7] + a_p_td * t + (a_p_to - a_p_td) * t * t / (2.0 * t_s);
  return o;
}

State applyStance(State s, Action a) { return applyStance(s, a, a[6]); }

State applyFlight(State s, double t_f) {  // :282-306
  const double g = 9.81;
  State o;
  o[0] = s[0] + s[3] * t_f;
  o[1] = s[1] + s[4] * t_f;
  o[2] = s[2] + s[5] * t_f - 0.5 * g * t_f * t_f;
  o[3] = s[3];
  o[4] = s[4];
  o[5] = s[5] - g * t_f;
  o[6] = s[6] + s[7] * t_f;
  o[7] = s[7];
  return o;
}

State applyAction(State s, Action a) { return applyFlight(applyStance(s, a), a[7]); }

State applyStanceReverse(State s, Action a, double t) {  // :324-367
  const double a_x_td = a[0], a_y_td = a[1], a_z_td = a[2];
  const double a_x_to = a[3], a_y_to = a[4], a_z_to = a[5];
  const double t_s = a[6], a_p_td = a[8], a_p_to = a[9];
  const double cx = s[3] - a_x_td * t_s - 0.5 * (a_x_to - a_x_td) * t_s;
  const double cy = s[4] - a_y_td * t_s - 0.5 * (a_y_to - a_y_td) * t_s;
  const double cz = s[5] - a_z_td * t_s - 0.5 * (a_z_to - a_z_td) * t_s;
  const double cp = s[7] - a_p_td * t_s - 0.5 * (a_p_to - a_p_td) * t_s;
  State o;
  o[0] = s[0] - cx * (t_s - t) - 0.5 * a_x_td * (t_s * t_s - t * t) -
         (a_x_to - a_x_td) * (t_s * t_s * t_s - t * t * t) / (6.0 * t_s);
  o[1] = s[1] - cy * (t_s - t) - 0.5 * a_y_td * (t_s * t_s - t * t) -
         (a_y_to - a_y_td) * (t_s * t_s * t_s - t * t * t) / (6.0 * t_s);
  o[2] = s[2] - cz * (t_s - t) - 0.5 * a_z_td * (t_s * t_s - t * t) -
         (a_z_to - a_z_td) * (t_s * t_s * t_s - t * t * t) / (6.0 * t_s);
  o[3] = s[3] - a_x_td * (t_s - t) - (a_x_to - a_x_td) * (t_s * t_s - t * t) / (2.0 * t_s);
  o[4] = s[4] - a_y_td * (t_s - t) - (a_y_to - a_y_td) * (t_s * t_s - t * t) / (2.0 * t_s);
  o[5] = s[5] - a_z_td * (t_s - t) - (a_z_to - a_z_td) * (t_s * t_s - t * t) / (2.0 * t_s);
  o[7] = s[7] - a_p_td * (t_s - t) - (a_p_to - a_p_td) * (t_s * t_s - t * t) / (2.0 * t_s);
  o[6] = s[6] - cp * (t_s - t) - 0.5 * a_p_td * (t_s * t_s - t * t) -
         (a_p_to - a_p_td) * (t_s * t_s * t_s - t * t * t) / (6.0 * t_s);
  return o;
}

State applyStanceReverse(State s, Action a) { return applyStanceReverse(s, a, 0); }

std::array<double, 3> rotate_grf(std::array<double, 3> n, std::array<double, 3> f) {  // :198-231
  const double v0 = n[1] * 1.0 - n[2] * 0.0, v1 = n[2] * 0.0 - n[0] * 1.0,
               v2 = n[0] * 0.0 - n[1] * 0.0;
  const double s = std::sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  const double c = n[0] * 0.0 + n[1] * 0.0 + n[2] * 1.0;
  if (s < 0.000001) return f;
  const double K[3][3] = {{0, -v2, v1}, {v2, 0, -v0}, {-v1, v0, 0}};
  std::array<double, 3> out;
  for (int i = 0; i < 3; i++) {
    double acc = 0;
    for (int j = 0; j < 3; j++) {
      const double kk = K[i][0] * K[0][j] + K[i][1] * K[1][j] + K[i][2] * K[2][j];
      const double r = (i == j ? 1.0 : 0.0) + K[i][j] + kk * (1 - c) / (s * s);
      acc = j == 0 ? r * f[0] : acc + r * f[j];
    }
    out[i] = acc;
  }
  return out;
}

bool isValidAction(Action a) {  // :519-556
  if ((a[6] <= 0) || (a[7] < 0)) return false;
  const double m = M_CONST, g = G_CONST, mu = MU;
  const double f_x_td = m * a[0], f_y_td = m * a[1], f_z_td = m * (a[2] + g);
  const double f_x_to = m * a[3], f_y_to = m * a[4], f_z_to = m * (a[5] + g);
  if ((std::sqrt(f_x_td * f_x_td + f_y_td * f_y_td + f_z_td * f_z_td) >= F_MAX) ||
      (std::sqrt(f_x_to * f_x_to + f_y_to * f_y_to + f_z_to * f_z_to) >= F_MAX) || (f_z_td < 0) ||
      (f_z_to < 0) || (a[8] >= F_MAX) || (a[9] >= F_MAX))
    return false;
  if ((std::sqrt(f_x_td * f_x_td + f_y_td * f_y_td) >= mu * f_z_td) ||
      (std::sqrt(f_x_to * f_x_to + f_y_to * f_y_to) >= mu * f_z_to))
    return false;
  return true;
}

}  // namespace planning_utils
}  // namespace gbp_amd
