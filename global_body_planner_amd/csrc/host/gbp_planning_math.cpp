// gbp_planning_math.cpp — the engine-free arithmetic of planning_utils:
// distances, the propagation closed forms, isValidAction, as State / Action
// wrappers over gbp_closed_forms.h.  No call into include/gbp.h, so the path
// join (gbp_tree_path.cpp) and its stand-alone test program link it without
// the engine.  Compiled without FMA contraction (-ffp-contract=off): the
// expressions are the reference's.
#include "gbp_planner.h"

#include <cmath>

#include "../gbp_closed_forms.h"

namespace gbp_amd {
namespace planning_utils {

// gbp_planner.h is installed and cannot include csrc/: its constants are its
// own, and each one is the shared header's
#define GBP_SAME_CONSTANT(name) static_assert(name == gbp::name, #name " differs from gbp_closed_forms.h")
GBP_SAME_CONSTANT(H_MAX);
GBP_SAME_CONSTANT(H_MIN);
GBP_SAME_CONSTANT(V_MAX);
GBP_SAME_CONSTANT(V_NOM);
GBP_SAME_CONSTANT(P_MAX);
GBP_SAME_CONSTANT(ANG_ACC_MAX);
GBP_SAME_CONSTANT(ROBOT_L);
GBP_SAME_CONSTANT(ROBOT_W);
GBP_SAME_CONSTANT(ROBOT_H);
GBP_SAME_CONSTANT(M_CONST);
GBP_SAME_CONSTANT(G_CONST);
GBP_SAME_CONSTANT(F_MAX);
GBP_SAME_CONSTANT(MU);
GBP_SAME_CONSTANT(T_F_MAX);
GBP_SAME_CONSTANT(T_F_MIN);
GBP_SAME_CONSTANT(KINEMATICS_RES);
GBP_SAME_CONSTANT(BACKUP_RATIO);
GBP_SAME_CONSTANT(GOAL_BOUNDS);
GBP_SAME_CONSTANT(MY_PI);
#undef GBP_SAME_CONSTANT
static_assert(FLIGHT == GBP_FLIGHT && STANCE == GBP_STANCE && FORWARD == GBP_FORWARD &&
                  REVERSE == GBP_REVERSE && STATEDIM == 8 && ACTIONDIM == 10 && POSEDIM == 3,
              "the shared forms' phases, directions and dimensions");

State interp(State q1, State q2, double x) {  // planning_utils.cpp:97-103
  State q;
  for (int d = 0; d < 8; d++) q[d] = (q2[d] - q1[d]) * x + q1[d];
  return q;
}

double poseDistance(const State &q1, const State &q2) {  // :106-115
  return gbp::pose_distance(q1.data(), q2.data());
}

double stateDistance(const State &q1, const State &q2) {  // :116-127
  return gbp::state_distance(q1.data(), q2.data());
}

double stateYawDistance(const State &q1, const State &q2) {  // planning_utils.h:133-145
  const double yaw1 = std::atan2(q1[4], q1[3]);
  const double yaw2 = std::atan2(q2[4], q2[3]);
  return gbp::yaw_distance(yaw1, yaw2);
}

double stateDistance(const State &q1, const State &q2, bool f, double lw, double yw) {
  if (f) return poseDistance(q1, q2) * lw + stateYawDistance(q1, q2) * yw;
  return stateDistance(q1, q2);
}

bool isWithinBounds(State s1, State s2) { return stateDistance(s1, s2) <= GOAL_BOUNDS; }

State applyStance(State s, Action a, double t) {  // :237-274
  State o;
  gbp::apply_stance(s.data(), a.data(), t, o.data());
  return o;
}

State applyStance(State s, Action a) { return applyStance(s, a, a[6]); }

State applyFlight(State s, double t_f) {  // :282-306
  State o;
  gbp::apply_flight(s.data(), t_f, o.data());
  return o;
}

State applyAction(State s, Action a) { return applyFlight(applyStance(s, a), a[7]); }

State applyStanceReverse(State s, Action a, double t) {  // :324-367
  State o;
  gbp::apply_stance_reverse(s.data(), a.data(), t, o.data());
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

bool isValidAction(Action a) { return gbp::is_valid_action(a.data()); }  // :519-556

}  // namespace planning_utils
}  // namespace gbp_amd
