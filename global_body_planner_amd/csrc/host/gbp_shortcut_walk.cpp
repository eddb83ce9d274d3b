// gbp_shortcut_walk.cpp — postProcessPath's walk over a connect table
// (gbp_shortcut_walk.h).  Built like gbp_host_check.cpp: g++ without FMA
// contraction, glibc's atan2 — the reference's arithmetic for the kept
// connect actions and the path's length, yaw and cost.
#include "gbp_shortcut_walk.h"

#include <algorithm>
#include <array>
#include <cmath>

#include "../gbp_closed_forms.h"
#include "gbp_host_check.h"

namespace gbp_shortcut {
namespace {

using State = std::array<double, 8>;
using Action = std::array<double, 10>;

using gbp::V_NOM;

double state_yaw_distance(const State &q1, const State &q2) {  // planning_utils.h:133-145
  const double yaw1 = std::atan2(q1[4], q1[3]);
  const double yaw2 = std::atan2(q2[4], q2[3]);
  return gbp::yaw_distance(yaw1, yaw2);
}

}  // namespace

int64_t walk(int64_t n, const double *states, const double *actions, const uint8_t *reached,
             const CostWeights &cw, double *out_states, double *out_actions, double *path_length,
             double *path_yaw, double *path_cost) {  // rrt_connect.cpp:139-227
  auto state_at = [&](int64_t k) {
    State q;
    std::copy(states + 8 * k, states + 8 * k + 8, q.begin());
    return q;
  };
  auto action_at = [&](int64_t k) {
    Action a;
    std::copy(actions + 10 * k, actions + 10 * k + 10, a.begin());
    return a;
  };
  int64_t m = 0;  // states kept so far; action m - 1 leads into state m
  auto keep = [&](const State &q, const Action *a) {
    std::copy(q.begin(), q.end(), out_states + 8 * m);
    if (a) std::copy(a->begin(), a->end(), out_actions + 10 * (m - 1));
    m++;
  };
  State s = state_at(0);
  const State s_goal = state_at(n - 1);
  Action a_new{};
  int64_t at = 0;  // s's place in the path: the table's row, nothing else
  keep(s, nullptr);
  double len = 0, yaw = 0, cost = 0;
  auto weighted_cost = [&](double dl, double dy) {
    return gbp::weighted_cost(cw.add_yaw != 0, cw.length_weight, cw.yaw_weight, dl, dy);
  };
  while (s != s_goal) {
    // the reference copies both sequences and pops their backs; `back` is the
    // place of the state copy's back(), whose action is the action copy's
    int64_t back = n - 1;
    State s_next = state_at(back);
    Action a_next = action_at(back - 1);
    State old_state{};
    Action old_action{};
    int64_t old_at = at;
    // attemptConnect(s, s_next, dummy, a_new, terrain, FORWARD) == REACHED: the
    // decision from the table, the action as attemptConnect forms it (:53-63, :89)
    auto reaches = [&]() {
      if (back <= at || !reached[pair_index(n, at, back)]) return false;
      const double t_s = gbp_host::pose_distance(s_next.data(), s.data()) / V_NOM;
      gbp_host::connect_action(s.data(), s_next.data(), t_s, a_new.data());
      return true;
    };
    while (!reaches() && (s != s_next)) {
      if (back == 0) return -1;  // a NaN state equals nothing: the reference pops an empty vector
      old_state = s_next;
      old_action = a_next;
      old_at = back;
      back--;
      s_next = state_at(back);
      // the reference reads back() of the now-empty action copy when it pops
      // down to the first state (never used afterwards): keep the last value
      if (back > 0) a_next = action_at(back - 1);
    }
    if (s != s_next) {
      keep(s_next, &a_new);
      const double dl = gbp_host::pose_distance(s.data(), s_next.data());
      const double dy = state_yaw_distance(s, s_next);
      len += dl;
      yaw += dy;
      cost += weighted_cost(dl, dy);
      s = s_next;
      at = back;
    } else {
      // the reference adds to path_cost_ but not path_length_ here (:210-215)
      keep(old_state, &old_action);
      const double dl = gbp_host::pose_distance(s.data(), old_state.data());
      const double dy = state_yaw_distance(s, old_state);
      cost += weighted_cost(dl, dy);
      s = old_state;
      at = old_at;
    }
  }
  *path_length = len;
  *path_yaw = yaw;
  *path_cost = cost;
  return m;
}

}  // namespace gbp_shortcut
