// The node's loop against a search that stays on the device (ReplanSession,
// INTEGRATION.md "Replanning"), without ROS and through the reference's global
// names: the slope CSV loaded as in node_config1.cpp, one plan, then a
// terrainMapCallback that changes a rectangle of the map (updateDataFlat on the
// same FastTerrainMap), mapChanged, bestPath (the search resumed only when no
// kept connection survives) and getInterpPath.
//
//   node_replan <csv dir> <engine batch> <seed>
// prints one JSON line; exit 0 when both plans run start -> goal.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gbp_planner_compat.h"

static bool whole(const std::vector<State> &s, const std::vector<Action> &a, const State &start,
                  const State &goal) {
  return s.size() >= 2 && s.front() == start && s.back() == goal && a.size() + 1 == s.size();
}

int main(int argc, char **argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s <csv dir> <engine batch> <seed>\n", argv[0]);
    return 2;
  }
  try {
    FastTerrainMap terrain_;
    terrain_.loadMapFromCSV(argv[1]);
    State robot_start_ = {1.0, 0.0, 0.375, 1, 0, 0, 0, 0};
    State robot_goal_ = {8.0, 0.0, 0.375, 1, 0, 0, 0, 0};
    robot_start_[2] += terrain_.getGroundHeight(robot_start_[0], robot_start_[1]);
    robot_goal_[2] += terrain_.getGroundHeight(robot_goal_[0], robot_goal_[1]);
    ReplanSession session_;
    session_.set_state_action_pair_check_adaptive_step_size_flag_(false);
    session_.begin(terrain_, robot_start_, robot_goal_, std::atoi(argv[2]), 3.0,
                   std::strtoull(argv[3], nullptr, 10));
    // callPlanner, first tick: search until a connection is held (at most 20 s)
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [&]() {
      return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    };
    while (!session_.search(0.25) && since() < 20.0) {
    }
    std::vector<State> state_sequence_;
    std::vector<Action> action_sequence_;
    const bool first = session_.bestPath(state_sequence_, action_sequence_) &&
                       whole(state_sequence_, action_sequence_, robot_start_, robot_goal_);
    const double t_first = since(), cost_first = session_.pathCost();
    const size_t n_first = state_sequence_.size();
    // terrainMapCallback: a 0.5 m square beside the straight line raised by 5 cm
    // (values an fp32-storage handle holds too)
    const std::vector<double> &xs = terrain_.getXData(), &ys = terrain_.getYData();
    int ix0 = -1, ix1 = -1, iy0 = -1, iy1 = -1;
    for (int i = 0; i < (int)xs.size(); i++)
      if (xs[i] >= 4.0 && xs[i] <= 4.5) {
        if (ix0 < 0) ix0 = i;
        ix1 = i + 1;
      }
    for (int j = 0; j < (int)ys.size(); j++)
      if (ys[j] >= 0.5 && ys[j] <= 1.0) {
        if (iy0 < 0) iy0 = j;
        iy1 = j + 1;
      }
    if (ix0 < 0 || iy0 < 0) {
      std::fprintf(stderr, "the map does not cover the rectangle\n");
      return 3;
    }
    const int pnx = ix1 - ix0, pny = iy1 - iy0;
    std::vector<double> patch((size_t)pnx * pny);
    for (int i = 0; i < pnx; i++)
      for (int j = 0; j < pny; j++)
        patch[(size_t)i * pny + j] = (double)(float)(terrain_.getGroundHeight(xs[ix0 + i], ys[iy0 + j]) + 0.05);
    terrain_.updateDataFlat(ix0, iy0, pnx, pny, patch.data(), nullptr, nullptr, nullptr);
    const double t1 = since();
    PruneStats pruned[2];
    SharedStats shared;
    session_.mapChanged(terrain_, pruned, &shared);
    bool second = session_.bestPath(state_sequence_, action_sequence_);
    const double t_replan = since() - t1;
    const bool survived = second;
    while (!second && since() < 40.0)  // nothing survived: the search goes on from the pruned trees
      second = session_.search(0.25) && session_.bestPath(state_sequence_, action_sequence_);
    second = second && whole(state_sequence_, action_sequence_, robot_start_, robot_goal_);
    std::vector<State> body_plan_;
    std::vector<double> t_plan_;
    std::vector<int> interp_phase;
    if (second)
      getInterpPath(state_sequence_, action_sequence_, 0.05, body_plan_, t_plan_, interp_phase);
    std::printf("{\"first_ok\": %d, \"first_s\": %.6f, \"first_states\": %zu, \"first_cost\": %.6f, "
                "\"kept_a\": %lld, \"of_a\": %lld, \"kept_b\": %lld, \"of_b\": %lld, "
                "\"connections\": %lld, \"connections_kept\": %lld, \"survived\": %d, "
                "\"replan_s\": %.6f, \"second_ok\": %d, \"second_states\": %zu, \"second_cost\": %.6f, "
                "\"interp\": %zu}\n",
                first ? 1 : 0, t_first, n_first, cost_first, (long long)pruned[0].n_kept,
                (long long)pruned[0].n_before, (long long)pruned[1].n_kept,
                (long long)pruned[1].n_before, (long long)shared.n_before, (long long)shared.n_kept,
                survived ? 1 : 0, t_replan, second ? 1 : 0, state_sequence_.size(), session_.pathCost(),
                body_plan_.size());
    return first && second && !body_plan_.empty() ? 0 : 1;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "node_replan: %s\n", e.what());
    return 1;
  }
}
