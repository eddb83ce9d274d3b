// gbp_shortcut_walk.h — RRTConnectClass::postProcessPath's walk
// (rrt_connect.cpp:139-227) over a table of connect decisions (internal to
// libgbp; plain C++, no HIP or engine types).
//
// attemptConnect(s, s_next, FORWARD) == REACHED depends on the two states and
// the terrain alone, so every decision a path's walk can ask for is known
// before the walk starts: reached[] holds them for all pairs (i, j), i < j, of
// the path's n states, packed row-major over the upper triangle,
//   pair_index(n, i, j) = i (2n - i - 1) / 2 + (j - i - 1).
// The walk itself is the reference's loop, state values and all; it follows a
// state's position in the path only to address the table.
#pragma once

#include <cstdint>

namespace gbp_shortcut {

inline int64_t pair_count(int64_t n) { return n * (n - 1) / 2; }
inline int64_t pair_index(int64_t n, int64_t i, int64_t j) {
  return i * (2 * n - i - 1) / 2 + (j - i - 1);
}

// the reference's path cost (rrt_connect.cpp:193-215): the length, or with
// cost_add_yaw the weighted sum of length and yaw
struct CostWeights {
  int add_yaw = 0;
  double length_weight = 1, yaw_weight = 1;
};

// states[n][8], actions[n - 1][10] (n >= 2), reached[pair_count(n)] nonzero
// where the pair's connect is REACHED.  Writes the kept states and actions
// (at most n and n - 1 of them: the walk never lengthens a path) and
// path_length_ / path_yaw_ / path_cost_ as postProcessPath leaves them;
// returns the number of kept states.
int64_t walk(int64_t n, const double *states, const double *actions, const uint8_t *reached,
             const CostWeights &cw, double *out_states, double *out_actions, double *path_length,
             double *path_yaw, double *path_cost);

}  // namespace gbp_shortcut
