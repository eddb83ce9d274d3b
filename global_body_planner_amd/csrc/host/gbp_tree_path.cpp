// gbp_tree_path.cpp — see gbp_tree_path.h.  Built with the host planner's flags
// (-ffp-contract=off): the sums are the reference's, term by term.
#include "gbp_tree_path.h"

#include <algorithm>
#include <cstring>

namespace gbp_amd {

using planning_utils::stateYawDistance;

std::vector<int> pathFromRoot(const int *parent, int idx) {
  std::vector<int> path{idx};
  while (idx != 0) {
    idx = parent[idx];
    path.push_back(idx);
  }
  std::reverse(path.begin(), path.end());
  return path;
}

std::vector<int> startTreePath(const std::vector<int32_t> &parent, int32_t meet_a) {
  const int64_t n = (int64_t)parent.size();
  std::vector<int> path;
  if (meet_a < 0 || meet_a >= n) return path;
  int32_t idx = meet_a;
  for (int64_t steps = 0; steps < n; steps++) {
    path.push_back(idx);
    if (idx == 0) {
      std::reverse(path.begin(), path.end());
      return path;
    }
    idx = parent[idx];
    if (idx < 0 || idx >= n) break;
  }
  return {};
}

int findStateAmong(const std::vector<State> &v, const std::vector<int> &vertices, const State &s) {
  for (int i : vertices)
    if (i >= 0 && (size_t)i < v.size() && std::memcmp(v[i].data(), s.data(), sizeof(State)) == 0)
      return i;
  return -1;
}

double pathDuration(const std::vector<Action> &actions) {
  double duration = 0;
  for (const Action &a : actions) duration += a[6] + a[7];
  return duration;
}

// y of the path's last vertex: updateGYValue's sums along the parent chain
// (rrt.cpp:91-92, graph_class.cpp:131-138)
static double chainYaw(const TreeView &T, const std::vector<int> &path) {
  double y = 0;
  for (size_t i = 1; i < path.size(); i++) y = y + stateYawDistance(T.v[path[i - 1]], T.v[path[i]]);
  return y;
}

JoinedPath joinTreePaths(const TreeView &Ta, int ia, const TreeView &Tb, int ib) {
  const std::vector<int> path_a = pathFromRoot(Ta.parent, ia);
  const std::vector<int> path_b = pathFromRoot(Tb.parent, ib);
  JoinedPath p;
  for (int i : path_a) p.states.push_back(Ta.v[i]);
  for (size_t i = 1; i < path_a.size(); i++) p.actions.push_back(Ta.a[path_a[i]]);
  // Tb from ib back to its root: ib's state is dropped (the connect put it at
  // ia's), its action leads on to its parent
  for (size_t i = path_b.size(); i-- > 1;) {
    p.actions.push_back(Tb.a[path_b[i]]);
    p.states.push_back(Tb.v[path_b[i - 1]]);
  }
  p.length = Ta.g[ia] + Tb.g[ib];
  p.yaw = chainYaw(Ta, path_a) + chainYaw(Tb, path_b);
  p.duration = pathDuration(p.actions);
  return p;
}

JoinedPath pathFromRows(std::vector<State> states, std::vector<Action> actions, int n_from_a,
                        const State &s_ib, double length) {
  JoinedPath p;
  const int n = (int)states.size();
  if (n < 1 || n_from_a < 1 || n_from_a > n || (int)actions.size() != n - 1) return p;
  // the two chains' sums, each from its own root down, as chainYaw forms them:
  // Ta's chain is states[0, n_from_a); Tb's runs from the path's last state
  // back to states[n_from_a] and ends at ib's own state
  double ya = 0, yb = 0;
  for (int i = 1; i < n_from_a; i++) ya = ya + stateYawDistance(states[i - 1], states[i]);
  for (int i = n - 1; i > n_from_a; i--) yb = yb + stateYawDistance(states[i], states[i - 1]);
  if (n > n_from_a) yb = yb + stateYawDistance(states[n_from_a], s_ib);
  p.yaw = ya + yb;
  p.length = length;
  p.duration = pathDuration(actions);
  p.states = std::move(states);
  p.actions = std::move(actions);
  return p;
}

}  // namespace gbp_amd
