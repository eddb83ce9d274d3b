// gbp_tree_path.h — the path through two half trees joined at a connection
// (rrt_connect.cpp:386-401, rrt_star_connect.cpp:70-89).  Pure host code with
// no engine call: every search form (PlannerClass trees on the host, trees
// read back from the device) builds its path here.
#pragma once

#include <vector>

#include "gbp_planner.h"

namespace gbp_amd {

// A read-only view of one tree, root at index 0: vertex states, the action
// reaching each vertex, parents (root -1) and g (path length from the root).
struct TreeView {
  const State *v;
  const Action *a;
  const int *parent;
  const double *g;
};

struct JoinedPath {
  std::vector<State> states;
  std::vector<Action> actions;
  double length = 0;    // g_a[ia] + g_b[ib]
  double yaw = 0;       // the two chains' yaw sums (what updateGYValue keeps in y)
  double duration = 0;  // pathDuration(actions)
};

// rrt.cpp:107-118: the vertices root -> idx
std::vector<int> pathFromRoot(const int *parent, int idx);

// The robot has moved along a found path: the start tree's vertices the path
// runs over, root -> meet_a (BatchStats::meet_a), from a dumped tree's
// parents; empty when meet_a is no vertex of the tree or the chain does not
// end at the root within the tree's size.
std::vector<int> startTreePath(const std::vector<int32_t> &parent, int32_t meet_a);

// Which of `vertices` (indices into v) holds exactly state s, all eight
// values bit for bit: a post-processed path keeps tree states but not tree
// indices.  The first match, or -1.
int findStateAmong(const std::vector<State> &v, const std::vector<int> &vertices, const State &s);

// sum of stance + flight time over the actions
double pathDuration(const std::vector<Action> &actions);

// Ta's root -> ia, then Tb's ib -> root without ib itself; Tb's edges are
// walked against their direction, so edge (parent <- child) carries the
// child's action (getActionSequenceReverse).
JoinedPath joinTreePaths(const TreeView &Ta, int ia, const TreeView &Tb, int ib);

// The same JoinedPath from the joined rows themselves (gbp_tree_path_host
// gathers them on the device): the first n_from_a states are Ta's chain, the
// rest Tb's chain below ib walked up to its root; s_ib is ib's own state,
// which the path drops but the yaw sum of Tb's chain ends at; length = g_a[ia]
// + g_b[ib] as the device returned it.  Yaw and duration are summed here in
// joinTreePaths' order.  An empty path when the sizes do not fit.
JoinedPath pathFromRows(std::vector<State> states, std::vector<Action> actions, int n_from_a,
                        const State &s_ib, double length);

}  // namespace gbp_amd
