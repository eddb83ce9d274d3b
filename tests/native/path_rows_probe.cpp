// path_rows_probe.cpp — gbp_amd::pathFromRows against gbp_amd::joinTreePaths
// (csrc/host/gbp_tree_path.cpp) on one pair of trees read from a text file in
// tree_path_probe.cpp's format: the joined rows of joinTreePaths, handed to
// pathFromRows with the count of Ta's vertices and ib's own state, must give
// the same states, actions, length, yaw and duration bit for bit.  Also the
// sizes pathFromRows refuses.  tests/test_shared_ref.py builds this with
// -fsanitize=address,undefined (heap arrays of exactly the trees' sizes).
//
// output: "ok <states> <n_from_a>" or a line naming what differs (exit 1)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "gbp_tree_path.h"

using gbp_amd::Action;
using gbp_amd::State;

static bool read_double(FILE *f, double *v) {
  char tok[64];
  if (std::fscanf(f, "%63s", tok) != 1) return false;
  char *end = nullptr;
  *v = std::strtod(tok, &end);
  return end && *end == 0;
}

struct Tree {
  std::unique_ptr<State[]> v;
  std::unique_ptr<Action[]> a;
  std::unique_ptr<int[]> parent;
  std::unique_ptr<double[]> g;
  bool read(FILE *f, long long n) {
    v.reset(new State[n]);
    a.reset(new Action[n]);
    parent.reset(new int[n]);
    g.reset(new double[n]);
    for (long long i = 0; i < n; i++)
      for (double &x : v[i])
        if (!read_double(f, &x)) return false;
    for (long long i = 0; i < n; i++)
      for (double &x : a[i])
        if (!read_double(f, &x)) return false;
    for (long long i = 0; i < n; i++)
      if (std::fscanf(f, "%d", &parent[i]) != 1) return false;
    for (long long i = 0; i < n; i++)
      if (!read_double(f, &g[i])) return false;
    return true;
  }
  gbp_amd::TreeView view() const { return {v.get(), a.get(), parent.get(), g.get()}; }
};

static bool same(double x, double y) { return std::memcmp(&x, &y, sizeof x) == 0; }

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  long long na = 0, nb = 0;
  int ia = 0, ib = 0;
  if (std::fscanf(f, "%lld %lld %d %d", &na, &nb, &ia, &ib) != 4) return 3;
  if (na < 1 || nb < 1 || ia < 0 || ia >= na || ib < 0 || ib >= nb) return 3;
  Tree A, B;
  if (!A.read(f, na) || !B.read(f, nb)) return 3;
  std::fclose(f);
  const gbp_amd::JoinedPath p = gbp_amd::joinTreePaths(A.view(), ia, B.view(), ib);
  const int n_from_a = (int)gbp_amd::pathFromRoot(A.parent.get(), ia).size();
  const gbp_amd::JoinedPath q = gbp_amd::pathFromRows(p.states, p.actions, n_from_a, B.v[ib], p.length);
  if (q.states != p.states || q.actions != p.actions) return std::puts("rows differ"), 1;
  if (!same(q.length, p.length)) return std::puts("length differs"), 1;
  if (!same(q.yaw, p.yaw)) return std::printf("yaw differs: %a %a\n", q.yaw, p.yaw), 1;
  if (!same(q.duration, p.duration)) return std::puts("duration differs"), 1;
  // sizes that do not fit give an empty path
  auto short_actions = p.actions;
  if (!short_actions.empty()) short_actions.pop_back();
  if (!p.actions.empty() &&
      !gbp_amd::pathFromRows(p.states, short_actions, n_from_a, B.v[ib], p.length).states.empty())
    return std::puts("an action short was accepted"), 1;
  if (!gbp_amd::pathFromRows(p.states, p.actions, 0, B.v[ib], p.length).states.empty() ||
      !gbp_amd::pathFromRows(p.states, p.actions, (int)p.states.size() + 1, B.v[ib], p.length)
           .states.empty())
    return std::puts("a bad count of Ta's vertices was accepted"), 1;
  std::printf("ok %zu %d\n", p.states.size(), n_from_a);
  return 0;
}
