/*
 * ref_driver.cpp — extern "C" surface over the compiled reference planner.
 *
 * TEST INFRASTRUCTURE ONLY.  Linked with the reference's own seven sources
 * (read in place, never copied) into oracle/_ref/libgbp_ref.so, which
 * tools/make_ref_golden.py and tests/test_reference_parity.py load.  Every
 * entry calls the reference's public functions and classes; none restates a
 * body.  Nothing here reaches rand() or the clock-seeded engines except
 * ref_extend, whose drawn action is recorded as data by the caller.
 */
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "global_body_planner/rrt_star_connect.h"

using namespace planning_utils;

namespace {

State to_state(const double *p) {
  State s;
  std::memcpy(s.data(), p, sizeof(double) * STATEDIM);
  return s;
}
Action to_action(const double *p) {
  Action a;
  std::memcpy(a.data(), p, sizeof(double) * ACTIONDIM);
  return a;
}
void put(double *p, const State &s) { std::memcpy(p, s.data(), sizeof(double) * STATEDIM); }
void put(double *p, const Action &a) { std::memcpy(p, a.data(), sizeof(double) * ACTIONDIM); }

/* the reference keeps its path figures protected; a derived class reads them */
struct Planner : RRTStarConnectClass {
  double length() const { return path_length_; }
  double yaw() const { return path_yaw_; }
  double cost() const { return path_cost_; }
};

/* a tree and the vertex count the caller has put in it */
struct Tree {
  PlannerClass t;
};

void configure(Planner &p, int adaptive) {
  p.set_state_action_pair_check_adaptive_step_size_flag_(adaptive != 0);
  p.set_action_direction_sampling(false, 0.0);
}

}  // namespace

extern "C" {

/* ---- terrain (FastTerrainMap::loadData; x-major arrays as the oracle's) ---- */
void *ref_terrain_new(int nx, int ny, const double *x, const double *y, const double *z,
                      const double *dx, const double *dy, const double *dz) {
  std::vector<double> xs(x, x + nx), ys(y, y + ny);
  std::vector<std::vector<double>> zz(nx), gx(nx), gy(nx), gz(nx);
  for (int i = 0; i < nx; i++) {
    zz[i].assign(z + (size_t)i * ny, z + (size_t)(i + 1) * ny);
    gx[i].assign(dx + (size_t)i * ny, dx + (size_t)(i + 1) * ny);
    gy[i].assign(dy + (size_t)i * ny, dy + (size_t)(i + 1) * ny);
    gz[i].assign(dz + (size_t)i * ny, dz + (size_t)(i + 1) * ny);
  }
  FastTerrainMap *T = new FastTerrainMap();
  T->loadData(nx, ny, xs, ys, zz, gx, gy, gz);
  return T;
}
void ref_terrain_free(void *T) { delete static_cast<FastTerrainMap *>(T); }

void ref_lookups(void *Tp, int64_t n, const double *xy, double *h, uint8_t *is_nan, double *nrm) {
  FastTerrainMap &T = *static_cast<FastTerrainMap *>(Tp);
  for (int64_t i = 0; i < n; i++) {
    h[i] = T.getGroundHeight(xy[2 * i], xy[2 * i + 1]);
    is_nan[i] = T.heightIsNan(xy[2 * i], xy[2 * i + 1]);
    std::array<double, 3> v = T.getSurfaceNormal(xy[2 * i], xy[2 * i + 1]);
    nrm[3 * i] = v[0], nrm[3 * i + 1] = v[1], nrm[3 * i + 2] = v[2];
  }
}

/* ---- closed forms ---- */
/* out[n][6][8]: applyStance(s,a,t), applyStance(s,a), applyFlight(s,t),
 * applyAction(s,a), applyStanceReverse(s,a,t), applyStanceReverse(s,a) */
void ref_apply(int64_t n, const double *s, const double *a, const double *t, double *out) {
  for (int64_t i = 0; i < n; i++) {
    State q = to_state(s + 8 * i);
    Action u = to_action(a + 10 * i);
    double *o = out + 48 * i;
    put(o, applyStance(q, u, t[i]));
    put(o + 8, applyStance(q, u));
    put(o + 16, applyFlight(q, t[i]));
    put(o + 24, applyAction(q, u));
    put(o + 32, applyStanceReverse(q, u, t[i]));
    put(o + 40, applyStanceReverse(q, u));
  }
}

/* out[n][5]: poseDistance, stateDistance, stateYawDistance, the weighted
 * stateDistance with the flag set and with it clear; within[n]: isWithinBounds */
void ref_distances(int64_t n, const double *q1, const double *q2, double lw, double yw, double *out,
                   uint8_t *within) {
  for (int64_t i = 0; i < n; i++) {
    State a = to_state(q1 + 8 * i), b = to_state(q2 + 8 * i);
    out[5 * i] = poseDistance(a, b);
    out[5 * i + 1] = stateDistance(a, b);
    out[5 * i + 2] = stateYawDistance(a, b);
    out[5 * i + 3] = stateDistance(a, b, true, lw, yw);
    out[5 * i + 4] = stateDistance(a, b, false, lw, yw);
    within[i] = isWithinBounds(a, b);
  }
}

void ref_valid_actions(int64_t n, const double *a, uint8_t *out) {
  for (int64_t i = 0; i < n; i++) out[i] = isValidAction(to_action(a + 10 * i));
}

void ref_rotate_grf(int64_t n, const double *nrm, const double *f, double *out) {
  for (int64_t i = 0; i < n; i++) {
    std::array<double, 3> r = rotate_grf({nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]},
                                         {f[3 * i], f[3 * i + 1], f[3 * i + 2]});
    out[3 * i] = r[0], out[3 * i + 1] = r[1], out[3 * i + 2] = r[2];
  }
}

void ref_interp(int64_t n, const double *q1, const double *q2, const double *x, double *out) {
  for (int64_t i = 0; i < n; i++) put(out + 8 * i, interp(to_state(q1 + 8 * i), to_state(q2 + 8 * i), x[i]));
}

/* getInterpPath over ns states / ns-1 actions: returns the number of path
 * points m (t has m entries, phase m-1), or -m if cap is too small */
int ref_interp_path(int ns, const double *states, const double *actions, double dt, int cap,
                    double *path, double *t, int32_t *phase) {
  std::vector<State> ss, ip;
  std::vector<Action> as;
  std::vector<double> it;
  std::vector<int> iph;
  for (int i = 0; i < ns; i++) ss.push_back(to_state(states + 8 * i));
  for (int i = 0; i + 1 < ns; i++) as.push_back(to_action(actions + 10 * i));
  getInterpPath(ss, as, dt, ip, it, iph);
  int m = (int)ip.size();
  if (m > cap) return -m;
  for (int i = 0; i < m; i++) put(path + 8 * i, ip[i]), t[i] = it[i];
  for (size_t i = 0; i < iph.size(); i++) phase[i] = iph[i];
  return m;
}

/* ---- validity ---- */
void ref_valid_states(void *Tp, int64_t n, const double *s, int phase, uint8_t *out) {
  FastTerrainMap &T = *static_cast<FastTerrainMap *>(Tp);
  for (int64_t i = 0; i < n; i++) out[i] = isValidState(to_state(s + 8 * i), T, phase);
}

/* s_new / t_new arrive preset by the caller and are written back as the
 * reference leaves them, so "never assigned" stays observable */
void ref_pairs(void *Tp, int64_t n, const double *s, const double *a, const uint8_t *direction,
               int adaptive, uint8_t *valid, double *s_new, double *t_new) {
  FastTerrainMap &T = *static_cast<FastTerrainMap *>(Tp);
  for (int64_t i = 0; i < n; i++) {
    State sn = to_state(s_new + 8 * i);
    double tn = t_new[i];
    State q = to_state(s + 8 * i);
    Action u = to_action(a + 10 * i);
    valid[i] = direction[i] == FORWARD ? isValidStateActionPair(q, u, T, sn, tn, adaptive != 0)
                                       : isValidStateActionPairReverse(q, u, T, sn, tn, adaptive != 0);
    put(s_new + 8 * i, sn);
    t_new[i] = tn;
  }
}

/* ---- connect: t_s[i] NaN selects the two-state overload ---- */
void ref_connects(void *Tp, int64_t n, const double *s_existing, const double *s, const double *t_s,
                  const uint8_t *direction, int adaptive, int32_t *result, double *s_new,
                  double *a_new) {
  FastTerrainMap &T = *static_cast<FastTerrainMap *>(Tp);
  Planner p;
  configure(p, adaptive);
  for (int64_t i = 0; i < n; i++) {
    State sn = to_state(s_new + 8 * i);
    Action an = to_action(a_new + 10 * i);
    State e = to_state(s_existing + 8 * i), q = to_state(s + 8 * i);
    result[i] = t_s[i] != t_s[i] ? p.attemptConnect(e, q, sn, an, T, direction[i])
                                 : p.attemptConnect(e, q, t_s[i], sn, an, T, direction[i]);
    put(s_new + 8 * i, sn);
    put(a_new + 10 * i, an);
  }
}

/* ---- trees through PlannerClass / GraphClass ---- */
void *ref_tree_new(const double *root, int yaw_flag, double lw, double yw) {
  Tree *t = new Tree();
  t->t.init(to_state(root), yaw_flag != 0, lw, yw);
  return t;
}
void ref_tree_free(void *t) { delete static_cast<Tree *>(t); }
int ref_tree_size(void *t) { return static_cast<Tree *>(t)->t.getNumVertices(); }

/* addVertex + addEdge + addAction, the reference's insertion sequence */
void ref_tree_add(void *tp, int idx, const double *s, int parent, const double *a) {
  PlannerClass &t = static_cast<Tree *>(tp)->t;
  t.addVertex(idx, to_state(s));
  t.addEdge(parent, idx);
  t.addAction(idx, to_action(a));
}
void ref_tree_update_gy(void *tp, int idx, double g, double y) {
  static_cast<Tree *>(tp)->t.updateGYValue(idx, g, y);
}
/* rows 0..n-1; the root's parent is written as -1 */
void ref_tree_dump(void *tp, int n, double *v, double *a, int32_t *parent, double *g, double *y) {
  PlannerClass &t = static_cast<Tree *>(tp)->t;
  for (int i = 0; i < n; i++) {
    put(v + 8 * i, t.getVertex(i));
    put(a + 10 * i, t.getAction(i));
    parent[i] = i == 0 ? -1 : t.getPredecessor(i);
    g[i] = t.getGValue(i);
    y[i] = t.getYValue(i);
  }
}
void ref_tree_nearest(void *tp, int64_t n, const double *q, int32_t *out) {
  PlannerClass &t = static_cast<Tree *>(tp)->t;
  for (int64_t i = 0; i < n; i++) out[i] = t.getNearestNeighbor(to_state(q + 8 * i));
}
int ref_tree_neighborhood_dist(void *tp, const double *q, double dist, int cap, int32_t *out) {
  std::vector<int> r = static_cast<Tree *>(tp)->t.neighborhoodDist(to_state(q), dist);
  for (int i = 0; i < (int)r.size() && i < cap; i++) out[i] = r[i];
  return (int)r.size();
}
int ref_tree_neighborhood_n(void *tp, const double *q, int N, int32_t *out) {
  std::vector<int> r = static_cast<Tree *>(tp)->t.neighborhoodN(to_state(q), N);
  for (int i = 0; i < (int)r.size(); i++) out[i] = r[i];
  return (int)r.size();
}
int ref_tree_connect(void *tp, void *Tp, const double *s, int direction, int adaptive) {
  Planner p;
  configure(p, adaptive);
  return p.connect(static_cast<Tree *>(tp)->t, to_state(s), *static_cast<FastTerrainMap *>(Tp),
                   direction);
}
/* pathFromStart(idx) with getStateSequence / getActionSequence on it and
 * getActionSequenceReverse on the reversed path; returns the path's length */
int ref_tree_path(void *tp, int idx, int32_t *path, double *states, double *actions,
                  double *actions_rev) {
  PlannerClass &t = static_cast<Tree *>(tp)->t;
  Planner p;
  std::vector<int> pa = p.pathFromStart(t, idx);
  std::vector<State> ss = p.getStateSequence(t, pa);
  std::vector<Action> as = p.getActionSequence(t, pa);
  std::vector<int> rev(pa.rbegin(), pa.rend());
  std::vector<Action> ar = p.getActionSequenceReverse(t, rev);
  for (size_t i = 0; i < pa.size(); i++) path[i] = pa[i], put(states + 8 * i, ss[i]);
  for (size_t i = 0; i < as.size(); i++) put(actions + 10 * i, as[i]);
  for (size_t i = 0; i < ar.size(); i++) put(actions_rev + 10 * i, ar[i]);
  return (int)pa.size();
}
/* getStateAndActionSequences; returns the state count (actions: one fewer) */
int ref_join(void *ta, void *tb, int ia, int ib, double *states, double *actions) {
  Planner p;
  std::vector<State> ss;
  std::vector<Action> as;
  p.getStateAndActionSequences(static_cast<Tree *>(ta)->t, static_cast<Tree *>(tb)->t, ia, ib, ss, as);
  for (size_t i = 0; i < ss.size(); i++) put(states + 8 * i, ss[i]);
  for (size_t i = 0; i < as.size(); i++) put(actions + 10 * i, as[i]);
  return (int)ss.size();
}

/* ---- postProcessPath on n states / n-1 actions; returns the new state count ---- */
int ref_post_process(void *Tp, int n, const double *states, const double *actions, int adaptive,
                     int yaw_flag, double lw, double yw, double *out_states, double *out_actions,
                     double *figures /* length, yaw, cost */) {
  Planner p;
  configure(p, adaptive);
  p.set_cost_add_yaw(yaw_flag != 0, lw, yw);
  std::vector<State> ss;
  std::vector<Action> as;
  for (int i = 0; i < n; i++) ss.push_back(to_state(states + 8 * i));
  for (int i = 0; i + 1 < n; i++) as.push_back(to_action(actions + 10 * i));
  p.postProcessPath(ss, as, *static_cast<FastTerrainMap *>(Tp));
  for (size_t i = 0; i < ss.size(); i++) put(out_states + 8 * i, ss[i]);
  for (size_t i = 0; i < as.size(); i++) put(out_actions + 10 * i, as[i]);
  figures[0] = p.length(), figures[1] = p.yaw(), figures[2] = p.cost();
  return (int)ss.size();
}

/* ---- extend, for record and replay: the caller seeds rand() once, queries
 * the nearest vertex, calls this and dumps the tree.  star: RRTStarConnectClass::
 * extend, else RRTClass::extend. ---- */
void ref_srand(unsigned seed) { srand(seed); }
int ref_extend(void *tp, void *Tp, const double *target, int direction, int adaptive, int star) {
  Planner p;
  configure(p, adaptive);
  PlannerClass &t = static_cast<Tree *>(tp)->t;
  FastTerrainMap &T = *static_cast<FastTerrainMap *>(Tp);
  return star ? p.extend(t, to_state(target), T, direction)
              : p.RRTClass::extend(t, to_state(target), T, direction);
}

}  // extern "C"
