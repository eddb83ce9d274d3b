// gbp_tree_prune.cpp — see gbp_tree_prune.h
#include "gbp_tree_prune.h"

namespace gbp_amd {

int64_t applyPruneRemap(const int32_t *remap, int64_t n, State *v, Action *a, int32_t *parent,
                        double *g) {
  if (n < 1 || !remap || !v || !a || !parent || remap[0] != 0 || parent[0] != -1) return -1;
  // the whole map is checked before the first row moves
  int64_t kept = 0;
  for (int64_t i = 0; i < n; i++) {
    if (remap[i] < 0) continue;
    if (remap[i] != kept) return -1;
    if (i > 0 && (parent[i] < 0 || parent[i] >= n || remap[parent[i]] < 0)) return -1;
    kept++;
  }
  // a row moves down or stays (remap[i] <= i), so no unread row is overwritten;
  // a parent is renumbered from remap, never from a moved row
  for (int64_t i = 0; i < n; i++) {
    const int64_t j = remap[i];
    if (j < 0) continue;
    const int32_t p = parent[i];
    v[j] = v[i];
    a[j] = a[i];
    if (g) g[j] = g[i];
    parent[j] = p >= 0 ? remap[p] : -1;
  }
  return kept;
}

bool applyPruneRemap(const std::vector<int32_t> &remap, TreeDump &trees, int k) {
  const size_t n = remap.size();
  if (k < 0 || k > 1 || trees.v[k].size() != n || trees.a[k].size() != n ||
      trees.parent[k].size() != n || trees.g[k].size() != n)
    return false;
  const int64_t kept = applyPruneRemap(remap.data(), (int64_t)n, trees.v[k].data(), trees.a[k].data(),
                                       trees.parent[k].data(), trees.g[k].data());
  if (kept < 0) return false;
  trees.v[k].resize(kept);
  trees.a[k].resize(kept);
  trees.parent[k].resize(kept);
  trees.g[k].resize(kept);
  return true;
}

bool applyTrimRemap(const std::vector<int32_t> &remap, const std::vector<uint8_t> &keep, TreeDump &trees,
                    int k, TrimRemapRecord *rec) {
  const size_t n = remap.size();
  if (k < 0 || k > 1 || n < 1 || keep.size() != n || trees.parent[k].size() != n || !keep[0]) return false;
  const std::vector<int32_t> &parent = trees.parent[k];
  TrimRemapRecord r;
  r.n_before = (int64_t)n;
  for (size_t i = 0; i < n; i++) {
    if (remap[i] >= 0) {
      if (!keep[i]) return false;
      r.n_kept++;
    } else if (!keep[i]) {
      r.n_flagged++;
    } else {  // dropped with its flag set: only below a dropped parent
      if (i == 0 || parent[i] < 0 || (size_t)parent[i] >= n || remap[parent[i]] >= 0) return false;
      r.n_inherited++;
    }
  }
  if (!applyPruneRemap(remap, trees, k)) return false;
  if (rec) *rec = r;
  return true;
}

int64_t applyRerootRemap(const int32_t *remap, int64_t n, int32_t new_root, State *v, Action *a,
                         int32_t *parent, double *g) {
  if (n < 1 || !remap || !v || !a || !parent || new_root < 0 || new_root >= n || remap[new_root] != 0)
    return -1;
  // the whole map is checked before the first row moves
  int64_t kept = 1;
  for (int64_t i = 0; i < n; i++) {
    if (i == new_root || remap[i] < 0) continue;
    if (remap[i] != kept) return -1;
    if (parent[i] < 0 || parent[i] >= n || remap[parent[i]] < 0) return -1;
    kept++;
  }
  // the new root's row is set aside: a later row may land on its place.  Every
  // other kept row moves down or stays (vertex 0 is not kept unless it is the
  // new root, so at most i - 1 kept rows precede row i), and never onto row 0.
  const State root_v = v[new_root];
  const double root_g = g ? g[new_root] : 0.0;
  for (int64_t i = 0; i < n; i++) {
    const int64_t j = remap[i];
    if (i == new_root || j < 0) continue;
    const int32_t p = parent[i];
    v[j] = v[i];
    a[j] = a[i];
    if (g) g[j] = g[i];
    parent[j] = remap[p];
  }
  v[0] = root_v;
  a[0].fill(0.0);
  if (g) g[0] = root_g;
  parent[0] = -1;
  return kept;
}

bool applyRerootRemap(const std::vector<int32_t> &remap, int32_t new_root, TreeDump &trees, int k) {
  const size_t n = remap.size();
  if (k < 0 || k > 1 || trees.v[k].size() != n || trees.a[k].size() != n ||
      trees.parent[k].size() != n || trees.g[k].size() != n)
    return false;
  const int64_t kept = applyRerootRemap(remap.data(), (int64_t)n, new_root, trees.v[k].data(),
                                        trees.a[k].data(), trees.parent[k].data(), trees.g[k].data());
  if (kept < 0) return false;
  trees.v[k].resize(kept);
  trees.a[k].resize(kept);
  trees.parent[k].resize(kept);
  trees.g[k].resize(kept);
  return true;
}

bool applyGraftRemap(const std::vector<int32_t> &remap, const State &root,
                     const std::vector<uint8_t> &attach, const std::vector<Action> &actions,
                     TreeDump &trees, int k) {
  const size_t n = remap.size();
  if (k < 0 || k > 1 || n < 1 || attach.size() != n || actions.size() != n || trees.v[k].size() != n ||
      trees.a[k].size() != n || trees.parent[k].size() != n || trees.g[k].size() != n)
    return false;
  const std::vector<int32_t> &parent = trees.parent[k];
  // the whole map is checked before the first row moves
  int64_t kept = 1;
  for (size_t i = 0; i < n; i++) {
    if (remap[i] < 0) {
      if (attach[i]) return false;
      continue;
    }
    if (remap[i] != kept) return false;
    if (!attach[i] && (parent[i] < 0 || (size_t)parent[i] >= n || remap[parent[i]] < 0)) return false;
    kept++;
  }
  // out of place: with every vertex kept the rows move up by one
  std::vector<State> v((size_t)kept);
  std::vector<Action> a((size_t)kept);
  std::vector<int32_t> p((size_t)kept);
  std::vector<double> g((size_t)kept);
  v[0] = root;
  a[0].fill(0.0);
  p[0] = -1;
  g[0] = 0.0;
  for (size_t i = 0; i < n; i++) {
    const int64_t j = remap[i];
    if (j < 0) continue;
    v[j] = trees.v[k][i];
    a[j] = attach[i] ? actions[i] : trees.a[k][i];
    p[j] = attach[i] ? 0 : remap[parent[i]];
    g[j] = trees.g[k][i];
  }
  trees.v[k] = std::move(v);
  trees.a[k] = std::move(a);
  trees.parent[k] = std::move(p);
  trees.g[k] = std::move(g);
  return true;
}

}  // namespace gbp_amd
