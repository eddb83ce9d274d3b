// gbp_tree_maint.hip — a device tree kept through a change: pruned against a
// changed terrain (gbp_tree_revalidate_dev, gbp_tree_prune_dev,
// gbp_tree_revalidate_host / _keep_host) or re-rooted at one of
// its vertices (gbp_tree_reroot_dev, gbp_tree_reroot_host / _keep_host,
// gbp_tree_reroot_last) or grafted onto a root state that is none
// of them (gbp_tree_graft_dev, gbp_tree_graft_host / _keep_host; DESIGN §5.11;
// its stage A is gbp_tree_graft.hip's).  A translation unit of its own beside
// gbp_replan.hip: the planner loop (gbp_plan.hip) does not depend on it.
//
// Both are one pipeline (tree_keep) around a new root k, the prune with k = 0:
// k_prune_gather writes every edge as an attempt row for the validate kernels
// (the prune's stage A), k_keep_seed / k_keep_jump find the vertices below k
// whose edges up to k all hold, k_keep_count / k_keep_scan / k_keep_rank
// number them in order with k first (gbp_compact.h), and k_prune_move_rows /
// k_prune_move_links move them into fresh arrays.  The re-root (DEPTH) sums the
// depth below k along the jumps and derives g again level by level
// (k_reroot_levels / k_reroot_order sort the vertices by depth,
// k_reroot_g_wide / k_reroot_g_narrow write g).  The graft (GRAFT) is the
// re-root at one more vertex, the root state, under which the attached
// vertices hang (k_graft_attach, k_graft_root).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <type_traits>
#include <vector>

#include "gbp.h"
#include "gbp_compact.h"
#include "gbp_device.h"
#include "gbp_internal.h"

using namespace gbp;

namespace {

// ============================================================================
// the edges as attempt rows (gbp_tree_revalidate_dev)
// ============================================================================
// Stage A: edge (parent[i] -> i), i in [1, n), as attempt row i - 1 of the
// validate kernels: s = v[parent[i]], a = a[i].  One 16-B piece per thread, a
// row's 9 pieces (4 of s, 5 of a) on consecutive lanes.  n must be the tree's
// device count: otherwise nothing of the tree is read (every row zero) and
// edge_valid[0] = 0 tells the caller.
constexpr int PRUNE_PIECES = 9;
__global__ __launch_bounds__(TB) void k_prune_gather(gbp_tree t, int32_t n, double2 *__restrict__ rs,
                                                     double2 *__restrict__ ra,
                                                     uint8_t *__restrict__ edge_valid,
                                                     uint32_t *__restrict__ flags) {
  const bool ok = *t.count == n;
  const double2 *tv = (const double2 *)t.v, *ta = (const double2 *)t.a;
  const int64_t pieces = (int64_t)(n - 1) * PRUNE_PIECES;
  const int64_t first = (int64_t)blockIdx.x * TB + threadIdx.x;
  for (int64_t x = first; x < pieces; x += (int64_t)gridDim.x * TB) {
    const int64_t row = x / PRUNE_PIECES, i = row + 1;
    const int k = (int)(x - row * PRUNE_PIECES);
    double2 val = make_double2(0.0, 0.0);
    if (k < 4) {
      const int32_t p = ok ? t.parent[i] : -1;
      if (p >= 0 && p < n) val = tv[4 * (int64_t)p + k];
      rs[4 * row + k] = val;
    } else {
      if (ok) val = ta[5 * i + (k - 4)];
      ra[5 * row + (k - 4)] = val;
    }
  }
  if (first == 0) {  // the root is never tested
    edge_valid[0] = ok ? 1 : 0;
    flags[0] = 0;
  }
}

// ============================================================================
// the keep rule and the compaction (tree_keep); DEPTH: the re-root's form
// ============================================================================
// The keep rule by pointer jumping.  A vertex's word is (ancestor << 1) | dead:
// after r rounds its 2^r-th ancestor (a terminal once the path is shorter) and
// whether one of the 2^r edges up to it failed.  Two terminals: the new root k
// is its own ancestor and never dead, the old root is its own ancestor and
// dead (with k = 0, the prune, they are one vertex and the second case is
// never reached).  A round reads one buffer and writes the other, so every
// word read is the previous round's whatever the workgroups' order;
// ceil(log2 n) rounds reach a terminal from every vertex (a path has at most
// n - 1 edges).  After them a vertex's ancestor is k exactly when it lies
// below k, and its dead bit then tells whether an edge between the two failed.
// A parent outside [0, n) counts as a failed edge below the old root.
// With DEPTH a second pair of buffers carries the number of edges jumped so
// far (terminals add 0): integer sums are associative, so the depth below k
// is exact.  edge_valid may be null (every edge holds); edge_valid[k] is never
// read.
//
// GRAFT (the graft): the tree of n vertices whose last one, k =
// n - 1, is the new root state and has no row in parent / edge_valid /
// attach; an attached vertex's parent is k and its own old edge is ignored,
// the old root included.  Everything else is the re-root at k.
template <bool DEPTH, bool GRAFT = false>
__global__ __launch_bounds__(TB) void k_keep_seed(const int32_t *__restrict__ parent,
                                                  const uint8_t *__restrict__ edge_valid,
                                                  const uint8_t *__restrict__ attach, int32_t n,
                                                  int32_t k, uint32_t *__restrict__ w,
                                                  uint32_t *__restrict__ d) {
  const int32_t nv = GRAFT ? k : n;  // the vertices parent[] may name
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
    uint32_t x, e = 0;
    if (i == k) {
      x = (uint32_t)k << 1;
    } else if (GRAFT && attach[i]) {
      x = (uint32_t)k << 1;
      e = 1u;
    } else if (i == 0) {
      x = 1u;
    } else {
      const int32_t p = parent[i];
      const bool in = p >= 0 && p < nv;
      x = in ? ((uint32_t)p << 1) | ((edge_valid && !edge_valid[i]) ? 1u : 0u) : 1u;
      e = in ? 1u : 0u;
    }
    w[i] = x;
    if constexpr (DEPTH) d[i] = e;
  }
}

template <bool DEPTH>
__global__ __launch_bounds__(TB) void k_keep_jump(const uint32_t *__restrict__ ws,
                                                  const uint32_t *__restrict__ ds,
                                                  uint32_t *__restrict__ wd,
                                                  uint32_t *__restrict__ dd, int32_t n) {
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
    const uint32_t x = ws[i], y = ws[x >> 1];
    wd[i] = (y & ~1u) | ((x | y) & 1u);
    if constexpr (DEPTH) dd[i] = ds[i] + ds[x >> 1];
  }
}

// below k: the walk ended at k.  The prune does not ask: every vertex of a
// tree lies below its root, and on a malformed parent array a vertex on a
// cycle reaches no terminal (its word's ancestor is some vertex of the cycle),
// which the prune has always kept and counted by its dead bit and its own edge
// alone, while the re-root puts it outside.  The two rules are kept as they
// were.
template <bool DEPTH>
__device__ __forceinline__ bool keep_below(uint32_t w, int32_t k) {
  if constexpr (DEPTH)
    return (w >> 1) == (uint32_t)k;
  else
    return true;
}

// a tile's record: its kept vertices other than k, those below k whose own
// edge failed, and with DEPTH those not below k and the largest depth of a
// kept vertex
template <bool DEPTH>
using KeepTile = TileRec<DEPTH ? 4 : 2>;
template <bool DEPTH>
using KeepStats = std::conditional_t<DEPTH, gbp_reroot_stats, gbp_prune_stats>;

template <bool DEPTH, bool GRAFT = false>
__global__ __launch_bounds__(CB) void k_keep_count(const uint32_t *__restrict__ w,
                                                   const uint32_t *__restrict__ d,
                                                   const uint8_t *__restrict__ edge_valid,
                                                   const uint8_t *__restrict__ attach, int32_t n,
                                                   int32_t k, KeepTile<DEPTH> *__restrict__ tile) {
  const int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x;
  const bool in = i < n;
  const uint32_t x = in ? w[i] : 1u;
  const bool below = in && keep_below<DEPTH>(x, k);
  const bool keep = below && !(x & 1u);
  const bool bad = below && i != k && !(GRAFT && attach[i]) && edge_valid && !edge_valid[i];
  KeepTile<DEPTH> t;
  if constexpr (DEPTH)
    t = tile_count<4, true>({keep && i != k, bad, in && !below}, keep ? d[i] : 0u);
  else
    t = tile_count<2>({keep && i != k, bad});
  if (threadIdx.x == 0) tile[blockIdx.x] = t;
}

// one workgroup: toff[b] = 1 + the kept vertices other than k of the tiles
// before b (k itself becomes vertex 0); the stats record and the tree's new count
template <bool DEPTH>
__global__ __launch_bounds__(CB) void k_keep_scan(const KeepTile<DEPTH> *__restrict__ tile,
                                                  int64_t ntile, uint32_t *__restrict__ toff, int32_t n,
                                                  KeepStats<DEPTH> *__restrict__ stats,
                                                  int32_t *__restrict__ count) {
  const KeepTile<DEPTH> tot =
      tile_scan<DEPTH ? 4 : 2, DEPTH>([tile](int64_t b) { return tile[b]; }, ntile, 1u, toff);
  if (threadIdx.x == 0) {
    const uint32_t kept = tot.c[0], bad = tot.c[1];
    stats->n_before = n;
    stats->n_kept = kept;
    stats->n_edge_invalid = bad;
    if constexpr (DEPTH) {
      stats->n_outside = tot.c[2];
      stats->n_inherited = (int64_t)n - kept - bad - tot.c[2];
      stats->depth = tot.c[3];
    } else {
      stats->n_inherited = (int64_t)n - kept - bad;
    }
    *count = (int32_t)kept;
  }
}

// remap (k -> 0, the other kept vertices from 1 in their order); with DEPTH
// every kept vertex's depth under its new index and the levels' sizes (hist
// zeroed before this launch; an integer count does not depend on the atomics'
// order).  GRAFT: k has no entry in remap.
template <bool DEPTH, bool GRAFT = false>
__global__ __launch_bounds__(CB) void k_keep_rank(const uint32_t *__restrict__ w,
                                                  const uint32_t *__restrict__ d, int32_t n, int32_t k,
                                                  const uint32_t *__restrict__ toff,
                                                  int32_t *__restrict__ remap,
                                                  uint32_t *__restrict__ depth,
                                                  uint32_t *__restrict__ hist) {
  const int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x;
  const uint32_t x = i < n ? w[i] : 1u;
  const bool keep = i < n && keep_below<DEPTH>(x, k) && !(x & 1u);
  const uint32_t at = tile_rank(keep && i != k, toff[blockIdx.x]);
  if (i >= n) return;
  const int32_t j = !keep ? -1 : i == k ? 0 : (int32_t)at;
  if (!GRAFT || i != k) remap[i] = j;
  if constexpr (DEPTH) {
    if (j >= 0) {
      depth[j] = d[i];
      atomicAdd(&hist[d[i]], 1u);
    }
  }
}

// the kept rows of v and a into the fresh arrays, in 16-B pieces like the gather
__global__ __launch_bounds__(TB) void k_prune_move_rows(gbp_tree o, gbp_tree f, int32_t n,
                                                        const int32_t *__restrict__ remap) {
  const double2 *ov = (const double2 *)o.v, *oa = (const double2 *)o.a;
  double2 *fv = (double2 *)f.v, *fa = (double2 *)f.a;
  const int64_t pieces = (int64_t)n * PRUNE_PIECES;
  for (int64_t x = (int64_t)blockIdx.x * TB + threadIdx.x; x < pieces; x += (int64_t)gridDim.x * TB) {
    const int64_t i = x / PRUNE_PIECES;
    const int k = (int)(x - i * PRUNE_PIECES);
    const int64_t j = remap[i];
    if (j < 0) continue;
    if (k < 4)
      fv[4 * j + k] = ov[4 * i + k];
    else
      fa[5 * j + (k - 4)] = oa[5 * i + (k - 4)];
  }
}

// the next kept vertex of a successor list from c on (c itself included),
// renumbered; -1 at the list's end.  A list holds at most n vertices: the walk
// stops there whatever the arrays hold.  GRAFT: an attached vertex has left
// its old parent's list, kept though it is.
template <bool GRAFT>
__device__ __forceinline__ int32_t prune_next_kept(int32_t c, const int32_t *__restrict__ link,
                                                   const int32_t *__restrict__ remap,
                                                   const uint8_t *__restrict__ attach, int32_t n) {
  for (int32_t steps = 0; c >= 0 && c < n && steps < n; c = link[c], steps++)
    if (remap[c] >= 0 && !(GRAFT && attach[c])) return remap[c];
  return -1;
}

// a kept vertex's g (copied: it is g[parent] + poseDistance already), its
// parent renumbered, its fp16 row (hm zeroed before this launch), and its
// places in the successor lists: the old lists with the pruned vertices left
// out, so each list keeps its order.  Every word written belongs to the
// vertex's own fresh row.  A new root's old parent is not kept, so its parent
// becomes -1 and it is in no list.  GRAFT: n is the old tree's size; an
// attached vertex's parent and places in the root's list are k_graft_root's.
template <bool GRAFT = false>
__global__ __launch_bounds__(TB) void k_prune_move_links(gbp_tree o, gbp_tree f, int32_t n,
                                                         const int32_t *__restrict__ remap,
                                                         const uint8_t *__restrict__ attach) {
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
    const int32_t j = remap[i];
    if (j < 0) continue;
    const int32_t p = o.parent[i];
    f.parent[j] = (p >= 0 && p < n) ? remap[p] : -1;
    f.g[j] = o.g[i];
    double s[8];
    copy8(s, o.v + 8 * i);
    nn_put_hrow(f.vh, f.hm, j, s, false);
    f.child[j] = prune_next_kept<GRAFT>(o.child[i], o.sibling, remap, attach, n);
    f.sibling[j] = prune_next_kept<GRAFT>(o.sibling[i], o.sibling, remap, attach, n);
    f.prev[j] = prune_next_kept<GRAFT>(o.prev[i], o.prev, remap, attach, n);
  }
}

// ============================================================================
// the re-root's own part: g derived again, level by level
// ============================================================================
// one workgroup, after the move: first[r] = the kept vertices of the levels
// before r, r in [0, depth + 1] (hist keeps the sizes for k_reroot_order), and
// the new root's action zeroed as k_tree_init writes it
__global__ __launch_bounds__(CB) void k_reroot_levels(const uint32_t *__restrict__ hist,
                                                      const gbp_reroot_stats *__restrict__ stats,
                                                      uint32_t *__restrict__ first, double *__restrict__ a) {
  const int64_t nl = stats->depth + 1;
  const TileRec<1> tot = tile_scan<1>([hist](int64_t r) { return TileRec<1>{{hist[r]}}; }, nl, 0u, first);
  if (threadIdx.x == 0) first[nl] = tot.c[0];
  if (threadIdx.x < 10) a[threadIdx.x] = 0.0;
}

// the counting sort's scatter: order[first[r] ..] = the vertices of level r.
// Their order within a level depends on the atomics and is immaterial: a
// vertex's g depends on its parent's alone.
__global__ __launch_bounds__(TB) void k_reroot_order(const uint32_t *__restrict__ depth,
                                                     const int32_t *__restrict__ count,
                                                     const uint32_t *__restrict__ first,
                                                     uint32_t *__restrict__ hist,
                                                     int32_t *__restrict__ order) {
  const int64_t m = *count;
  for (int64_t j = (int64_t)blockIdx.x * TB + threadIdx.x; j < m; j += (int64_t)gridDim.x * TB) {
    const uint32_t r = depth[j];
    order[first[r] + atomicSub(&hist[r], 1u) - 1u] = (int32_t)j;
  }
}

// g of one vertex from its parent's, as k_tree_load derives it
__device__ __forceinline__ void reroot_g(const gbp_tree &t, int32_t c) {
  const int32_t p = t.parent[c];
  t.g[c] = p >= 0 ? t.g[p] + pose_distance(t.v + 8 * (int64_t)p, t.v + 8 * (int64_t)c) : 0.0;
}

// g by levels.  A level's vertices read the g their parents' level wrote: the
// two are separated by a kernel boundary (a level wider than a workgroup is a
// launch of its own over its slice of `order`) or by the barrier between the
// steps of the one workgroup that walks a run of narrow levels.  No workgroup
// waits for another.
__global__ __launch_bounds__(TB) void k_reroot_g_wide(gbp_tree t, const int32_t *__restrict__ order,
                                                      int64_t lo, int64_t hi) {
  for (int64_t x = lo + (int64_t)blockIdx.x * TB + threadIdx.x; x < hi; x += (int64_t)gridDim.x * TB)
    reroot_g(t, order[x]);
}

__global__ __launch_bounds__(TB) void k_reroot_g_narrow(gbp_tree t, const int32_t *__restrict__ order,
                                                        const uint32_t *__restrict__ first, int64_t r0,
                                                        int64_t r1) {
  for (int64_t r = r0; r < r1; r++) {
    const uint32_t x = first[r] + threadIdx.x;
    if (x < first[r + 1]) reroot_g(t, order[x]);
    __syncthreads();  // workgroup-scope release / acquire of the g just written
  }
}

// ============================================================================
// the graft's own part: the attached vertices under the new root
// ============================================================================
// after the move: an attached vertex hangs under the new root, vertex 0, by its
// connect action (every attached vertex is kept)
__global__ __launch_bounds__(TB) void k_graft_attach(gbp_tree f, int32_t n,
                                                     const int32_t *__restrict__ remap,
                                                     const uint8_t *__restrict__ attach,
                                                     const double *__restrict__ actions) {
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
    if (!attach[i]) continue;
    const int64_t j = remap[i];
    if (j < 0) continue;
    f.parent[j] = 0;
    copy10(f.a + 10 * j, actions + 10 * i);
  }
}

struct GraftState {  // the root state travels as the kernel's argument
  double s[8];
};

// one workgroup, after k_graft_attach: the new root's row (its action is
// k_reroot_levels'), its successor list (the vertices whose parent is 0, the
// attached ones and no others, in ascending index: att[] lists them, then
// each links to its neighbours) and the call's record from the keep's
__global__ __launch_bounds__(CB) void k_graft_root(gbp_tree f, GraftState R, int32_t *__restrict__ att,
                                                   const gbp_reroot_stats *__restrict__ rs,
                                                   gbp_graft_stats *__restrict__ gs) {
  __shared__ uint32_t sw[CB / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const int64_t m = *f.count;
  if (threadIdx.x == 0) {
    copy8(f.v, R.s);
    nn_put_hrow(f.vh, f.hm, 0, R.s, false);
    f.parent[0] = -1;
    f.g[0] = 0.0;
    f.sibling[0] = -1;
    f.prev[0] = -1;
  }
  uint32_t total = 0;  // the same in every thread
  for (int64_t base = 0; base < m; base += CB) {
    const int64_t j = base + threadIdx.x;
    const bool is = j >= 1 && j < m && f.parent[j] == 0;
    const unsigned long long bm = __ballot(is);
    if (lane == 0) sw[wv] = (uint32_t)__popcll(bm);
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int q = 0; q < CB / WAVE; q++) {
      if (q < wv) before += sw[q];
      all += sw[q];
    }
    if (is) att[total + before + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull))] = (int32_t)j;
    total += all;
    __syncthreads();  // sw is read before the next pass writes it; att before the links read it
  }
  for (uint32_t x = threadIdx.x; x < total; x += CB) {
    const int32_t j = att[x];
    f.sibling[j] = x + 1 < total ? att[x + 1] : -1;
    f.prev[j] = x > 0 ? att[x - 1] : -1;
  }
  if (threadIdx.x == 0) {
    f.child[0] = total ? att[0] : -1;
    gs->n_before = rs->n_before - 1;  // (the keep counted the root state's vertex)
    gs->n_kept = rs->n_kept;
    gs->n_candidates = 0;
    gs->n_checked = 0;
    gs->n_attached = total;
    gs->n_outside = rs->n_outside;
    gs->n_edge_invalid = rs->n_edge_invalid;
    gs->n_inherited = rs->n_inherited;
    gs->depth = rs->depth;
  }
}

// ============================================================================
// host side
// ============================================================================
// stage A's attempt rows in the tree's own grow-only buffer (the call only
// enqueues: nothing of it may be freed when it returns)
int prune_rows(gbp_tree *tree, int64_t n, double *&rs, double *&ra) {
  auto carve = [&](Stage &S) { S.take(rs, 8 * (n - 1)); S.take(ra, 10 * (n - 1)); };
  const int rc = ensure_ws(&tree->rv, &tree->rv_bytes, stage_bytes_of(carve));
  return rc ? rc : stage_carve(tree->rv, tree->rv_bytes, carve);
}
int prune_args(const gbp_tree *tree, int64_t n, bool arrays) {
  if (!tree_ok(tree)) return GBP_E_BAD_HANDLE;
  if (n < 1 || !arrays) return GBP_E_INVALID_ARG;
  return n > tree->cap ? GBP_E_SHAPE : GBP_OK;
}

// What a re-root adds to tree_keep (RerootDepth below); the prune adds nothing.
struct NoDepth {
  static constexpr bool DEPTH = false, GRAFT = false;
  using Stats = gbp_prune_stats;
  const uint8_t *attach = nullptr;
  uint32_t *d[2] = {nullptr, nullptr}, *depth = nullptr, *hist = nullptr;
  void carve(Stage &, int64_t) {}
  gbp_prune_stats *keep_stats(gbp_prune_stats *s) { return s; }
  void mark(int, hipStream_t) {}
  bool before_rank(int64_t, hipStream_t) { return true; }
  int after_move(const gbp_tree &, int64_t, unsigned, const gbp_prune_stats *, hipStream_t) {
    return GBP_OK;
  }
};

// The tree's vertices below k whose edges up to k all hold (edge_valid; null:
// every edge), moved into fresh arrays in their order with k first; remap and
// stats written on the device.  The survivors get arrays, a count and search
// bounds of their own: until the swap at the end the tree is untouched, so a
// failed call leaves it as it was.  Synchronises the stream.
// The graft (Extra::GRAFT, GraftRoot below) runs the rule on nv = n + 1
// vertices, the last one the new root state k = n, which has no row in the
// tree: the moves take the n old rows, and the fresh arrays hold nv rows at
// least.
template <class Extra>
int tree_keep(gbp_tree *tree, int64_t n, int32_t k, const uint8_t *edge_valid, int32_t *remap,
              typename Extra::Stats *stats, hipStream_t s, Extra &x) {
  constexpr bool DEPTH = Extra::DEPTH, GRAFT = Extra::GRAFT;
  int rc = prune_args(tree, n, remap && stats && (DEPTH || edge_valid));
  if (rc) return rc;
  int64_t have = 0;
  if ((rc = gbp_tree_size(tree, &have, s))) return rc;  // synchronises
  if (have != n) return GBP_E_SHAPE;
  const int64_t nv = n + (GRAFT ? 1 : 0);
  if (GRAFT) k = (int32_t)n;
  if (k < 0 || k >= nv || nv > 0x7FFFFFFF) return GBP_E_INVALID_ARG;
  DeviceGuard g(tree->device);
  const int64_t ntile = (nv + CB - 1) / CB;
  DevBuf buf;
  uint32_t *w[2], *toff;
  KeepTile<DEPTH> *tile;
  rc = stage_buf(buf, [&](Stage &S) {
    S.take(w[0], nv); S.take(w[1], nv); S.take(tile, ntile); S.take(toff, ntile);
    x.carve(S, nv);
  });
  if (rc) return rc;
  KeepStats<DEPTH> *kst = x.keep_stats(stats);
  gbp_tree fresh = *tree;
  const int64_t cap = nv > tree->cap ? std::min<int64_t>(std::max(2 * tree->cap, nv), 0x7FFFFFFF) : tree->cap;
  if ((rc = tree_alloc(&fresh, cap))) return rc;
  fresh.count = nullptr;
  fresh.hm = nullptr;
  auto drop_fresh = [&](int code) {
    (void)hipDeviceSynchronize();
    tree_free_arrays(&fresh);
    if (fresh.count) (void)hipFree(fresh.count);
    if (fresh.hm) (void)hipFree(fresh.hm);
    return code;
  };
  if (hipMalloc(&fresh.count, 4) != hipSuccess || hipMalloc(&fresh.hm, 64) != hipSuccess)
    return drop_fresh(GBP_E_ALLOC);
  const unsigned gv = grid_for(nv, TB, 2048);
  x.mark(0, s);
  hipLaunchKernelGGL((k_keep_seed<DEPTH, GRAFT>), dim3(gv), dim3(TB), 0, s, tree->parent, edge_valid,
                     x.attach, (int32_t)nv, k, w[0], x.d[0]);
  int cur = 0;  // ceil(log2 nv) rounds, back to back
  for (int64_t reach = 1; reach < nv; reach <<= 1, cur ^= 1)
    hipLaunchKernelGGL(k_keep_jump<DEPTH>, dim3(gv), dim3(TB), 0, s, w[cur], x.d[cur], w[cur ^ 1],
                       x.d[cur ^ 1], (int32_t)nv);
  x.mark(1, s);
  hipLaunchKernelGGL((k_keep_count<DEPTH, GRAFT>), dim3((unsigned)ntile), dim3(CB), 0, s, w[cur],
                     x.d[cur], edge_valid, x.attach, (int32_t)nv, k, tile);
  hipLaunchKernelGGL(k_keep_scan<DEPTH>, dim3(1), dim3(CB), 0, s, tile, ntile, toff, (int32_t)nv, kst,
                     fresh.count);
  if (hipGetLastError() != hipSuccess || hipMemsetAsync(fresh.hm, 0, 64, s) != hipSuccess ||
      !x.before_rank(nv, s))
    return drop_fresh(GBP_E_HIP);
  hipLaunchKernelGGL((k_keep_rank<DEPTH, GRAFT>), dim3((unsigned)ntile), dim3(CB), 0, s, w[cur], x.d[cur],
                     (int32_t)nv, k, toff, remap, x.depth, x.hist);
  hipLaunchKernelGGL(k_prune_move_rows, dim3(grid_for(n * PRUNE_PIECES, TB, 2048)), dim3(TB), 0, s, *tree,
                     fresh, (int32_t)n, remap);
  hipLaunchKernelGGL(k_prune_move_links<GRAFT>, dim3(gv), dim3(TB), 0, s, *tree, fresh, (int32_t)n, remap,
                     x.attach);
  if (hipGetLastError() != hipSuccess) return drop_fresh(GBP_E_HIP);
  if ((rc = x.after_move(fresh, nv, gv, kst, s))) return drop_fresh(rc);
  if (hipStreamSynchronize(s) != hipSuccess) return drop_fresh(GBP_E_HIP);
  tree_free_arrays(tree);
  (void)hipFree(tree->count);
  (void)hipFree(tree->hm);
  *tree = fresh;
  return GBP_OK;
}

// The synchronous entries' edge decisions: stage A into dev (edge_valid[n],
// then flags[n] at byte fl_at: one read-back), the FRAGILE edges re-decided
// with glibc and edge_valid written back.  dev holds the final decisions and
// nothing is in flight when this returns.
int tree_edge_decisions(gbp_terrain *t, gbp_tree *tree, int64_t n, int direction, int adaptive,
                        uint8_t *dev, size_t fl_at, int64_t *n_resolved, hipStream_t s) {
  const size_t dec_bytes = fl_at + (size_t)n * sizeof(uint32_t);
  uint32_t *dfl = (uint32_t *)(dev + fl_at);
  int rc = gbp_tree_revalidate_dev(t, tree, n, direction, adaptive, dev, dfl, s);
  if (rc) return rc;
  std::vector<uint8_t> dec(dec_bytes);
  if ((rc = d2h(dec.data(), dev, dec_bytes, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  uint8_t *ev = dec.data();
  uint32_t *fl = (uint32_t *)(dec.data() + fl_at);
  bool fragile = false;
  for (int64_t i = 1; i < n && !fragile; i++) fragile = (fl[i] & GBP_F_FRAGILE) != 0;
  if (fragile) {
    // the FRAGILE edges again with glibc, from the rows stage A gathered: the
    // rows in one copy, the decisions back in one
    double *rs = nullptr, *ra = nullptr;
    if ((rc = prune_rows(tree, n, rs, ra))) return rc;  // (the buffer stage A filled)
    std::vector<double> hs(8 * (n - 1)), ha(10 * (n - 1));
    if ((rc = d2h(hs.data(), rs, 8 * (n - 1), s))) return rc;
    if ((rc = d2h(ha.data(), ra, 10 * (n - 1), s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    rc = gbp_resolve_fragile_host(t, n - 1, hs.data(), ha.data(), nullptr, direction, adaptive, ev + 1,
                                  nullptr, nullptr, fl + 1, nullptr, n_resolved);
    if (!rc) rc = h2d(dev, ev, n, s);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));  // dec leaves scope only after the copy
  }
  return GBP_OK;
}

// The synchronous entries: the edges tested on terrain t (null, the re-root
// alone: no edge is tested), FRAGILE ones re-decided, then the prune (DEPTH
// false, k = 0) or the re-root at k; the remap read back and / or left in the
// caller's device array, the stats read back.
template <bool DEPTH>
int keep_host(gbp_terrain *t, gbp_tree *tree, int32_t k, int direction, int adaptive, int32_t *remap,
              int32_t *remap_dev, int64_t remap_cap, KeepStats<DEPTH> *stats, int64_t *n_resolved) {
  if (n_resolved) *n_resolved = 0;
  if ((!DEPTH && !t) || !tree_ok(tree)) return GBP_E_BAD_HANDLE;
  if (!stats || (t && direction != GBP_FORWARD && direction != GBP_REVERSE)) return GBP_E_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GBP_E_NO_DEVICE;
  if (t && !t->d_z) return GBP_E_BAD_HANDLE;
  DeviceGuard g(tree->device);
  hipStream_t s = t ? t->host_stream : nullptr;
  int64_t n = 0;
  int rc = gbp_tree_size(tree, &n, s);
  if (rc) return rc;
  if (DEPTH && (k < 0 || k >= n)) return GBP_E_INVALID_ARG;
  // edge_valid and flags back to back: one read-back
  const size_t fl_at = ((size_t)n + 255) & ~(size_t)255;
  const size_t dec_bytes = fl_at + (size_t)n * sizeof(uint32_t);
  DevBuf buf;
  uint8_t *dev;
  int32_t *dmap;
  KeepStats<DEPTH> *dst;
  if (remap_dev && n > remap_cap) return GBP_E_SHAPE;
  if (remap_dev) {  // the caller keeps the device remap: it must lie on the tree's device
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, remap_dev) != hipSuccess || at.device != tree->device) {
      (void)hipGetLastError();
      return GBP_E_INVALID_ARG;
    }
  }
  rc = stage_buf(buf, [&](Stage &S) {
    S.take(dev, dec_bytes);
    S.take(dmap, remap_dev ? 0 : n);
    S.take(dst, 1);
  });
  if (rc) return rc;
  if (remap_dev) dmap = remap_dev;
  if (t && (rc = tree_edge_decisions(t, tree, n, direction, adaptive, dev, fl_at, n_resolved, s)))
    return rc;
  if constexpr (DEPTH)
    rc = gbp_tree_reroot_dev(tree, n, k, t ? dev : nullptr, dmap, dst, s);
  else
    rc = gbp_tree_prune_dev(tree, n, dev, dmap, dst, s);
  if (rc) return rc;
  if (remap && (rc = d2h(remap, dmap, n, s))) return rc;
  if ((rc = d2h(stats, dst, 1, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  return GBP_OK;
}

// the last successful gbp_tree_reroot_dev / gbp_tree_graft_dev of the process,
// for gbp_tree_reroot_last / gbp_tree_graft_last
struct LastCall {
  double ms[3] = {0, 0, 0};
  int64_t launches = 0;
};
std::mutex last_mu;
LastCall reroot_last, graft_last;
// the four marks between the call's three parts; a mark that could not be
// created or recorded only leaves the times at zero
struct RerootMarks {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ok = true;
  RerootMarks() {
    for (auto &x : e) ok = hipEventCreate(&x) == hipSuccess && ok;
  }
  ~RerootMarks() {
    for (auto &x : e)
      if (x) (void)hipEventDestroy(x);
  }
  void mark(int k, hipStream_t s) { ok = ok && hipEventRecord(e[k], s) == hipSuccess; }
};

// The re-root's additions to tree_keep: the depth buffers of the jumps, the
// levels' sizes counted by the rank, and after the move the vertices sorted by
// level and g written again from the new root down; the marks between the
// call's three parts (keep rule | compaction, move and level sort | g) and
// the launches made.
struct RerootDepth {
  static constexpr bool DEPTH = true, GRAFT = false;
  using Stats = gbp_reroot_stats;
  const uint8_t *attach = nullptr;
  gbp_reroot_stats *keep_stats(gbp_reroot_stats *s) { return s; }
  uint32_t *d[2] = {nullptr, nullptr}, *depth = nullptr, *hist = nullptr, *first = nullptr;
  int32_t *order = nullptr;
  RerootMarks marks;
  int64_t launches = 8;  // seed, count, scan, rank, two moves, levels, order
  void carve(Stage &S, int64_t n) {
    S.take(d[0], n); S.take(d[1], n); S.take(depth, n); S.take(hist, n + 1); S.take(first, n + 2);
    S.take(order, n);
  }
  void mark(int k, hipStream_t s) { marks.mark(k, s); }
  bool before_rank(int64_t n, hipStream_t s) {
    return hipMemsetAsync(hist, 0, (n + 1) * sizeof(uint32_t), s) == hipSuccess;
  }
  // the g copied by the move is written again here
  int after_move(const gbp_tree &fresh, int64_t n, unsigned gv, const gbp_reroot_stats *stats,
                 hipStream_t s) {
    for (int64_t reach = 1; reach < n; reach <<= 1) launches++;  // the jump rounds
    hipLaunchKernelGGL(k_reroot_levels, dim3(1), dim3(CB), 0, s, hist, stats, first, fresh.a);
    hipLaunchKernelGGL(k_reroot_order, dim3(gv), dim3(TB), 0, s, depth, fresh.count, first, hist, order);
    marks.mark(2, s);
    HIPCHK(hipGetLastError());
    // the levels' sizes decide the launches of g
    gbp_reroot_stats hs;
    if (d2h(&hs, stats, 1, s) || hipStreamSynchronize(s) != hipSuccess) return GBP_E_HIP;
    const int64_t nl = hs.depth + 1;
    if (hs.n_kept < 1 || hs.n_kept > n || nl < 1 || nl > hs.n_kept) return GBP_E_HIP;
    std::vector<uint32_t> lv(nl + 1);
    if (d2h(lv.data(), first, nl + 1, s) || hipStreamSynchronize(s) != hipSuccess) return GBP_E_HIP;
    for (int64_t r = 0; r < nl; launches++) {
      if (lv[r + 1] - lv[r] > (uint32_t)TB) {
        hipLaunchKernelGGL(k_reroot_g_wide, dim3(grid_for(lv[r + 1] - lv[r], TB, 2048)), dim3(TB), 0, s,
                           fresh, order, (int64_t)lv[r], (int64_t)lv[r + 1]);
        r++;
        continue;
      }
      int64_t e = r + 1;  // a run of levels no wider than a workgroup
      while (e < nl && lv[e + 1] - lv[e] <= (uint32_t)TB) e++;
      hipLaunchKernelGGL(k_reroot_g_narrow, dim3(1), dim3(TB), 0, s, fresh, order, first, r, e);
      r = e;
    }
    marks.mark(3, s);
    HIPCHK(hipGetLastError());
    return GBP_OK;
  }
};

// a finished call's times between its marks and its launches into `to`
void keep_last(LastCall &to, const RerootDepth &x) {
  std::lock_guard<std::mutex> lk(last_mu);
  for (int q = 0; q < 3; q++) {
    float t = 0.f;
    to.ms[q] =
        x.marks.ok && hipEventElapsedTime(&t, x.marks.e[q], x.marks.e[q + 1]) == hipSuccess ? t : 0.0;
  }
  to.launches = x.launches;
}
int read_last(const LastCall &from, double ms[3], int64_t *launches) {
  if (!ms || !launches) return GBP_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(last_mu);
  for (int k = 0; k < 3; k++) ms[k] = from.ms[k];
  *launches = from.launches;
  return GBP_OK;
}

// The graft's additions to the re-root's: the keep's record in a buffer of its
// own (the call's is gbp_graft_stats), and after the move the attached
// vertices hung under the new root and the root's row, list and record
// (k_graft_attach, k_graft_root: before g is derived from them).  att, the
// root's children in order, lives in `order` until k_reroot_order fills it.
struct GraftRoot : RerootDepth {
  static constexpr bool GRAFT = true;
  using Stats = gbp_graft_stats;
  const double *actions = nullptr;
  const int32_t *remap = nullptr;
  GraftState root{};
  gbp_reroot_stats *rs = nullptr;
  gbp_graft_stats *out = nullptr;
  void carve(Stage &S, int64_t nv) {
    RerootDepth::carve(S, nv);
    S.take(rs, 1);
  }
  gbp_reroot_stats *keep_stats(gbp_graft_stats *s) {
    out = s;
    return rs;
  }
  int after_move(const gbp_tree &fresh, int64_t nv, unsigned gv, const gbp_reroot_stats *stats,
                 hipStream_t s) {
    launches += 2;
    hipLaunchKernelGGL(k_graft_attach, dim3(gv), dim3(TB), 0, s, fresh, (int32_t)(nv - 1), remap, attach,
                       actions);
    hipLaunchKernelGGL(k_graft_root, dim3(1), dim3(CB), 0, s, fresh, root, order, rs, out);
    HIPCHK(hipGetLastError());
    return RerootDepth::after_move(fresh, nv, gv, stats, s);
  }
};

bool has_nan8(const double *s) {
  for (int k = 0; k < 8; k++)
    if (s[k] != s[k]) return true;
  return false;
}

// The synchronous graft: stage A on t, with test_edges the edges' decisions
// as well (tree_edge_decisions), attach and the checks' flags back in one
// copy, the FRAGILE checks re-decided with glibc from the vertex's own row
// (attach and the action written back), then stage B.
int graft_host(gbp_terrain *t, gbp_tree *tree, const double *root, double radius, int direction,
               int adaptive, int test_edges, int32_t *remap, int32_t *remap_dev, int64_t remap_cap,
               gbp_graft_stats *stats, int64_t *n_resolved) {
  if (n_resolved) *n_resolved = 0;
  if (!t || !tree_ok(tree)) return GBP_E_BAD_HANDLE;
  if (!root || !stats || (direction != GBP_FORWARD && direction != GBP_REVERSE) || !(radius >= 0.0) ||
      has_nan8(root))
    return GBP_E_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GBP_E_NO_DEVICE;
  if (!t->d_z) return GBP_E_BAD_HANDLE;
  DeviceGuard g(tree->device);
  hipStream_t s = t->host_stream;
  int64_t n = 0;
  int rc = gbp_tree_size(tree, &n, s);
  if (rc) return rc;
  if (remap_dev && n > remap_cap) return GBP_E_SHAPE;
  if (remap_dev) {  // the caller keeps the device remap: it must lie on the tree's device
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, remap_dev) != hipSuccess || at.device != tree->device) {
      (void)hipGetLastError();
      return GBP_E_INVALID_ARG;
    }
  }
  // attach and flags back to back, like edge_valid and its flags: one read-back each
  const size_t fl_at = ((size_t)n + 255) & ~(size_t)255;
  const size_t dec_bytes = fl_at + (size_t)n * sizeof(uint32_t);
  DevBuf buf;
  uint8_t *dchk, *dedge;
  double *dact;
  int32_t *dmap;
  gbp_graft_stats *dst;
  rc = stage_buf(buf, [&](Stage &S) {
    S.take(dchk, dec_bytes);
    S.take(dedge, test_edges ? dec_bytes : 0);
    S.take(dact, 10 * n);
    S.take(dmap, remap_dev ? 0 : n);
    S.take(dst, 1);
  });
  if (rc) return rc;
  if (remap_dev) dmap = remap_dev;
  rc = gbp_tree_graft_check_dev(t, tree, n, root, radius, direction, adaptive, dchk, dact,
                                (uint32_t *)(dchk + fl_at), s);
  if (rc) return rc;
  int64_t resolved = 0;
  if (test_edges && (rc = tree_edge_decisions(t, tree, n, direction, adaptive, dedge, fl_at, &resolved, s)))
    return rc;
  std::vector<uint8_t> chk(dec_bytes);
  if ((rc = d2h(chk.data(), dchk, dec_bytes, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  uint8_t *att = chk.data();
  const uint32_t *fl = (const uint32_t *)(chk.data() + fl_at);
  int64_t candidates = 0, checked = 0, redone = 0;
  for (int64_t j = 0; j < n; j++) {
    candidates += (fl[j] & GBP_F_GRAFT_CANDIDATE) != 0;
    checked += (fl[j] & GBP_F_GRAFT_CHECKED) != 0;
    if (!(fl[j] & GBP_F_FRAGILE)) continue;
    // depth 0 of attemptConnect(r, v[j]) again with glibc (host/gbp_host_check.cpp)
    const gbp_host::Terrain *H = host_mirror(t);
    if (!H) return GBP_E_HIP;
    double sj[8], a[10], sn[8], tn = 0;
    if ((rc = d2h(sj, tree->v + 8 * j, 8, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    const double t_s = gbp_host::pose_distance(sj, root) / V_NOM;
    bool ok = false;
    if (t_s > KINEMATICS_RES) {
      gbp_host::connect_action(direction == GBP_FORWARD ? root : sj, direction == GBP_FORWARD ? sj : root,
                               t_s, a);
      if (gbp_host::is_valid_action(a)) {
        uint32_t f = 0;
        ok = gbp_host::pair_check(*H, root, a, direction, adaptive, sn, &tn, &f, nullptr);
        if ((rc = h2d(dact + 10 * j, a, 10, s))) return rc;
        HIPCHK(hipStreamSynchronize(s));  // a leaves scope only after the copy
      }
    }
    att[j] = ok ? 1 : 0;
    redone++;
  }
  if (redone) {
    if ((rc = h2d(dchk, att, n, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
  }
  rc = gbp_tree_graft_dev(tree, n, root, dchk, dact, test_edges ? dedge : nullptr, dmap, dst, s);
  if (rc) return rc;
  if (remap && (rc = d2h(remap, dmap, n, s))) return rc;
  if ((rc = d2h(stats, dst, 1, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  stats->n_candidates = candidates;
  stats->n_checked = checked;
  if (n_resolved) *n_resolved = resolved + redone;
  return GBP_OK;
}

}  // namespace

extern "C" {

// ---- pruning against a changed terrain ---------------------------
int gbp_tree_revalidate_dev(gbp_terrain *t, gbp_tree *tree, int64_t n, int direction, int adaptive,
                            uint8_t *edge_valid, uint32_t *flags, gbp_stream stream) {
  if (!t) return GBP_E_BAD_HANDLE;
  int rc = prune_args(tree, n, edge_valid && flags);
  if (rc) return rc;
  if (direction != GBP_FORWARD && direction != GBP_REVERSE) return GBP_E_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GBP_E_NO_DEVICE;
  if (!t->d_z) return GBP_E_BAD_HANDLE;
  if (t->device != tree->device) return GBP_E_INVALID_ARG;
  DeviceGuard g(tree->device);
  hipStream_t s = (hipStream_t)stream;
  double *rs = nullptr, *ra = nullptr;
  if (n > 1 && (rc = prune_rows(tree, n, rs, ra))) return rc;
  hipLaunchKernelGGL(k_prune_gather, dim3(grid_for((n - 1) * PRUNE_PIECES, TB, t->num_cus * 8)),
                     dim3(TB), 0, s, *tree, (int32_t)n, (double2 *)rs, (double2 *)ra, edge_valid, flags);
  HIPCHK(hipGetLastError());
  if (n == 1) return GBP_OK;
  // vertex i's decision is row i - 1's: straight into edge_valid[i] / flags[i]
  return gbp_validate_pairs_dev(t, n - 1, rs, ra, nullptr, direction, adaptive, edge_valid + 1, nullptr,
                                nullptr, flags + 1, nullptr, stream);
}

int gbp_tree_prune_dev(gbp_tree *tree, int64_t n, const uint8_t *edge_valid, int32_t *remap,
                       gbp_prune_stats *stats, gbp_stream stream) {
  NoDepth x;
  return tree_keep(tree, n, 0, edge_valid, remap, stats, (hipStream_t)stream, x);
}

int gbp_tree_revalidate_host(gbp_terrain *t, gbp_tree *tree, int direction, int adaptive,
                             int32_t *remap, gbp_prune_stats *stats, int64_t *n_resolved) {
  return keep_host<false>(t, tree, 0, direction, adaptive, remap, nullptr, 0, stats, n_resolved);
}

int gbp_tree_revalidate_keep_host(gbp_terrain *t, gbp_tree *tree, int direction, int adaptive,
                                  int32_t *remap, int32_t *remap_dev, int64_t remap_cap,
                                  gbp_prune_stats *stats, int64_t *n_resolved) {
  return keep_host<false>(t, tree, 0, direction, adaptive, remap, remap_dev, remap_cap, stats,
                          n_resolved);
}

// ---- re-rooting at a vertex ---------------------------------------
int gbp_tree_reroot_last(double ms[3], int64_t *launches) {
  return read_last(reroot_last, ms, launches);
}

int gbp_tree_reroot_dev(gbp_tree *tree, int64_t n, int32_t new_root, const uint8_t *edge_valid,
                        int32_t *remap, gbp_reroot_stats *stats, gbp_stream stream) {
  RerootDepth x;
  const int rc = tree_keep(tree, n, new_root, edge_valid, remap, stats, (hipStream_t)stream, x);
  if (rc) return rc;
  keep_last(reroot_last, x);
  return GBP_OK;
}

int gbp_tree_reroot_host(gbp_terrain *t, gbp_tree *tree, int32_t new_root, int direction,
                         int adaptive, int32_t *remap, gbp_reroot_stats *stats, int64_t *n_resolved) {
  return keep_host<true>(t, tree, new_root, direction, adaptive, remap, nullptr, 0, stats, n_resolved);
}

int gbp_tree_reroot_keep_host(gbp_terrain *t, gbp_tree *tree, int32_t new_root, int direction,
                              int adaptive, int32_t *remap, int32_t *remap_dev, int64_t remap_cap,
                              gbp_reroot_stats *stats, int64_t *n_resolved) {
  return keep_host<true>(t, tree, new_root, direction, adaptive, remap, remap_dev, remap_cap, stats,
                         n_resolved);
}

// ---- grafting onto a root state that is no vertex -------------------
int gbp_tree_graft_last(double ms[3], int64_t *launches) { return read_last(graft_last, ms, launches); }

int gbp_tree_graft_dev(gbp_tree *tree, int64_t n, const double *root, const uint8_t *attach,
                       const double *actions, const uint8_t *edge_valid, int32_t *remap,
                       gbp_graft_stats *stats, gbp_stream stream) {
  if (!tree_ok(tree)) return GBP_E_BAD_HANDLE;
  if (!root || !attach || !actions || has_nan8(root)) return GBP_E_INVALID_ARG;
  GraftRoot x;
  x.attach = attach;
  x.actions = actions;
  x.remap = remap;
  for (int k = 0; k < 8; k++) x.root.s[k] = root[k];
  const int rc = tree_keep(tree, n, 0, edge_valid, remap, stats, (hipStream_t)stream, x);
  if (rc) return rc;
  keep_last(graft_last, x);
  return GBP_OK;
}

int gbp_tree_graft_host(gbp_terrain *t, gbp_tree *tree, const double *root, double radius,
                        int direction, int adaptive, int test_edges, int32_t *remap,
                        gbp_graft_stats *stats, int64_t *n_resolved) {
  return graft_host(t, tree, root, radius, direction, adaptive, test_edges, remap, nullptr, 0, stats,
                    n_resolved);
}

int gbp_tree_graft_keep_host(gbp_terrain *t, gbp_tree *tree, const double *root, double radius,
                             int direction, int adaptive, int test_edges, int32_t *remap,
                             int32_t *remap_dev, int64_t remap_cap, gbp_graft_stats *stats,
                             int64_t *n_resolved) {
  return graft_host(t, tree, root, radius, direction, adaptive, test_edges, remap, remap_dev, remap_cap,
                    stats, n_resolved);
}

}  // extern "C"
