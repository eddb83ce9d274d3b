// gbp_tree_maint.hip — a device tree kept through a change: pruned against a
// changed terrain (gbp_tree_revalidate_dev, gbp_tree_prune_dev,
// gbp_tree_revalidate_host / _keep_host) or re-rooted at one of
// its vertices (gbp_tree_reroot_dev, gbp_tree_reroot_host / _keep_host,
// gbp_tree_reroot_last).  A translation unit of its own beside
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
// k_reroot_g_wide / k_reroot_g_narrow write g).
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
template <bool DEPTH>
__global__ __launch_bounds__(TB) void k_keep_seed(const int32_t *__restrict__ parent,
                                                  const uint8_t *__restrict__ edge_valid, int32_t n,
                                                  int32_t k, uint32_t *__restrict__ w,
                                                  uint32_t *__restrict__ d) {
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
    uint32_t x, e = 0;
    if (i == k) {
      x = (uint32_t)k << 1;
    } else if (i == 0) {
      x = 1u;
    } else {
      const int32_t p = parent[i];
      const bool in = p >= 0 && p < n;
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

template <bool DEPTH>
__global__ __launch_bounds__(CB) void k_keep_count(const uint32_t *__restrict__ w,
                                                   const uint32_t *__restrict__ d,
                                                   const uint8_t *__restrict__ edge_valid, int32_t n,
                                                   int32_t k, KeepTile<DEPTH> *__restrict__ tile) {
  const int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x;
  const bool in = i < n;
  const uint32_t x = in ? w[i] : 1u;
  const bool below = in && keep_below<DEPTH>(x, k);
  const bool keep = below && !(x & 1u);
  const bool bad = below && i != k && edge_valid && !edge_valid[i];
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
// order)
template <bool DEPTH>
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
  remap[i] = j;
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
// stops there whatever the arrays hold.
__device__ __forceinline__ int32_t prune_next_kept(int32_t c, const int32_t *__restrict__ link,
                                                   const int32_t *__restrict__ remap, int32_t n) {
  for (int32_t steps = 0; c >= 0 && c < n && steps < n; c = link[c], steps++)
    if (remap[c] >= 0) return remap[c];
  return -1;
}

// a kept vertex's g (copied: it is g[parent] + poseDistance already), its
// parent renumbered, its fp16 row (hm zeroed before this launch), and its
// places in the successor lists: the old lists with the pruned vertices left
// out, so each list keeps its order.  Every word written belongs to the
// vertex's own fresh row.  A new root's old parent is not kept, so its parent
// becomes -1 and it is in no list.
__global__ __launch_bounds__(TB) void k_prune_move_links(gbp_tree o, gbp_tree f, int32_t n,
                                                         const int32_t *__restrict__ remap) {
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
    const int32_t j = remap[i];
    if (j < 0) continue;
    const int32_t p = o.parent[i];
    f.parent[j] = (p >= 0 && p < n) ? remap[p] : -1;
    f.g[j] = o.g[i];
    double s[8];
    copy8(s, o.v + 8 * i);
    nn_put_hrow(f.vh, f.hm, j, s, false);
    f.child[j] = prune_next_kept(o.child[i], o.sibling, remap, n);
    f.sibling[j] = prune_next_kept(o.sibling[i], o.sibling, remap, n);
    f.prev[j] = prune_next_kept(o.prev[i], o.prev, remap, n);
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
  static constexpr bool DEPTH = false;
  uint32_t *d[2] = {nullptr, nullptr}, *depth = nullptr, *hist = nullptr;
  void carve(Stage &, int64_t) {}
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
template <class Extra>
int tree_keep(gbp_tree *tree, int64_t n, int32_t k, const uint8_t *edge_valid, int32_t *remap,
              KeepStats<Extra::DEPTH> *stats, hipStream_t s, Extra &x) {
  constexpr bool DEPTH = Extra::DEPTH;
  int rc = prune_args(tree, n, remap && stats && (DEPTH || edge_valid));
  if (rc) return rc;
  int64_t have = 0;
  if ((rc = gbp_tree_size(tree, &have, s))) return rc;  // synchronises
  if (have != n) return GBP_E_SHAPE;
  if (k < 0 || k >= n) return GBP_E_INVALID_ARG;
  DeviceGuard g(tree->device);
  const int64_t ntile = (n + CB - 1) / CB;
  DevBuf buf;
  uint32_t *w[2], *toff;
  KeepTile<DEPTH> *tile;
  rc = stage_buf(buf, [&](Stage &S) {
    S.take(w[0], n); S.take(w[1], n); S.take(tile, ntile); S.take(toff, ntile);
    x.carve(S, n);
  });
  if (rc) return rc;
  gbp_tree fresh = *tree;
  if ((rc = tree_alloc(&fresh, tree->cap))) return rc;
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
  const unsigned gv = grid_for(n, TB, 2048);
  x.mark(0, s);
  hipLaunchKernelGGL(k_keep_seed<DEPTH>, dim3(gv), dim3(TB), 0, s, tree->parent, edge_valid, (int32_t)n, k,
                     w[0], x.d[0]);
  int cur = 0;  // ceil(log2 n) rounds, back to back
  for (int64_t reach = 1; reach < n; reach <<= 1, cur ^= 1)
    hipLaunchKernelGGL(k_keep_jump<DEPTH>, dim3(gv), dim3(TB), 0, s, w[cur], x.d[cur], w[cur ^ 1],
                       x.d[cur ^ 1], (int32_t)n);
  x.mark(1, s);
  hipLaunchKernelGGL(k_keep_count<DEPTH>, dim3((unsigned)ntile), dim3(CB), 0, s, w[cur], x.d[cur],
                     edge_valid, (int32_t)n, k, tile);
  hipLaunchKernelGGL(k_keep_scan<DEPTH>, dim3(1), dim3(CB), 0, s, tile, ntile, toff, (int32_t)n, stats,
                     fresh.count);
  if (hipGetLastError() != hipSuccess || hipMemsetAsync(fresh.hm, 0, 64, s) != hipSuccess ||
      !x.before_rank(n, s))
    return drop_fresh(GBP_E_HIP);
  hipLaunchKernelGGL(k_keep_rank<DEPTH>, dim3((unsigned)ntile), dim3(CB), 0, s, w[cur], x.d[cur],
                     (int32_t)n, k, toff, remap, x.depth, x.hist);
  hipLaunchKernelGGL(k_prune_move_rows, dim3(grid_for(n * PRUNE_PIECES, TB, 2048)), dim3(TB), 0, s, *tree,
                     fresh, (int32_t)n, remap);
  hipLaunchKernelGGL(k_prune_move_links, dim3(gv), dim3(TB), 0, s, *tree, fresh, (int32_t)n, remap);
  if (hipGetLastError() != hipSuccess) return drop_fresh(GBP_E_HIP);
  if ((rc = x.after_move(fresh, n, gv, stats, s))) return drop_fresh(rc);
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

// the last successful gbp_tree_reroot_dev of the process, for gbp_tree_reroot_last
std::mutex reroot_last_mu;
double reroot_last_ms[3] = {0, 0, 0};
int64_t reroot_last_launches = 0;
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
  static constexpr bool DEPTH = true;
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
  if (!ms || !launches) return GBP_E_INVALID_ARG;
  std::lock_guard<std::mutex> lk(reroot_last_mu);
  for (int k = 0; k < 3; k++) ms[k] = reroot_last_ms[k];
  *launches = reroot_last_launches;
  return GBP_OK;
}

int gbp_tree_reroot_dev(gbp_tree *tree, int64_t n, int32_t new_root, const uint8_t *edge_valid,
                        int32_t *remap, gbp_reroot_stats *stats, gbp_stream stream) {
  RerootDepth x;
  const int rc = tree_keep(tree, n, new_root, edge_valid, remap, stats, (hipStream_t)stream, x);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(reroot_last_mu);
  for (int q = 0; q < 3; q++) {
    float t = 0.f;
    reroot_last_ms[q] =
        x.marks.ok && hipEventElapsedTime(&t, x.marks.e[q], x.marks.e[q + 1]) == hipSuccess ? t : 0.0;
  }
  reroot_last_launches = x.launches;
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

}  // extern "C"
