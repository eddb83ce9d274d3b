// gbp_replan.hip — what a replanning caller keeps on the device between
// searches: RRT*-Connect's list of kept connections read,
// loaded and carried through a prune's or a re-root's remap
// (gbp_plan_shared_read_host / _load_host / _remap_dev), and the joined path
// of two device trees extracted without reading the trees
// (gbp_tree_path_dev / _host).  A translation unit of its own: the objects of
// gbp_engine.hip, gbp_plan.hip, gbp_tree_maint.hip and gbp_terrain.hip do not
// depend on it.  The handles, tree_ok and the block sizes WAVE / TB / CB:
// gbp_internal.h.
//
// The list is gbp_plan_ws::sshared, pairs (a, b) of a vertex of Ta and one of
// Tb in the order stage 5's append listed them; its length is the status's
// n_shared and the word the ranking reads (ss[].meta[3]).  Every entry here
// that changes the list leaves it ranked: the best is reset first (k_star_rank
// only ever lowers best_cost, and after a remap the old best may be gone or
// its g derived again), then the cheapest of the list by the trees' current g
// is taken with k_star_rank's rule (NaN skipped, strictly cheaper, ties to
// the earliest).
//
// The remap's compaction is gbp_compact.h's, over tiles of 1,024 pairs; the
// ranked pairs go into a second buffer, which is then copied over the list
// (compacting in place would let a tile overwrite pairs another tile has not
// read).  The list's length is read on the device, so the grids are sized from
// the number of CUs and walk the tiles with a stride.
#pragma clang fp contract(off)

#include <cmath>

#include "gbp_compact.h"
#include "gbp_internal.h"

namespace {

// what the new index of a listed vertex is (NULL remap: the identity)
__device__ __forceinline__ int32_t remapped(const int32_t *__restrict__ remap, int32_t i) {
  return remap ? remap[i] : i;
}

struct PairFate {
  bool keep, lost_a, lost_b, bad;
  int32_t ra, rb;
};

// pair i of the list under the two remaps; a pair lost on both sides counts
// under a; an index outside [0, n_*) reads no remap and is reported (bad)
__device__ __forceinline__ PairFate pair_fate(const int2 *__restrict__ list, int64_t i, int64_t n,
                                              const int32_t *__restrict__ remap_a, int64_t n_a,
                                              const int32_t *__restrict__ remap_b, int64_t n_b) {
  PairFate f{false, false, false, false, -1, -1};
  if (i >= n) return f;
  const int2 p = list[i];
  f.bad = p.x < 0 || p.x >= n_a || p.y < 0 || p.y >= n_b;
  if (f.bad) return f;
  f.ra = remapped(remap_a, p.x);
  f.rb = remapped(remap_b, p.y);
  f.lost_a = f.ra < 0;
  f.lost_b = !f.lost_a && f.rb < 0;
  f.keep = !f.lost_a && !f.lost_b;
  return f;
}

// the list's length as the kernels use it: the status's, never past the buffer
__device__ __forceinline__ int64_t list_len(const gbp_plan_status *st, int64_t max_shared) {
  const int64_t n = st->n_shared;
  return n < 0 ? 0 : (n > max_shared ? max_shared : n);
}

// tile t: [0] kept pairs, [1] lost with a, [2] lost with b alone, [3] an index
// outside its tree
using PairTile = TileRec<4>;

__global__ __launch_bounds__(CB) void k_shared_count(const gbp_plan_status *__restrict__ st,
                                                     int64_t max_shared,
                                                     const int2 *__restrict__ list,
                                                     const int32_t *__restrict__ remap_a, int64_t n_a,
                                                     const int32_t *__restrict__ remap_b, int64_t n_b,
                                                     PairTile *__restrict__ tile,
                                                     gbp_shared_stats *__restrict__ ctl) {
  const int64_t n = list_len(st, max_shared), ntile = (n + CB - 1) / CB;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const PairFate f = pair_fate(list, t * CB + threadIdx.x, n, remap_a, n_a, remap_b, n_b);
    const PairTile c = tile_count<4>({f.keep, f.lost_a, f.lost_b, f.bad});
    if (threadIdx.x == 0) {
      tile[t] = c;
      if (c.c[3]) atomicOr((unsigned long long *)&ctl->error, 1ull);
    }
    __syncthreads();
  }
}

// one workgroup: toff[t] = the kept pairs of the tiles before t; the record
__global__ __launch_bounds__(CB) void k_shared_scan(const gbp_plan_status *__restrict__ st,
                                                    int64_t max_shared,
                                                    const PairTile *__restrict__ tile,
                                                    uint32_t *__restrict__ toff,
                                                    gbp_shared_stats *__restrict__ ctl) {
  const int64_t n = list_len(st, max_shared), ntile = (n + CB - 1) / CB;
  const PairTile tot = tile_scan<4>([tile](int64_t t) { return tile[t]; }, ntile, 0u, toff);
  if (threadIdx.x == 0) {
    ctl->n_before = n;
    ctl->n_kept = tot.c[0];
    ctl->n_dropped_a = tot.c[1];
    ctl->n_dropped_b = tot.c[2];
  }
}

// the kept pairs, remapped, into the second buffer in list order
__global__ __launch_bounds__(CB) void k_shared_move(const gbp_plan_status *__restrict__ st,
                                                    int64_t max_shared,
                                                    const int2 *__restrict__ list,
                                                    const int32_t *__restrict__ remap_a, int64_t n_a,
                                                    const int32_t *__restrict__ remap_b, int64_t n_b,
                                                    const uint32_t *__restrict__ toff,
                                                    int2 *__restrict__ list2,
                                                    const gbp_shared_stats *__restrict__ ctl) {
  if (ctl->error) return;  // an index outside its tree: the list stays as it is
  const int64_t n = list_len(st, max_shared), ntile = (n + CB - 1) / CB;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const PairFate f = pair_fate(list, t * CB + threadIdx.x, n, remap_a, n_a, remap_b, n_b);
    const uint32_t at = tile_rank(f.keep, toff[t]);
    // at < n_kept <= n <= max_shared: inside the second buffer
    if (f.keep) list2[at] = make_int2(f.ra, f.rb);
    __syncthreads();
  }
}

// gbp_plan_shared_load_host: the staged pairs against the trees' counts, one
// pass before anything changes
__global__ __launch_bounds__(TB) void k_shared_check(const gbp_plan_status *__restrict__ st,
                                                     const int2 *__restrict__ list2, int64_t n,
                                                     const int32_t *__restrict__ count_a,
                                                     const int32_t *__restrict__ count_b,
                                                     gbp_shared_stats *__restrict__ ctl) {
  const int32_t na = *count_a, nb = *count_b;
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
    const int2 p = list2[i];
    bad = bad || p.x < 0 || p.x >= na || p.y < 0 || p.y >= nb;
  }
  if (__ballot(bad) && (threadIdx.x & (WAVE - 1)) == 0)
    atomicOr((unsigned long long *)&ctl->error, 1ull);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctl->n_before = st->n_shared;
    ctl->n_kept = n;
  }
}

// the second buffer over the list
__global__ __launch_bounds__(TB) void k_shared_commit(int2 *__restrict__ list,
                                                      const int2 *__restrict__ list2,
                                                      const gbp_shared_stats *__restrict__ ctl) {
  if (ctl->error) return;
  const int64_t n = ctl->n_kept;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB)
    list[i] = list2[i];
}

// one workgroup: the length published, the best reset and the new list ranked
// (read from the second buffer, which holds the same pairs); the record copied
// to the caller's.  A listed vertex past its tree's count is skipped like a NaN
// cost (only a remap out of step with its tree produces one).
__global__ __launch_bounds__(CB) void k_shared_finish(gbp_plan_status *__restrict__ st,
                                                      const int2 *__restrict__ list2,
                                                      int64_t *__restrict__ meta0,
                                                      int64_t *__restrict__ meta1,
                                                      const double *__restrict__ ga,
                                                      const int32_t *__restrict__ count_a,
                                                      const double *__restrict__ gb,
                                                      const int32_t *__restrict__ count_b,
                                                      const gbp_shared_stats *__restrict__ ctl,
                                                      gbp_shared_stats *__restrict__ stats) {
  if (threadIdx.x == 0 && stats) *stats = *ctl;
  if (ctl->error) return;
  __shared__ double kd[CB];
  __shared__ int64_t ki[CB];
  const int64_t n = ctl->n_kept;
  const int32_t na = *count_a, nb = *count_b;
  double key = INFINITY;
  int64_t at = -1;
  for (int64_t p = threadIdx.x; p < n; p += CB) {
    const int2 q = list2[p];
    if (q.x >= na || q.y >= nb) continue;
    const double c = ga[q.x] + gb[q.y];
    if (c == c && (at < 0 || c < key)) {
      key = c;
      at = p;
    }
  }
  kd[threadIdx.x] = key;
  ki[threadIdx.x] = at;
  __syncthreads();
  for (int o = CB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double k2 = kd[threadIdx.x + o], k1 = kd[threadIdx.x];
      const int64_t i2 = ki[threadIdx.x + o], i1 = ki[threadIdx.x];
      if (i2 >= 0 && (i1 < 0 || k2 < k1 || (k2 == k1 && i2 < i1))) {
        kd[threadIdx.x] = k2;
        ki[threadIdx.x] = i2;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    at = ki[0];
    st->n_shared = (int32_t)n;
    meta0[3] = n;
    meta1[3] = n;
    // k_star_rank's `key < best_cost` against a best of none: an INFINITY cost never becomes the best
    const bool some = at >= 0 && kd[0] < INFINITY;
    st->best_cost = some ? kd[0] : INFINITY;
    st->best_a = some ? list2[at].x : -1;
    st->best_b = some ? list2[at].y : -1;
  }
}

// ---- the joined path --------------------------------------------------------
// the parent chain i -> root of tree T into its level-queue scratch (bfs, free
// between planner calls), bounded by the tree's count; the chain's length, or
// -1 when i or a parent is outside the tree or the root is not reached
__device__ int32_t walk_chain(const gbp_tree &T, int32_t i) {
  const int32_t n = *T.count;
  if (n < 1 || n > T.cap || i < 0 || i >= n) return -1;
  int32_t len = 0, idx = i;
  for (int32_t steps = 0; steps < n; steps++) {
    T.bfs[len++] = idx;
    if (idx == 0) return len;
    idx = T.parent[idx];
    if (idx < 0 || idx >= n) return -1;
  }
  return -1;
}

__global__ __launch_bounds__(TB) void k_tree_path(gbp_tree A, int32_t ia, gbp_tree B, int32_t ib,
                                                  const gbp_plan_status *__restrict__ st,
                                                  int64_t max_states, double2 *__restrict__ states,
                                                  double2 *__restrict__ actions,
                                                  gbp_path_info *__restrict__ info) {
  __shared__ int32_t s_len[2];
  if (st && ia < 0 && ib < 0) {  // the ranked best (uniform: every lane reads the same words)
    ia = st->best_a;
    ib = st->best_b;
    if (ia < 0 || ib < 0) {
      if (threadIdx.x == 0) *info = gbp_path_info{0, 0, 0, 0, INFINITY};
      return;
    }
  }
  // one lane per chain, on two waves
  if (threadIdx.x == 0) s_len[0] = walk_chain(A, ia);
  if (threadIdx.x == WAVE) s_len[1] = walk_chain(B, ib);
  __threadfence_block();
  __syncthreads();
  const int32_t la = s_len[0], lb = s_len[1];
  if (la < 0 || lb < 0) {
    if (threadIdx.x == 0) *info = gbp_path_info{0, 0, 0, GBP_PATH_E_CHAIN, 0.0};
    return;
  }
  const int64_t n = (int64_t)la + lb - 1;
  if (threadIdx.x == 0)
    *info = gbp_path_info{(int32_t)n, la, lb - 1, n > max_states ? GBP_PATH_E_SHORT : 0,
                          A.g[ia] + B.g[ib]};
  if (n > max_states) return;
  // rows in output order, 16 B per lane: state j is Ta's chain reversed, then
  // Tb's chain without ib; action j leads into state j + 1 (Tb's edges carry
  // the child's action)
  const double2 *av = (const double2 *)A.v, *bv = (const double2 *)B.v;
  const double2 *aa = (const double2 *)A.a, *ba = (const double2 *)B.a;
  for (int64_t x = threadIdx.x; x < 4 * n; x += TB) {
    const int64_t j = x >> 2;
    const int piece = (int)(x & 3);
    states[x] = j < la ? av[4 * (int64_t)A.bfs[la - 1 - j] + piece]
                       : bv[4 * (int64_t)B.bfs[j - la + 1] + piece];
  }
  for (int64_t x = threadIdx.x; x < 5 * (n - 1); x += TB) {
    const int64_t j = x / 5;
    const int piece = (int)(x - 5 * j);
    actions[x] = j < la - 1 ? aa[5 * (int64_t)A.bfs[la - 2 - j] + piece]
                            : ba[5 * (int64_t)B.bfs[j - (la - 1)] + piece];
  }
}

// ---- host side ----------------------------------------------------------------
struct Scratch {
  int2 *list2 = nullptr;
  PairTile *tile = nullptr;
  uint32_t *toff = nullptr;
  gbp_shared_stats *ctl = nullptr;
};

// the workspace's scratch for its current max_shared (allocated, or grown
// after a gbp_plan_star_config with a larger limit, by the call that finds it
// too small: that call synchronises the device)
int scratch_of(gbp_plan_ws *w, Scratch &S) {
  const int64_t ms = w->star_max_shared, ntile = (ms + CB - 1) / CB;
  auto arrays = [&S, ms, ntile](Stage &st) {
    st.take(S.list2, ms);
    st.take(S.tile, ntile);
    st.take(S.toff, ntile);
    st.take(S.ctl, 1);
  };
  const size_t need = stage_bytes_of(arrays);
  if (w->replan_bytes < need) {
    if (w->replan) {
      HIPCHK(hipDeviceSynchronize());
      (void)hipFree(w->replan);
    }
    w->replan = nullptr;
    w->replan_bytes = 0;
    if (hipMalloc(&w->replan, need) != hipSuccess) {
      w->replan = nullptr;
      return GBP_E_ALLOC;
    }
    w->replan_bytes = need;
  }
  return stage_carve(w->replan, w->replan_bytes, arrays);
}

// behind the workspace's replay stream: the list, both trees' g and the best
// are final only after its last replay and ranking (stage 5 waits for
// star_rdone the same way).  What the next planner call puts on the replay
// stream waits for an event of the caller's stream, so it follows this entry
// when that call uses the same stream.
int behind_replay(gbp_plan_ws *w, hipStream_t s) {
  HIPCHK(hipEventRecord(w->star_sdone, w->star_stream));
  HIPCHK(hipStreamWaitEvent(s, w->star_sdone, 0));
  return GBP_OK;
}

int shared_args(const gbp_plan_ws *w, const gbp_tree *Ta, const gbp_tree *Tb) {
  if (!w || !tree_ok(Ta) || !tree_ok(Tb)) return GBP_E_BAD_HANDLE;
  if (Ta == Tb || Ta->device != w->device || Tb->device != w->device) return GBP_E_INVALID_ARG;
  if (!w->star || !w->sshared || !w->star_stream) return GBP_E_UNSUPPORTED;
  return GBP_OK;
}

void launch_finish(gbp_plan_ws *w, gbp_tree *Ta, gbp_tree *Tb, const Scratch &S,
                   gbp_shared_stats *stats, hipStream_t s) {
  const unsigned g = grid_for(w->star_max_shared, TB, 4 * w->num_cus);
  hipLaunchKernelGGL(k_shared_commit, dim3(g), dim3(TB), 0, s, (int2 *)w->sshared, S.list2, S.ctl);
  hipLaunchKernelGGL(k_shared_finish, dim3(1), dim3(CB), 0, s, w->st, S.list2, w->ss[0].meta,
                     w->ss[1].meta, Ta->g, Ta->count, Tb->g, Tb->count, S.ctl, stats);
}

}  // namespace

extern "C" {

int gbp_plan_shared_read_host(gbp_plan_ws *w, int64_t max, int32_t *pairs, int64_t *n,
                              int32_t *best_a, int32_t *best_b, double *best_cost,
                              gbp_stream stream) {
  if (!w) return GBP_E_BAD_HANDLE;
  if (max < 0 || (max > 0 && !pairs)) return GBP_E_INVALID_ARG;
  if (!w->star || !w->sshared || !w->star_stream) return GBP_E_UNSUPPORTED;
  DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)stream;
  int rc = behind_replay(w, s);
  if (rc) return rc;
  gbp_plan_status ps;
  HIPCHK(hipMemcpyAsync(&ps, w->st, sizeof ps, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const int64_t len = std::max<int64_t>(0, std::min<int64_t>(ps.n_shared, w->star_max_shared));
  const int64_t take = std::min(len, max);
  if (take > 0) {
    HIPCHK(hipMemcpyAsync(pairs, w->sshared, 8 * (size_t)take, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  if (n) *n = len;
  if (best_a) *best_a = ps.best_a;
  if (best_b) *best_b = ps.best_b;
  if (best_cost) *best_cost = ps.best_cost;
  return GBP_OK;
}

int gbp_plan_shared_load_host(gbp_plan_ws *w, gbp_tree *Ta, gbp_tree *Tb, int64_t n,
                              const int32_t *pairs, gbp_stream stream) {
  int rc = shared_args(w, Ta, Tb);
  if (rc) return rc;
  if (n < 0 || n > w->star_max_shared || (n > 0 && !pairs)) return GBP_E_INVALID_ARG;
  DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)stream;
  Scratch S;
  rc = scratch_of(w, S);
  if (!rc) rc = behind_replay(w, s);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(S.ctl, 0, sizeof *S.ctl, s));
  if (n > 0) HIPCHK(hipMemcpyAsync(S.list2, pairs, 8 * (size_t)n, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_shared_check, dim3(grid_for(n, TB, 4 * w->num_cus)), dim3(TB), 0, s, w->st,
                     S.list2, n, Ta->count, Tb->count, S.ctl);
  launch_finish(w, Ta, Tb, S, nullptr, s);
  gbp_shared_stats done;
  HIPCHK(hipMemcpyAsync(&done, S.ctl, sizeof done, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));  // (also: `pairs` may be pageable host memory)
  if (hipGetLastError() != hipSuccess) return GBP_E_HIP;
  return done.error ? GBP_E_INVALID_ARG : GBP_OK;
}

int gbp_plan_shared_remap_dev(gbp_plan_ws *w, gbp_tree *Ta, gbp_tree *Tb, const int32_t *remap_a,
                              int64_t n_a, const int32_t *remap_b, int64_t n_b,
                              gbp_shared_stats *stats, gbp_stream stream) {
  int rc = shared_args(w, Ta, Tb);
  if (rc) return rc;
  if (n_a < 0 || n_b < 0 || n_a > 0x7FFFFFFF || n_b > 0x7FFFFFFF) return GBP_E_INVALID_ARG;
  DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)stream;
  Scratch S;
  rc = scratch_of(w, S);
  if (!rc) rc = behind_replay(w, s);
  if (rc) return rc;
  const int64_t ms = w->star_max_shared;
  const unsigned gt = grid_for(ms, CB, 2 * w->num_cus);
  const int2 *list = (const int2 *)w->sshared;
  HIPCHK(hipMemsetAsync(S.ctl, 0, sizeof *S.ctl, s));
  hipLaunchKernelGGL(k_shared_count, dim3(gt), dim3(CB), 0, s, w->st, ms, list, remap_a, n_a, remap_b,
                     n_b, S.tile, S.ctl);
  hipLaunchKernelGGL(k_shared_scan, dim3(1), dim3(CB), 0, s, w->st, ms, S.tile, S.toff, S.ctl);
  hipLaunchKernelGGL(k_shared_move, dim3(gt), dim3(CB), 0, s, w->st, ms, list, remap_a, n_a, remap_b,
                     n_b, S.toff, S.list2, S.ctl);
  launch_finish(w, Ta, Tb, S, stats, s);
  return hipGetLastError() == hipSuccess ? GBP_OK : GBP_E_HIP;
}

int gbp_tree_path_dev(gbp_tree *Ta, int32_t ia, gbp_tree *Tb, int32_t ib, gbp_plan_ws *w,
                      int64_t max_states, double *states, double *actions, gbp_path_info *info,
                      gbp_stream stream) {
  if (!tree_ok(Ta) || !tree_ok(Tb)) return GBP_E_BAD_HANDLE;
  if (Ta == Tb || Ta->device != Tb->device || (w && w->device != Ta->device) || !info ||
      max_states < 0 || max_states > 0x7FFFFFFF || (max_states > 0 && !states) ||
      (max_states > 1 && !actions) || ((uintptr_t)states & 15) || ((uintptr_t)actions & 15))
    return GBP_E_INVALID_ARG;
  // the best connection is the workspace's: RRT* must be configured for it
  const bool best = ia < 0 && ib < 0;
  if (best && !w) return GBP_E_INVALID_ARG;
  if (!best && (ia < 0 || ib < 0)) return GBP_E_INVALID_ARG;
  if (best && (!w->star || !w->star_stream)) return GBP_E_UNSUPPORTED;
  DeviceGuard g(Ta->device);
  hipStream_t s = (hipStream_t)stream;
  if (w && w->star_stream) {
    const int rc = behind_replay(w, s);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_tree_path, dim3(1), dim3(TB), 0, s, *Ta, ia, *Tb, ib,
                     best ? (const gbp_plan_status *)w->st : nullptr, max_states, (double2 *)states,
                     (double2 *)actions, info);
  return hipGetLastError() == hipSuccess ? GBP_OK : GBP_E_HIP;
}

int gbp_tree_path_host(gbp_tree *Ta, int32_t ia, gbp_tree *Tb, int32_t ib, gbp_plan_ws *w,
                       int64_t max_states, double *states, double *actions, gbp_path_info *info,
                       gbp_stream stream) {
  if (!tree_ok(Ta) || !tree_ok(Tb)) return GBP_E_BAD_HANDLE;
  if (!info || max_states < 0 || (max_states > 0 && !states) || (max_states > 1 && !actions))
    return GBP_E_INVALID_ARG;
  DeviceGuard g(Ta->device);
  hipStream_t s = (hipStream_t)stream;
  DevBuf buf;
  double *ds, *da;
  gbp_path_info *di;
  int rc = stage_buf(buf, [&](Stage &S) {
    S.take(ds, 8 * std::max<int64_t>(max_states, 1));
    S.take(da, 10 * std::max<int64_t>(max_states, 1));
    S.take(di, 1);
  });
  if (!rc) rc = gbp_tree_path_dev(Ta, ia, Tb, ib, w, max_states, ds, da, di, stream);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(info, di, sizeof *info, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (info->error || info->n_states < 1) return GBP_OK;
  const size_t n = (size_t)info->n_states;
  HIPCHK(hipMemcpyAsync(states, ds, 64 * n, hipMemcpyDeviceToHost, s));
  if (n > 1) HIPCHK(hipMemcpyAsync(actions, da, 80 * (n - 1), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return GBP_OK;
}

}  // extern "C"
