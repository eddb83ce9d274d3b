// gbp_star.hip — RRT*-Connect's insertion on the device
// (rrt_star_connect.cpp:12-67; gbp_plan_star_config), stages 6 and 7 of the
// half-iteration gbp_plan.hip enqueues:
//   stage 6  k_star_count       neighbourhoods in the vertex map's order, chunked
//                               (its last workgroup scans the items' offsets)
//            k_star_fill        the neighbour lists
//            k_star_check       one wave per connect check: its action and pair check
//   stage 7  k_star_replay      (own stream) the ordered choose-parent / rewire replay
// and the ranking of the kept connections after Tb's halves (k_star_rank);
// their three enqueue functions (star_enqueue_*), the workspace's RRT* block
// and its side stream.  The list of kept connections is written by stage 5's
// append (k_append, StarShared: gbp_plan.hip) and carried between searches by
// gbp_replan.hip.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gbp.h"
#include "gbp_device.h"
#include "gbp_internal.h"
#include "gbp_plan_dev.h"
#include "gbp_compact.h"
#include "gbp_um_order.h"

using namespace gbp;

namespace {

// ============================================================================
// RRT*-Connect insertion (rrt_star_connect.cpp:12-67), stages 6 and 7
// ============================================================================
// After stage 3 has appended the half's new vertices base + k (parent = their
// nearest vertex, not yet joined), every one is inserted in order as the
// reference's extend does: its neighbourhood is the vertices before it within
// delta (neighborhoodDist, planner_class.cpp:173-182, ascending index); the
// parent is the neighbour that REACHES it cheapest (choose-parent, :31-49),
// then every neighbour it REACHES more cheaply is rewired under it with the g
// of its subtree updated (:51-66, graph_class.cpp:131-138).  The connect
// decisions depend on the states alone, so stage 6 runs all of them at once:
// two per neighbour pair (choose-parent attemptConnect(s_near, s_new) and
// rewire attemptConnect(s_new, s_near), the depth-0 REACHED decision), their
// pair checks on the persistent kernel.  Stage 7 replays the insertions in
// order (one workgroup: a vertex's choices read the g values its predecessors
// left), each choice a block-wide reduction.

constexpr int RB = 1024;  // threads of the single-workgroup star kernels

__device__ __forceinline__ int block_sum_tb(int v, int *sh) {
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o);
  if (lane == 0) sh[w] = v;
  __syncthreads();
  int t = 0;
  for (int i = 0; i < (int)(blockDim.x / WAVE); i++) t += sh[i];
  __syncthreads();
  return t;
}

// The neighbourhoods are scanned in the vertex map's iteration order
// (gbp_um_order.h: new vertex k sees keys 0..base+k, position p holding key
// um_key_at(p, base+k+1)), split into chunks of `ch` positions: item
// (k, c) = positions [c·ch, (c+1)·ch) of vertex k, k-major, so concatenating the
// items' hits in item order lists each vertex's neighbours in the reference's
// order.  A half adds a few vertices to trees of tens of thousands: one
// workgroup per vertex (the round-5 form) left nearly every CU idle.
constexpr int64_t STAR_CH = 1024;  // positions per item (grown until the items fit)
#ifndef GBP_STAR_GK
#define GBP_STAR_GK 1  // k_star_count / k_star_fill workgroups per CU
#endif
// (GBP_STAR_GC, k_star_check's workgroups per CU: gbp_plan_dev.h)

__device__ __forceinline__ void star_chunking(int64_t n_added, int64_t base, int64_t cap_items,
                                              int64_t ch0, int64_t &ch, int64_t &nch) {
  const int64_t nv = base + n_added;
  ch = ch0;  // STAR_CH (GBP_STAR_CH in tests); cap_items >= the batch >= n_added: it ends
  nch = (nv + ch - 1) / ch;
  while (n_added * nch > cap_items) {
    ch *= 2;
    nch = (nv + ch - 1) / ch;
  }
}

// stage 6a: hits per item; the grid's last workgroup to finish then scans
// them (star_scan_items: the items' offsets, k-major, and each vertex's
// first pair) — one launch, not a count and a one-workgroup scan
// an item's count, published by its workgroup as tile_word(epoch, 1, hits)
// with one agent-scope exchange (no fence: the word carries its own epoch)
__device__ __forceinline__ int64_t star_item_count(gbp_plan_status *st, unsigned long long *cnt,
                                                   int64_t i, uint32_t ep) {
  uint32_t spins = 0;
  for (;;) {
    const unsigned long long x =
        __hip_atomic_fetch_add(&cnt[i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((uint32_t)(x >> 32) == ep) return (int64_t)(x & 0x3FFFFFFFu);
    if (++spins > LOOKBACK_SPIN_LIMIT) {  // bounded: report, never hang
      atomicOr(&st->error, 1u);
      return 0;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

__device__ void star_scan_items(gbp_plan_status *st, unsigned long long *cnt, uint32_t ep, int64_t N,
                                int64_t nch, int64_t n, int64_t base, int32_t *__restrict__ ioff,
                                int32_t *__restrict__ off, int64_t *__restrict__ meta,
                                int64_t max_pairs, int32_t half, uint64_t seq) {
  const int nt = (int)blockDim.x;
  const int64_t per = (N + nt - 1) / nt;
  const int64_t lo = min<int64_t>(N, threadIdx.x * per), hi = min<int64_t>(N, lo + per);
  int64_t sum = 0;
  for (int64_t i = lo; i < hi; i++) sum += star_item_count(st, cnt, i, ep);
  // block-wide exclusive scan of the threads' sums: waves, then the wave totals
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  int64_t inc = sum;
  for (int o = 1; o < WAVE; o <<= 1) {
    const int64_t u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  __shared__ int64_t wt[RB / WAVE + 1];
  if (lane == WAVE - 1) wt[w] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int i = 0; i < nt / WAVE; i++) {
      const int64_t v = wt[i];
      wt[i] = run;
      run += v;
    }
    wt[RB / WAVE] = run;
  }
  __syncthreads();
  const int64_t total = wt[RB / WAVE];
  int64_t run = wt[w] + inc - sum;
  for (int64_t i = lo; i < hi; i++) {
    const int32_t o = (int32_t)min<int64_t>(run, 0x7FFFFFFF);
    ioff[i] = o;
    if (i % nch == 0) off[i / nch] = o;  // vertex i / nch starts here
    run += star_item_count(st, cnt, i, ep);
  }
  if (threadIdx.x == 0) {
    off[n] = (int32_t)min<int64_t>(total, 0x7FFFFFFF);
    st->star_pairs = (int32_t)min<int64_t>(total, 0x7FFFFFFF);
    // the replay's own copy: it runs beside the next half, which rewrites st's
    meta[0] = n;
    meta[1] = base;
    meta[2] = min<int64_t>(total, 0x7FFFFFFF);
    st->star_rows = (int32_t)min<int64_t>(2 * total, 0x7FFFFFFF);  // rows = checks (k_star_check)
    st->star_vrows = st->star_rows;
    if (total > max_pairs) {  // the host grows the sets and resumes this half at stage 6
      atomicOr(&st->halt, (uint32_t)GBP_PLAN_HALT_STAR_PAIRS);
      st->halt_half = half;
      raise_gate(st, seq);
    } else {
      st->stat_star_connects += 2 * total;  // a choose-parent and a rewire connect per pair
    }
  }
}

__global__ __launch_bounds__(RB) void k_star_count(gbp_plan_status *st, const double *__restrict__ tv,
                                                   double delta, unsigned long long *cnt,
                                                   int32_t *__restrict__ ioff, int32_t *__restrict__ off,
                                                   int64_t *__restrict__ meta, int64_t max_pairs,
                                                   uint32_t *__restrict__ fin, int64_t cap_items,
                                                   int64_t ch0, int32_t half, uint64_t seq) {
  if (gated(st, seq)) return;
  const int64_t n = st->n_added, base = st->added_base;
  int64_t ch, nch;
  star_chunking(n, base, cap_items, ch0, ch, nch);
  // the workgroups with an item take part in the finish count (the grid is
  // sized for the largest half; most of it exits here); with no items
  // workgroup 0 alone scans (an empty list still resets the half's counts)
  const int64_t N = n * nch, parts = max<int64_t>(1, min<int64_t>(gridDim.x, N));
  const uint32_t ep = (uint32_t)seq;  // this launch's epoch (seq grows every launch)
  if ((int64_t)blockIdx.x >= parts) return;
  __shared__ int sh[RB / WAVE];
  __shared__ bool last;
  for (int64_t it = blockIdx.x; it < N; it += gridDim.x) {
    const int64_t k = it / nch, c = it - k * nch;
    const int64_t nk = base + k + 1;  // the map holds keys 0..base+k (rrt_star_connect.cpp:22)
    const int m = um_epoch(nk);
    double q[8];
    copy8(q, tv + 8 * (base + k));
    const int64_t p1 = min<int64_t>((c + 1) * ch, nk);
    int hits = 0;
    for (int64_t p = c * ch + threadIdx.x; p < p1; p += blockDim.x) {
      const int64_t j = um_key_at(p, nk, m);
      const double d = state_distance(q, tv + 8 * j);  // planner_class.cpp:178
      hits += (d <= delta && d > 0) ? 1 : 0;
    }
    hits = block_sum_tb(hits, sh);
    if (threadIdx.x == 0)
      __hip_atomic_exchange(&cnt[it], tile_word(ep, 1, (uint32_t)hits), __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 0) last = atomicAdd(fin, 1u) == (uint32_t)(parts - 1);
  __syncthreads();
  if (!last) return;
  star_scan_items(st, cnt, ep, N, nch, n, base, ioff, off, meta, max_pairs, half, seq);
  if (threadIdx.x == 0) *fin = 0;  // reset for the next half (stream-ordered)
}

// stage 6c: the neighbour lists, each item's hits in position order at its offset
__global__ __launch_bounds__(RB) void k_star_fill(gbp_plan_status *st, const double *__restrict__ tv,
                                                  double delta, const int32_t *__restrict__ ioff,
                                                  int32_t *__restrict__ nb, int32_t *__restrict__ own,
                                                  int64_t cap_items, int64_t ch0, uint64_t seq) {
  if (gated(st, seq)) return;
  const int64_t n = st->n_added, base = st->added_base;
  int64_t ch, nch;
  star_chunking(n, base, cap_items, ch0, ch, nch);
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  __shared__ int wc[RB / WAVE];
  for (int64_t it = blockIdx.x; it < n * nch; it += gridDim.x) {
    const int64_t k = it / nch, c = it - k * nch;
    const int64_t nk = base + k + 1;
    const int m = um_epoch(nk);
    double q[8];
    copy8(q, tv + 8 * (base + k));
    const int64_t p1 = min<int64_t>((c + 1) * ch, nk);
    int64_t run = ioff[it];
    for (int64_t p0 = c * ch; p0 < p1; p0 += blockDim.x) {
      const int64_t p = p0 + threadIdx.x;
      bool hit = false;
      int64_t j = 0;
      if (p < p1) {
        j = um_key_at(p, nk, m);
        const double d = state_distance(q, tv + 8 * j);
        hit = d <= delta && d > 0;
      }
      const unsigned long long bm = __ballot(hit);
      if (lane == 0) wc[w] = __popcll(bm);
      __syncthreads();
      int before = 0, total = 0;
      for (int i = 0; i < (int)(blockDim.x / WAVE); i++) {
        if (i < w) before += wc[i];
        total += wc[i];
      }
      if (hit) {
        const int64_t at = run + before + __popcll(bm & ((1ull << lane) - 1ull));
        nb[at] = (int32_t)j;
        own[at] = (int32_t)k;
      }
      run += total;
      __syncthreads();
    }
  }
}

// stage 6d's connect check c of the half's pairs (rrt_connect.cpp:20-70 at
// depth 0; pair c >> 1 = (new vertex idx, neighbour j); c even: choose-parent
// attemptConnect(s_near, s_new, poseDistance(s_new, s_near) / V_NOM), odd:
// rewire attemptConnect(s_new, s_near, ...)): whether it needs a pair check
// (the rest are not REACHED: t_s <= KINEMATICS_RES or an invalid action,
// :23-24, :66), its action a and the state sp the check starts from
__device__ __forceinline__ bool star_row(const double *__restrict__ tv, int dir, int64_t idx,
                                         int64_t j, bool rewire, double (&a)[10], double (&sp)[8]) {
  double sn[8], sj[8];
  copy8(sn, tv + 8 * idx);
  copy8(sj, tv + 8 * j);
  const double *se = rewire ? sn : sj, *sq = rewire ? sj : sn;  // (s_existing, s)
  const double t_s = (rewire ? pose_distance(sj, sn) : pose_distance(sn, sj)) / V_NOM;
  if (!(t_s > KINEMATICS_RES)) return false;
  const double *s_start = dir == GBP_FORWARD ? se : sq, *s_goal = dir == GBP_FORWARD ? sq : se;
  connect_action(s_start, s_goal, t_s, a);
  copy8(sp, dir == GBP_FORWARD ? s_start : s_goal);
  return is_valid_action(a);
}

// stage 6e: the connect checks, one wave per check c: its action
// (star_row, every lane alike) and, when it has one, its pair check
// (wave_pair_check, as k_connect: the 64 lanes evaluate 64 successive
// samples of the action, then replay them in order).  The checks are few
// (hundreds per half) and their actions long (connect actions, tens of
// samples): the persistent validate kernel's fixed cost was ~90 us for them
// (63 us per half in the planner), this one's a few steps of one wave per
// check.  Rows are the checks themselves (row c: rs / ra / rf[c], rowof[c]
// = c or -1; rf[c] = 0 for a check with no pair check); flags as
// gbp_validate's (no s_new / t_new kept).  A FRAGILE decision halts the
// sequence (the host re-decides it with glibc and resumes at stage 7).
template <class ZT, bool ADAPTIVE, int CM>
__global__ __launch_bounds__(TB) void k_star_check(TerrainView<ZT> T, gbp_plan_status *st, int dir,
                                                   const double *__restrict__ tv,
                                                   const int32_t *__restrict__ nb,
                                                   const int32_t *__restrict__ own,
                                                   int32_t *__restrict__ rowof, double *__restrict__ rs,
                                                   double *__restrict__ ra, uint32_t *__restrict__ rf,
                                                   int32_t half, uint64_t seq) {
  if (gated(st, seq)) return;
  const int64_t m = 2 * (int64_t)st->star_pairs, base = st->added_base;
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int64_t nw = (int64_t)gridDim.x * blockDim.x / WAVE;
  uint32_t rows = 0;
  for (int64_t c = wv; c < m; c += nw) {
    double a[10], sp[8];
    const int64_t pr = c >> 1;
    const bool row = star_row(tv, dir, base + own[pr], nb[pr], (c & 1) != 0, a, sp);
    uint32_t f = 0;
    if (row) {
      double sn[8], tn = 0;
      wave_pair_check<ZT, ADAPTIVE, CM>(T, sp, a, dir, sn, tn, f);
      rows++;
    }
    if (lane == 0) {
      rowof[c] = row ? (int32_t)c : -1;
      rf[c] = f;
      if (row) {
        copy8(rs + 8 * c, sp);
        copy10(ra + 10 * c, a);
      }
      if (f & GBP_F_FRAGILE) {
        atomicOr(&st->halt, (uint32_t)GBP_PLAN_HALT_STAR);
        st->halt_half = half;
        raise_gate(st, seq);
      }
    }
  }
  if (lane == 0 && rows)  // the pair checks (engine attempts) made
    atomicAdd((unsigned long long *)&st->stat_attempts, (unsigned long long)rows);
}

// block-wide (min key, min index) over the RB threads; NaN keys never win
__device__ void block_argmin(double &key, int64_t &at, double *kd, int64_t *ki) {
  kd[threadIdx.x] = key;
  ki[threadIdx.x] = at;
  __syncthreads();
  for (int o = RB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double k2 = kd[threadIdx.x + o];
      const int64_t i2 = ki[threadIdx.x + o];
      const double k1 = kd[threadIdx.x];
      const int64_t i1 = ki[threadIdx.x];
      if (i2 >= 0 && (i1 < 0 || k2 < k1 || (k2 == k1 && i2 < i1))) {
        kd[threadIdx.x] = k2;
        ki[threadIdx.x] = i2;
      }
    }
    __syncthreads();
  }
  key = kd[0];
  at = ki[0];
  __syncthreads();
}

// Stage 7 runs on ONE wave: a half inserts a few vertices (~3 at config 5),
// each with ~100 neighbours, ~2 rewires and subtree updates of ~17 vertices
// over ~1-2 levels (oracle statistics of config 5's continuation), so its
// length is a chain of dependent steps — a 1024-thread workgroup paid a
// 10-barrier reduction ladder per choice and a 16-wave barrier per subtree
// level (61 us per half); one wave reduces by shuffles and its barriers
// cost nothing.
constexpr int RW = 64;

// wave-wide lexicographic (key, position) minimum; position < 0 never wins,
// NaN keys never win (the loops only keep comparable keys)
__device__ __forceinline__ void wave_argmin(double &key, int64_t &at) {
#pragma unroll
  for (int o = RW / 2; o > 0; o >>= 1) {
    const double k2 = __shfl_xor(key, o);
    const int64_t i2 = __shfl_xor(at, o);
    if (i2 >= 0 && (at < 0 || k2 < key || (k2 == key && i2 < at))) {
      key = k2;
      at = i2;
    }
  }
}

// wave-wide least non-negative position (-1 if none)
__device__ __forceinline__ int64_t wave_first(int64_t at) {
#pragma unroll
  for (int o = RW / 2; o > 0; o >>= 1) {
    const int64_t i2 = __shfl_xor(at, o);
    if (i2 >= 0 && (at < 0 || i2 < at)) at = i2;
  }
  return at;
}

// g over the subtree below vertex r (graph_class.cpp:131-138: every successor's
// g = its parent's + poseDistance), level by level, the wave's lanes taking a
// level's vertices; the queues hold (vertex, g) in LDS up to RQ entries per
// level, in the tree's scratch past that (bounded: a list that is not a tree —
// never built here — stops at nv vertices and returns false)
constexpr int RQ = 2048;
__device__ bool subtree_g(const double *__restrict__ tv, double *tg, const int32_t *tch,
                          const int32_t *tsib, int32_t r, double gr, int32_t *q0, int32_t *q1,
                          int32_t nv, int32_t rq) {
  __shared__ int32_t lq[2][RQ];
  __shared__ double lg[2][RQ];
  __shared__ int32_t s_next;
  int32_t nq = 1, total = 1, cur = 0;
  if (threadIdx.x == 0) {
    lq[0][0] = r;
    lg[0][0] = gr;
    s_next = 0;
  }
  __syncthreads();
  while (nq > 0) {
    for (int32_t i = threadIdx.x; i < nq; i += RW) {
      const int32_t p = i < rq ? lq[cur][i] : q0[i];
      const double gp = i < rq ? lg[cur][i] : tg[p];
      double vp[8];
      copy8(vp, tv + 8 * (int64_t)p);
      for (int32_t c = tch[p]; c >= 0; c = tsib[c]) {
        const double gc = gp + pose_distance(vp, tv + 8 * (int64_t)c);
        tg[c] = gc;
        const int32_t slot = atomicAdd(&s_next, 1);
        if (slot >= nv) break;
        if (slot < rq) {
          lq[cur ^ 1][slot] = c;
          lg[cur ^ 1][slot] = gc;
        } else {
          q1[slot] = c;
        }
      }
    }
    __syncthreads();
    const int32_t next = s_next;
    __syncthreads();
    if (threadIdx.x == 0) s_next = 0;
    total += min(next, nv);
    if (next > nv || total > nv) return false;
    nq = next;
    int32_t *t = q0;
    q0 = q1;
    q1 = t;
    cur ^= 1;
    __syncthreads();
  }
  return true;
}

// addEdge(p, c)'s successor entry: c becomes p's first child
__device__ __forceinline__ void link_child(int32_t *tch, int32_t *tsib, int32_t *tprev, int32_t p,
                                           int32_t c) {
  const int32_t h = tch[p];
  tsib[c] = h;
  tprev[c] = -1;
  if (h >= 0) tprev[h] = c;
  tch[p] = c;
}

// the half's pairs, what the replay needs of them that no insertion changes:
// the neighbour, poseDistance(neighbour, s_new) (:35 and :59 alike, argument
// order included) and whether its choose-parent (bit 0) / rewire (bit 1)
// connection REACHED; the first RP in LDS (the prologue fills them), the rest
// recomputed from global memory where read
constexpr int RP = 2048;  // pairs held in LDS (config 5: ~300 per half)
constexpr int RS = 4;     // a lane's neighbour slots per insertion in registers
constexpr int RK = 512;   // new vertices held in LDS (their nearest vertex and g0's distance)

// what the replay keeps in LDS (tests shrink it: GBP_STAR_LDS = "rp,rk,rq")
struct StarLds {
  int32_t rp = RP, rk = RK, rq = RQ;
};

struct PairInfo {
  int32_t j;
  uint32_t f;
  double d;
};

__device__ __forceinline__ PairInfo pair_info_global(int64_t i, const double *__restrict__ tv,
                                                     int64_t base, const int32_t *__restrict__ nb,
                                                     const int32_t *__restrict__ own,
                                                     const int32_t *__restrict__ rowof,
                                                     const uint32_t *__restrict__ rf) {
  PairInfo pi;
  pi.j = nb[i];
  const int32_t r0 = rowof[2 * i], r1 = rowof[2 * i + 1];
  pi.f = ((r0 >= 0 && (rf[r0] & GBP_F_VALID)) ? 1u : 0u) |
         ((r1 >= 0 && (rf[r1] & GBP_F_VALID)) ? 2u : 0u);
  pi.d = pose_distance(tv + 8 * (int64_t)pi.j, tv + 8 * (base + own[i]));
  return pi;
}

// stage 7: the ordered replay of rrt_star_connect.cpp:18-66, one wave
__global__ __launch_bounds__(RW) void k_star_replay(gbp_plan_status *st, const double *__restrict__ tv,
                                                    double *ta, double *tg, int32_t *tp, int32_t *tch,
                                                    int32_t *tsib, int32_t *tprev,
                                                    const int32_t *__restrict__ off,
                                                    const int32_t *__restrict__ nb,
                                                    const int32_t *__restrict__ own,
                                                    const int32_t *__restrict__ rowof,
                                                    const double *__restrict__ ra,
                                                    const uint32_t *__restrict__ rf,
                                                    const int64_t *__restrict__ meta, int32_t *q0,
                                                    int32_t *q1, const int32_t *tcount, StarLds lim,
                                                    uint64_t seq) {
  if (gated(st, seq)) return;
  const int32_t rp = lim.rp, rk = lim.rk;  // (RP, RK; smaller in tests: the global paths)
  const int64_t n = meta[0], base = meta[1], npairs = meta[2];
  const int32_t nv = *tcount;
  const int lane = threadIdx.x;
  __shared__ int32_t lj[RP];
  __shared__ uint32_t lf[RP];
  __shared__ double ld[RP];
  __shared__ int32_t lnn[RK], loff[RK + 1];
  __shared__ double ld0[RK];
  // prologue: every pair's static part and every new vertex's nearest vertex,
  // its offsets and poseDistance(s_new, s_nearest) (:28), all lanes at once
  for (int64_t i = lane; i < min<int64_t>(npairs, rp); i += RW) {
    const PairInfo pi = pair_info_global(i, tv, base, nb, own, rowof, rf);
    lj[i] = pi.j;
    lf[i] = pi.f;
    ld[i] = pi.d;
  }
  for (int64_t k = lane; k < min<int64_t>(n, rk); k += RW) {
    const int32_t nn = tp[base + k];  // stage 3 wrote the nearest vertex here
    lnn[k] = nn;
    ld0[k] = pose_distance(tv + 8 * (base + k), tv + 8 * (int64_t)nn);
    loff[k] = off[k];
  }
  const int64_t nk_l = n < rk ? n : rk;
  if (lane == 0) loff[nk_l] = off[nk_l];
  __syncthreads();
  auto pair = [&](int64_t i) -> PairInfo {
    if (i < rp) return PairInfo{lj[i], lf[i], ld[i]};
    return pair_info_global(i, tv, base, nb, own, rowof, rf);
  };
  int64_t rewires = 0;
  for (int64_t k = 0; k < n; k++) {
    const int32_t idx = (int32_t)(base + k);
    const int32_t nn = k < rk ? lnn[k] : tp[idx];
    const double d0 = k < rk ? ld0[k] : pose_distance(tv + 8 * (int64_t)idx, tv + 8 * (int64_t)nn);
    const int64_t i0 = k < rk ? loff[k] : off[k], i1 = k + 1 <= rk ? loff[k + 1] : off[k + 1];
    // this lane's first RS neighbours (positions i0 + lane + RW s)
    int32_t sj[RS];
    uint32_t sf[RS];
    double sd[RS];
#pragma unroll
    for (int q = 0; q < RS; q++) {
      const int64_t i = i0 + lane + RW * q;
      sf[q] = 0;
      sj[q] = 0;
      sd[q] = 0;
      if (i < i1) {
        const PairInfo pi = pair(i);
        sj[q] = pi.j;
        sf[q] = pi.f;
        sd[q] = pi.d;
      }
    }
    const int64_t ix = i0 + (int64_t)RW * RS;  // positions past the slots
    // choose-parent (:27-44): from the nearest vertex, the first neighbour whose
    // REACHED connection is strictly cheaper than the best so far — the first
    // in the map's order of the cheapest, when that beats the nearest vertex's
    double key = INFINITY;
    int64_t at = -1;
    double gq[RS];
#pragma unroll
    for (int q = 0; q < RS; q++) gq[q] = (sf[q] & 1u) ? tg[sj[q]] : 0.0;
    const double g0 = tg[nn] + d0;  // :28
#pragma unroll
    for (int q = 0; q < RS; q++) {
      if (!(sf[q] & 1u)) continue;
      const double gc = gq[q] + sd[q];  // :35
      if (gc == gc && (at < 0 || gc < key)) {  // the first of this lane's minimum
        key = gc;
        at = i0 + lane + RW * q;
      }
    }
    for (int64_t i = ix + lane; i < i1; i += RW) {
      const PairInfo pi = pair(i);
      if (!(pi.f & 1u)) continue;
      const double gc = tg[pi.j] + pi.d;
      if (gc == gc && (at < 0 || gc < key)) {
        key = gc;
        at = i;
      }
    }
    wave_argmin(key, at);
    int32_t pmin = nn;
    double gn = g0;
    int64_t row = -1;
    if (at >= 0 && key < g0) {
      pmin = pair(at).j;
      gn = key;
      row = rowof[2 * at];
    }
    // addEdge(s_min, s_new) + updateGYValue + addAction (:47-49)
    if (lane == 0) {
      tp[idx] = pmin;
      link_child(tch, tsib, tprev, pmin, idx);
      tg[idx] = gn;
    }
    if (row >= 0 && lane < 10) ta[10 * (int64_t)idx + lane] = ra[10 * row + lane];
    __syncthreads();
    // rewire (:51-66): in neighbour order; a rewire's subtree update can change
    // the g a later neighbour is tested with, so each round finds the first
    // neighbour (from the cursor on) that rewires now
    for (int64_t cur = i0; cur < i1;) {
      const double gi = tg[idx];
#pragma unroll
      for (int q = 0; q < RS; q++)
        gq[q] = ((sf[q] & 2u) && sj[q] != pmin && i0 + lane + RW * q >= cur) ? tg[sj[q]] : 0.0;
      at = -1;
#pragma unroll
      for (int q = 0; q < RS; q++) {
        const int64_t i = i0 + lane + RW * q;
        if (at < 0 && (sf[q] & 2u) && sj[q] != pmin && i >= cur && gq[q] > (gi + sd[q])) at = i;
      }
      if (at < 0) {
        for (int64_t i = max(ix, cur) + ((lane - (max(ix, cur) - i0)) % RW + RW) % RW; i < i1; i += RW) {
          const PairInfo pi = pair(i);
          if (!(pi.f & 2u) || pi.j == pmin) continue;
          if (tg[pi.j] > (gi + pi.d)) {
            at = i;
            break;  // a lane's candidates ascend: its first is its least
          }
        }
      }
      at = wave_first(at);
      if (at < 0) break;
      const PairInfo pj = pair(at);
      const int32_t j = pj.j;
      const int64_t rrow = rowof[2 * at + 1];
      const double gj = gi + pj.d;  // updateGYValue (:60)
      if (lane == 0) {
        // removeEdge(parent, j) (graph_class.cpp:44-58) + addEdge(s_new, j): j
        // leaves its parent's list (never s_new's: s_new's children are the
        // vertices rewired before it) for the head of s_new's; every load first
        const int32_t op = tp[j], pv = tprev[j], nx = tsib[j], h = tch[idx];
        const int32_t oh = op >= 0 ? tch[op] : -1;
        if (op >= 0) {
          if (pv >= 0)
            tsib[pv] = nx;
          else if (oh == j)
            tch[op] = nx;
          if (nx >= 0) tprev[nx] = pv;
        }
        tsib[j] = h;
        tprev[j] = -1;
        if (h >= 0) tprev[h] = j;
        tch[idx] = j;
        tp[j] = idx;
        tg[j] = gj;
      }
      if (lane < 10) ta[10 * (int64_t)j + lane] = ra[10 * rrow + lane];
      __syncthreads();
      rewires++;
      // the rewired vertex's successors (recursion of updateGYValue)
      if (tch[j] >= 0 && !subtree_g(tv, tg, tch, tsib, j, gj, q0, q1, nv, lim.rq)) {
        if (lane == 0) {
          atomicOr(&st->error, 8u);  // a successor list that is not a tree
          raise_gate(st, seq);
        }
        return;
      }
      __syncthreads();
      cur = at + 1;
    }
  }
  if (lane == 0 && rewires) st->stat_rewires += rewires;
}

// after Tb's half (star_stream, behind both trees' replays): the cheapest
// of the meta[3] connections listed so far ranked with the current g values
// (:181-193: strictly cheaper than the best so far; ties to the first)
__global__ __launch_bounds__(RB) void k_star_rank(gbp_plan_status *st, const int32_t *__restrict__ shared,
                                                  const int64_t *__restrict__ meta,
                                                  const double *__restrict__ ga,
                                                  const double *__restrict__ gb, uint64_t seq) {
  if (gated(st, seq)) return;
  const int64_t ns = meta[3];
  __shared__ double kd[RB];
  __shared__ int64_t ki[RB];
  double key = INFINITY;
  int64_t at = -1;
  for (int64_t p = threadIdx.x; p < ns; p += RB) {
    const double c = ga[shared[2 * p]] + gb[shared[2 * p + 1]];
    if (c == c && (at < 0 || c < key)) {
      key = c;
      at = p;
    }
  }
  block_argmin(key, at, kd, ki);
  if (threadIdx.x == 0 && at >= 0 && key < st->best_cost) {
    st->best_cost = key;
    st->best_a = shared[2 * at];
    st->best_b = shared[2 * at + 1];
  }
}

}  // namespace

// ============================================================================
// the insertion's launches, enqueued by enqueue_stages (gbp_plan.hip)
// ============================================================================
template <class ZT>
int star_enqueue_checks(gbp_terrain *t, gbp_plan_ws *w, gbp_tree *T, int32_t half, int direction,
                        int adaptive, gbp_plan_ws::TimedHalf *th, hipStream_t s) {
  const TerrainView<ZT> V = view<ZT>(t);
  const int cus = t->num_cus;
  gbp_plan_status *st = w->st;
  gbp_plan_ws::StarSet &S = w->ss[half & 1];
  // RRT* insertion, stage 6: neighbourhoods, connect checks, their pair checks
  // one 1024-thread workgroup per CU at most (a half has ~100-200 items at
  // config 5; more are taken grid-stride): a grid of 8 per CU, nearly all
  // exiting at once, cost its dispatch
  unsigned gk = (unsigned)std::max<int64_t>(1, std::min<int64_t>(w->star_items, cus * GBP_STAR_GK));
  if (w->star_grid > 0) gk = std::min<unsigned>(gk, (unsigned)w->star_grid);
  hipLaunchKernelGGL(k_star_count, dim3(gk), dim3(RB), 0, s, st, T->v, w->star_delta, S.scnt,
                     S.sioff, S.soff, S.meta, w->star_max_pairs, S.sfin, w->star_items, w->star_ch,
                     half, ++w->seq);
  hipLaunchKernelGGL(k_star_fill, dim3(gk), dim3(RB), 0, s, st, T->v, w->star_delta, S.sioff,
                     S.snb, S.sown, w->star_items, w->star_ch, ++w->seq);
  if (th) HIPCHK(hipEventRecord(th->ev[6], s));
  const int64_t rmax = 2 * w->star_max_pairs;  // connect checks, one wave each
  const int cm = (t->opt_affine && t->affine) ? 2 : 0;
  unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cus * GBP_STAR_GC, (rmax + 3) / 4));
  if (w->star_grid > 0) g = std::min<unsigned>(g, (unsigned)w->star_grid);  // (tests: several checks a wave)
  const uint64_t cseq = ++w->seq;
  with_adaptive_cm(adaptive, cm, [&](auto ad, auto c) {
    hipLaunchKernelGGL((k_star_check<ZT, decltype(ad)::value, decltype(c)::value>), dim3(g), dim3(TB),
                       0, s, V, st, direction, T->v, S.snb, S.sown, S.srowof, S.srs, S.sra, S.srf,
                       half, cseq);
  });
  if (th) HIPCHK(hipEventRecord(th->ev[7], s));
  if (th) HIPCHK(hipEventRecord(th->ev[2], s));
  return GBP_OK;
}
template int star_enqueue_checks<float>(gbp_terrain *, gbp_plan_ws *, gbp_tree *, int32_t, int, int,
                                        gbp_plan_ws::TimedHalf *, hipStream_t);
template int star_enqueue_checks<double>(gbp_terrain *, gbp_plan_ws *, gbp_tree *, int32_t, int, int,
                                         gbp_plan_ws::TimedHalf *, hipStream_t);

int star_enqueue_replay(gbp_plan_ws *w, gbp_tree *T, int32_t half, int kT, gbp_plan_ws::TimedHalf *th,
                        hipStream_t s) {
  gbp_plan_status *st = w->st;
  gbp_plan_ws::StarSet &S = w->ss[half & 1];
  // stage 7, the ordered replay, on star_stream: it changes T's parents, g
  // and successor lists only, which nothing reads before half h + 1's
  // stage 5 (its appends into T wait for it: rdone[kT]); the connects of
  // this half and the next half's extends of O run beside it
  HIPCHK(hipEventRecord(w->star_e6, s));
  HIPCHK(hipStreamWaitEvent(w->star_stream, w->star_e6, 0));
  if (th) HIPCHK(hipEventRecord(th->ev[3], w->star_stream));
  StarLds lds;
  if (w->star_lds[0] >= 0) {
    lds.rp = w->star_lds[0];
    lds.rk = w->star_lds[1];
    lds.rq = w->star_lds[2];
  }
  hipLaunchKernelGGL(k_star_replay, dim3(1), dim3(RW), 0, w->star_stream, st, T->v, T->a, T->g,
                     T->parent, T->child, T->sibling, T->prev, S.soff, S.snb, S.sown, S.srowof,
                     S.sra, S.srf, S.meta, T->bfs, T->bfs + T->cap, T->count, lds, ++w->seq);
  HIPCHK(hipEventRecord(w->star_rdone[kT], w->star_stream));
  return GBP_OK;
}

int star_enqueue_rank(gbp_plan_ws *w, int32_t half, int kT, const double *ga, const double *gb,
                      hipStream_t s) {
  gbp_plan_ws::StarSet &S = w->ss[half & 1];
  // on star_stream behind this half's replay (Tb's g final) and half h - 1's
  // (Ta's); the next replay of Ta queues behind it, and half h + 1's
  // appends into Tb wait for it (rdone[kT] moves past it)
  HIPCHK(hipEventRecord(w->star_e5, s));
  HIPCHK(hipStreamWaitEvent(w->star_stream, w->star_e5, 0));
  hipLaunchKernelGGL(k_star_rank, dim3(1), dim3(RB), 0, w->star_stream, w->st, w->sshared, S.meta, ga,
                     gb, ++w->seq);
  HIPCHK(hipEventRecord(w->star_rdone[kT], w->star_stream));
  return GBP_OK;
}

// ============================================================================
// the workspace's RRT* side: its stream, its block, gbp_plan_star_config
// ============================================================================
// RRT*'s side stream and its events, all or none
void star_stream_destroy(gbp_plan_ws *w) {
  if (w->star_stream) (void)hipStreamSynchronize(w->star_stream);
  hipEvent_t *ev[] = {&w->star_e6, &w->star_e5, &w->star_rdone[0], &w->star_rdone[1], &w->star_sdone};
  for (hipEvent_t *e : ev) {
    if (*e) (void)hipEventDestroy(*e);
    *e = nullptr;
  }
  if (w->star_stream) (void)hipStreamDestroy(w->star_stream);
  w->star_stream = nullptr;
}

static int star_stream_create(gbp_plan_ws *w) {
  // the workspace's own (a device-wide stream would make one planner's joins
  // wait for another's replays), CU-masked to the last n/8 CUs, the ones
  // la_stream leaves free: a masked stream has a hardware queue of its own,
  // while a plain one shares one of the process's GPU_MAX_HW_QUEUES (4)
  // round-robin — with the caller's stream the replay then ran in line with
  // the connects it should overlap (config 5: 52 vs 66 M pair checks/s with
  // 8 queues)
  int xcc = 0;
  if (hipDeviceGetAttribute(&xcc, hipDeviceAttributeNumberOfXccs, w->device) != hipSuccess) xcc = 0;
  const int n = w->num_cus, lo = xcc >= 2 ? n - n / xcc : n;
  std::vector<uint32_t> mask((n + 31) / 32, 0u);
  for (int c = lo; c < n; c++) mask[c / 32] |= 1u << (c % 32);
  const hipError_t e = (lo > 0 && lo < n)
                           ? hipExtStreamCreateWithCUMask(&w->star_stream, (uint32_t)mask.size(),
                                                          mask.data())
                           : hipStreamCreateWithFlags(&w->star_stream, hipStreamNonBlocking);
  if (e != hipSuccess) w->star_stream = nullptr;
  if (e != hipSuccess ||
      hipEventCreateWithFlags(&w->star_e6, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&w->star_e5, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&w->star_rdone[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&w->star_rdone[1], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&w->star_sdone, hipEventDisableTiming) != hipSuccess) {
    star_stream_destroy(w);
    return GBP_E_HIP;
  }
  return GBP_OK;
}

// the RRT* block released and its limits forgotten: RRT* is off and the next
// gbp_plan_star_config allocates afresh
static void star_block_drop(gbp_plan_ws *w) {
  if (w->star_block) (void)hipFree(w->star_block);
  w->star_block = nullptr;
  w->star = 0;
  w->star_max_pairs = w->star_max_shared = 0;
}

// the RRT* block for these limits: allocated by its own list, its counters
// zeroed, the kept connections of a smaller block (keep_shared) put back, the
// side stream created with the first one.  Fails as a unit: the caller drops
// the block on any error.
static int star_block_create(gbp_plan_ws *w, int64_t max_pairs, int64_t max_shared,
                             const std::vector<int32_t> &keep_shared) {
  const int64_t b = w->bmax, r = 2 * max_pairs;
  int64_t items = std::max<int64_t>(4 * b, 1 << 15);
  // (tests: GBP_STAR_ITEMS, at least the batch, and GBP_STAR_CH small grow
  // the chunks; GBP_STAR_GRID makes every count / fill workgroup take
  // several items)
  const char *ie = getenv("GBP_STAR_ITEMS");
  if (ie && *ie) items = std::max<int64_t>(b, atoll(ie));
  const char *le = getenv("GBP_STAR_LDS");
  if (le && *le) {
    int a = RP, b2 = RK, c = RQ;
    if (sscanf(le, "%d,%d,%d", &a, &b2, &c) == 3) {
      w->star_lds[0] = std::max(0, std::min(a, RP));
      w->star_lds[1] = std::max(0, std::min(b2, RK));
      w->star_lds[2] = std::max(1, std::min(c, RQ));
    }
  }
  const char *ce = getenv("GBP_STAR_CH");
  w->star_ch = ce && *ce ? std::max<int64_t>(1, atoll(ce)) : STAR_CH;
  const char *ge = getenv("GBP_STAR_GRID");
  w->star_grid = ge && *ge ? std::max(1, atoi(ge)) : 0;
  w->star_items = items;
  // the block's arrays, in order; the list sizes the allocation (Stage)
  auto arrays = [w, b, r, items, max_pairs, max_shared](Stage &S) {
    for (auto &ss : w->ss) {
      S.take(ss.scnt, items);
      S.take(ss.sioff, items);
      S.take(ss.soff, b + 1);
      S.take(ss.snb, max_pairs);
      S.take(ss.sown, max_pairs);
      S.take(ss.srowof, r);
      S.take(ss.srs, 8 * r);
      S.take(ss.sra, 10 * r);
      S.take(ss.srf, r);
      S.take(ss.meta, 4);
      S.take(ss.sfin, 64);
    }
    // the last arrays of the block: kvtx written at a connection's index
    // < bmax (k_append), sshared at pairs < max_shared (k_append, k_star_rank),
    // element by element, so nothing pads them
    S.take(w->kvtx, b);
    S.take(w->sshared, 2 * max_shared);
  };
  const size_t bytes = stage_bytes_of(arrays);
  if (hipMalloc(&w->star_block, bytes) != hipSuccess) {
    w->star_block = nullptr;
    return GBP_E_ALLOC;
  }
  int rc = stage_carve(w->star_block, bytes, arrays);
  if (!rc && !w->star_stream) rc = star_stream_create(w);
  if (rc) return rc;
  for (auto &ss : w->ss)  // (epoch 0 is never a launch's: seq starts at 1)
    if (hipMemset(ss.sfin, 0, 4 * 64) != hipSuccess ||
        hipMemset(ss.scnt, 0, 8 * (size_t)items) != hipSuccess)
      return GBP_E_HIP;
  if (!keep_shared.empty() &&
      hipMemcpy(w->sshared, keep_shared.data(), 4 * keep_shared.size(), hipMemcpyHostToDevice) != hipSuccess)
    return GBP_E_HIP;
  w->star_max_pairs = max_pairs;
  w->star_max_shared = max_shared;
  return GBP_OK;
}

extern "C" {

int gbp_plan_star_config(gbp_plan_ws *w, int enable, double delta, int64_t max_pairs,
                         int64_t max_shared) {
  if (!w) return GBP_E_BAD_HANDLE;
  if (!enable) {
    w->star = 0;
    return GBP_OK;
  }
  if (!(delta >= 0) || max_pairs < 1 || max_pairs > (1 << 28) || max_shared < 1 ||
      max_shared > (1 << 28))
    return GBP_E_INVALID_ARG;
  DeviceGuard g(w->device);
  {
    const char *pe = getenv("GBP_STAR_PAIRS");  // (tests: a small first size, grown by the halts)
    if (pe && *pe && !w->star_block) max_pairs = std::max<int64_t>(1, std::min<int64_t>(max_pairs, atoll(pe)));
  }
  // a larger block keeps the run's list of kept connections (the ranking
  // after Tb's halves reads all of it); the per-half sets are rebuilt by the
  // half that resumes (GBP_PLAN_HALT_STAR_PAIRS)
  std::vector<int32_t> keep_shared;
  if (w->star_block && (max_pairs > w->star_max_pairs || max_shared > w->star_max_shared)) {
    (void)hipDeviceSynchronize();
    max_pairs = std::max(max_pairs, w->star_max_pairs);
    max_shared = std::max(max_shared, w->star_max_shared);
    keep_shared.resize(2 * (size_t)w->star_max_shared);
    if (hipMemcpy(keep_shared.data(), w->sshared, 8 * (size_t)w->star_max_shared,
                  hipMemcpyDeviceToHost) != hipSuccess)
      return GBP_E_HIP;
    star_block_drop(w);
  }
  if (!w->star_block) {
    const int rc = star_block_create(w, max_pairs, max_shared, keep_shared);
    if (rc) {
      star_block_drop(w);
      return rc;
    }
  }
  w->star = 1;
  w->star_delta = delta;
  return GBP_OK;
}

}  // extern "C"
