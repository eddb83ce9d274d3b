// gbp_nn.hip — the nearest-neighbour search in a device tree
// (planner_class.cpp:185-200): the filter on the matrix cores and its fp64
// reduce (k_nn_mfma / k_nn_hreduce, the listed segment scans k_nn_scan /
// k_nn_scan_merge), the direct fp64 search for a few queries (k_nn_small),
// their launch (nn_launch: stages 2 and 4 of gbp_plan.hip's half-iteration and
// its look-ahead search), the search's share of the planner workspace and
// gbp_tree_nearest_dev.  The one unit built with -amdgpu-mfma-vgpr-form
// (Makefile).  The fp16 rows' layout and writer: gbp_hrow.h.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "gbp.h"
#include "gbp_device.h"
#include "gbp_internal.h"
#include "gbp_plan_dev.h"
#include "gbp_compact.h"
#include "gbp_nn.h"

using namespace gbp;

namespace {

constexpr int NN_MAX_CHUNKS = 32;  // partial slots per query at the largest batch

// (nn_dist64, the exact stage of every search below: gbp_nn.h)

// lexicographic (distance, index) minimum: the lowest index among equal
// distances; a NaN distance never wins
__device__ __forceinline__ void ns_min(double &d, int &i, double od, int oi) {
  if (od < d || (od == d && oi < i)) {
    d = od;
    i = oi;
  }
}

// ============================================================================
// nearest neighbour in a device tree on the matrix cores (planner_class.cpp:185-200)
// ============================================================================
// The filter's scores S_j = |F_j|^2 - 2 G.F_j (F_j = 64 v_j, G = 64 q: scaled
// by a power of two, so exactly; |G - F_j|^2 = |G|^2 + S_j) for a tile of 32
// vertex rows x 32 queries are two v_mfma_f32_32x32x16_f16 with fp32
// accumulation, from each coordinate split into two fp16 parts (hi + lo):
//   MFMA 1  K = [F_hi(8) | F_lo(8)] . [-2 G_hi | -2 G_hi]
//   MFMA 2  K = [F_hi(8) | N_1 N_2 N_3 0..] . [-2 G_lo | 2^14 2^14 2^14 0..]
// with N_1 + N_2 + N_3 the row's fp64 squared norm times 2^-14 in three fp16
// parts (nn_put_hrow).  The dropped G_lo.F_lo term and the parts' rounding are
// ~2^-20 of the products, so the matrix cores score 1024 (query, vertex) pairs
// per 64 MFMA cycles (the packed fp32 VALU filter of round 2 spent ~4.5
// instructions per pair and pass).  The VALU only reduces: per lane (its
// query and its 32 rows of two consecutive chunks: a "lane-unit") the minimum
// by v_min3, then the three smallest unit minima with their units and a bound
// m4 on every other unit (NhTop: v_med3 / v_cndmask, branch-free).  Work item
// = (4 query tiles = 128 queries, a segment of whole units), one wave each;
// the two lanes of a query merge their lists and the (m1..m4, units) entry goes
// to the partial slots; k_nn_hreduce then takes B = min m1 over the segments
// and re-checks in fp64 every listed unit whose minimum is <= T(B), and every
// row of a segment whose m4 is <= T(B) (a fourth unit within the threshold:
// ~4 per planner half-iteration).
// Why no minimiser is lost (everything in the scaled units; M_k = the tree's
// hmax[k] >= max_j |F_jk|; S~_j the computed score):
//   * each fp16 split has |x - hi - lo| <= 2^-20 |x| + 2^-14 (lo may be
//     subnormal or flushed), the dropped G_lo F_lo term is <= 2^-20 |G_k||F_k|,
//     the norm's three parts are within 2^-29 |F|^2 + 1, and 32 fp32
//     accumulations (rounding or truncating) add at most
//     gamma (sum |terms|), gamma = 33 * 2^-23; so |S~_j - S_j| <= eps(G)
//     (nh_eps: gamma (1.01 MM + 2.02 GM) + 2^-29 MM + 1 + 2 sum_k
//     [(4 * 2^-20 |G_k| + 1.01 * 2^-14) M_k + 1.01 * 2^-14 |G_k| + 2^-27], MM = sum M_k^2,
//     GM = sum |G_k| M_k);
//   * the fp64 minimiser j* (the reference's sqrt of an fp64 sum) has
//     |G - F_j*|^2 <= |G - F_i|^2 (1 + 5e-15) for every row i, so with i the
//     row scoring B: S~_j* <= B + 2 eps + 5e-15 (B + eps + |G|^2) <= T(B)
//     (nh_threshold: fp64, 1e-14, rounded up to fp32) — and so does every row
//     tying with j*.  Its unit has minimum <= T: it is listed (checked), or
//     three other units of that segment are listed and then m4 <= T (the
//     segment is scanned).
// Rows with |F_k| >= 2^13 (|v_k| >= 128) or NaN mark the tree (hbad): its
// searches scan in fp64.  So do queries with |G_k| >= 2^13 or NaN.
// The row's layout and its writer (NH_ROW, NH_SCALE, NH_LIM, NH_NSCALE, nh8,
// nh_split, nn_put_hrow): gbp_hrow.h.
constexpr float NH_NCONST = 16384.0f;  // the norm parts (|F|^2 * 2^-14) times 2^14 on the query side
constexpr int NS_MAXQ = 32;            // k_nn_small: queries it takes (the connects')
constexpr int NS_GQ = 4;               // ... scored together per pass
constexpr int NS_TB = 256;
constexpr int NS_BLOCKS = 1024;        // its largest grid
constexpr int NH_NT = 4;               // query tiles (32 queries) per wave
constexpr int NH_ITEMS = 4096;         // waves a search aims for
constexpr int NH_MAX_SEG = 64;         // segments per query (the reduce reads them all)
// (NH_TB, k_nn_mfma's workgroup of 4 independent waves: gbp_nn.h)
constexpr int NH_RTB = 256;            // reduce: workgroup size
constexpr int NH_G = 16;               // reduce: lanes per query

typedef float nhacc __attribute__((ext_vector_type(16)));

// items: query groups (NH_NT tiles) x segments of cps chunks (32 rows); at
// most NN_MAX_CHUNKS * bmax partial slots (pm[seg * nq + qi])
__device__ __forceinline__ void nh_geometry(int64_t nq, int64_t nv, int64_t bmax, int items,
                                            int64_t &nqg, int64_t &nseg, int64_t &cps, int64_t &nch) {
  nch = nv > 0 ? (nv + 31) / 32 : 1;
  nqg = nq > 0 ? (nq + 32 * NH_NT - 1) / (32 * NH_NT) : 1;
  int64_t want = (items + nqg - 1) / nqg;
  const int64_t slots = (NN_MAX_CHUNKS * bmax) / (nq > 0 ? nq : 1);
  if (want > slots) want = slots;
  if (want > NH_MAX_SEG) want = NH_MAX_SEG;
  if (want > nch) want = nch;
  if (want < 1) want = 1;
  cps = (nch + want - 1) / want;
  cps += cps & 1;  // whole units (pairs of chunks)
  nseg = (nch + cps - 1) / cps;
}

// eps(G) above; q: the query (G = 64 q), hm: the tree's hmax
__device__ __forceinline__ double nh_eps(const double (&q)[8], const float *__restrict__ hm) {
  double mm = 0.0, gm = 0.0, lin = 0.0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const double m = (double)hm[k] * (1.0 + 0x1p-22), ag = fabs(q[k] * NH_SCALE);
    mm += m * m;
    gm += ag * m;
    lin += (4.0 * 0x1p-20 * ag + 1.01 * 0x1p-14) * m + 1.01 * 0x1p-14 * ag + 0x1p-27;
  }
  const double gamma = 33.0 * 0x1p-23;
  return gamma * (1.01 * mm + 2.02 * gm) + 0x1p-29 * mm + 1.0 + 2.0 * lin;
}

__device__ __forceinline__ float nh_threshold(float B, double eps, double g2) {
  const double t = (double)B + 2.0 * eps + 1e-14 * (fabs((double)B) + eps + g2);
  return isnan(t) ? INFINITY : nextafterf((float)t, INFINITY);
}

// min of two (v_med3 against -inf: no canonicalising v_max as fminf brings)
__device__ __forceinline__ float nh_min2(float a, float b) {
  return __builtin_amdgcn_fmed3f(a, b, -INFINITY);
}
// min over the 16 scores of a lane: 7 v_min3 + 1 v_med3
__device__ __forceinline__ float nh_min16(const nhacc &a) {
  const float x0 = fminf(fminf(a[0], a[1]), a[2]), x1 = fminf(fminf(a[3], a[4]), a[5]);
  const float x2 = fminf(fminf(a[6], a[7]), a[8]), x3 = fminf(fminf(a[9], a[10]), a[11]);
  const float x4 = fminf(fminf(a[12], a[13]), a[14]);
  return nh_min2(fminf(fminf(x0, x1), x2), fminf(fminf(x3, x4), a[15]));
}

// a lane's three smallest unit minima (m1 <= m2 <= m3, units i1, i2, i3) and
// a lower bound m4 on every other unit's minimum; branch-free (3 v_cmp,
// 3 v_med3, 6 v_cndmask).  Planner trees are clustered: with two units a
// third within the threshold (a segment scan) came ~25 times per half-iteration.
struct NhTop {
  float m1 = INFINITY, m2 = INFINITY, m3 = INFINITY, m4 = INFINITY;
  int i1 = -1, i2 = -1, i3 = -1;
  __device__ __forceinline__ void insert(float cm, int c) {
    const bool lt1 = cm < m1, lt2 = cm < m2, lt3 = cm < m3;
    const float n4 = __builtin_amdgcn_fmed3f(m3, cm, m4), n3 = __builtin_amdgcn_fmed3f(m2, cm, m3);
    const float n2 = __builtin_amdgcn_fmed3f(m1, cm, m2), n1 = lt1 ? cm : m1;
    const int j1 = lt1 ? c : i1, j2a = lt1 ? i1 : c, j2 = lt2 ? j2a : i2;
    const int j3a = lt2 ? i2 : c, j3 = lt3 ? j3a : i3;
    m1 = n1;
    m2 = n2;
    m3 = n3;
    m4 = n4;
    i1 = j1;
    i2 = j2;
    i3 = j3;
  }
};

// pass of one wave over chunks [c0, c1) (c0 even; wave-uniform, as is nv):
// NT query tiles (B operands b1, b2).  Lane (r, h) reads row c*32 + r: part
// h (F_hi / F_lo) for MFMA 1 and part 2 + h (F_hi / norm) for MFMA 2, two
// 16-B loads with one address; the row arrays hold whole units (tree_alloc),
// rows past nv are masked.  A lane's unit u is its 32 rows of chunks 2u and
// 2u + 1 (rows 64u + 32b + 4h + (i & 3) + 8 (i >> 2), b < 2, i < 16): the
// top-2 bookkeeping runs once per unit
template <int NT>
__device__ __forceinline__ void nh_sweep(const _Float16 *__restrict__ vh, int c0, int c1, int nv,
                                         const nh8 (&b1)[NT], const nh8 (&b2)[NT], NhTop (&t)[NT]) {
  const int lane = threadIdx.x & (WAVE - 1), r = lane & 31, h = lane >> 5;
  const nh8 *base = (const nh8 *)vh + (NH_ROW / 8) * r + h;
  constexpr int64_t CS = NH_ROW * 4;  // nh8 per chunk
  // tile u's minimum over the last lane-unit: the scores of chunks c and c + 1
  // (rows past nv masked, chunk c + 1 absent when c + 1 >= c1)
  auto unit_min = [&](int u, int c, const nh8 (&a)[4]) {
    float m = INFINITY;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      if (c + k >= c1) break;
      nhacc acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[2 * k], b1[u], nhacc{}, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[2 * k + 1], b2[u], acc, 0, 0, 0);
      const int rem = nv - 32 * (c + k);
#pragma unroll
      for (int i = 0; i < 16; i++)
        if ((i & 3) + 8 * (i >> 2) + 4 * h >= rem) acc[i] = INFINITY;
      m = k ? nh_min2(m, nh_min16(acc)) : nh_min16(acc);
    }
    return m;
  };
  auto load = [&](int c, nh8 (&d)[4]) {
    d[0] = base[CS * c];
    d[1] = base[CS * c + 2];
    d[2] = base[CS * (c + 1)];
    d[3] = base[CS * (c + 1) + 2];
  };
  // full units, the next unit's rows in flight while one is scored; a
  // scheduling barrier per tile keeps one tile's accumulators live at a time
  const int uf = min(c1, nv >> 5) & ~1;  // chunks [c0, uf) form full units
  // Full units, software-pipelined over two accumulators: a chunk's scores
  // (two MFMAs) are reduced while the next chunk's MFMAs run, so the wave's
  // VALU minimum and top-3 insert overlap its own matrix work instead of
  // waiting for it (the serial form scored a tile's two chunks and then
  // reduced them).  Job order: (tile 0, chunk c), (tile 0,
  // c + 1), (tile 1, c), ... then the next unit's (tile 0, c + 2) from the
  // rows loaded a unit ahead.
  if (c0 < uf) {
    auto score = [&](const nh8 (&a)[4], int k, int u) {
      nhacc acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[2 * k], b1[u], nhacc{}, 0, 0, 0);
      return __builtin_amdgcn_mfma_f32_32x32x16_f16(a[2 * k + 1], b2[u], acc, 0, 0, 0);
    };
    // one unit's tiles; NEXT: the last tile's slots score the next unit's
    // first jobs (a branch-free body, so that the scheduling barriers hold
    // the order)
    auto unit = [&](const nh8 (&a)[4], const nh8 (&p)[4], int c, nhacc &X, nhacc &Y, auto next_tag) {
      constexpr bool NEXT = decltype(next_tag)::value;
#pragma unroll
      for (int u = 0; u < NT; u++) {
        float m = nh_min16(X);
        __builtin_amdgcn_sched_barrier(0);
        if (u + 1 < NT)
          X = score(a, 0, u + 1);
        else if (NEXT)
          X = score(p, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        m = nh_min2(m, nh_min16(Y));
        t[u].insert(m, c >> 1);
        __builtin_amdgcn_sched_barrier(0);
        if (u + 1 < NT)
          Y = score(a, 1, u + 1);
        else if (NEXT)
          Y = score(p, 1, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    nh8 a[4], p[4];
    load(c0, a);
    nhacc X = score(a, 0, 0), Y = score(a, 1, 0);
    int c = c0;
    for (; c + 2 < uf; c += 2) {
      load(c + 2, p);
      unit(a, p, c, X, Y, std::true_type{});
#pragma unroll
      for (int k = 0; k < 4; k++) a[k] = p[k];
    }
    unit(a, a, c, X, Y, std::false_type{});
  }
  if (uf < c1) {  // the last unit: a lone chunk and/or rows past the tree's end
    nh8 a[4];
    load(uf, a);  // the row arrays hold whole units
#pragma unroll
    for (int u = 0; u < NT; u++) t[u].insert(unit_min(u, uf, a), uf >> 1);
  }
}

// (what a launch carries beside the search, NhDraw and NhPrep: gbp_nn.h)

// three waves per SIMD (168 VGPRs): the pipelined sweep's two live
// accumulators would otherwise take it to 189 and two waves; the few values
// it spills around the sweep cost less (planner 5-s runs 181.4 vs 177.8 M
// extends/s, the serial sweep 179.5; profiles/r06i_nn_pipe_ab.txt)
#ifndef GBP_NN_WPE
#define GBP_NN_WPE __attribute__((amdgpu_waves_per_eu(3)))
#endif
template <int NT, class ZT, bool PREP>
__global__ __launch_bounds__(NH_TB) GBP_NN_WPE void k_nn_mfma(gbp_plan_status *__restrict__ st,
                                                   const int32_t *__restrict__ nq_dev,
                                                   const double *__restrict__ q,
                                                   const int32_t *__restrict__ q_off_dev,
                                                   const _Float16 *__restrict__ qh,
                                                   const _Float16 *__restrict__ vh,
                                                   const float *__restrict__ hm,
                                                   const int32_t *__restrict__ nv_dev, int64_t bmax,
                                                   float4 *__restrict__ pm, int4 *__restrict__ pid,
                                                   uint64_t seq, int n_items, NhPrep<ZT> pp,
                                                   const uint32_t *__restrict__ go, int small_max,
                                                   uint32_t *scan_cnt) {
  // the reduce's scan list starts empty (whatever this launch then does:
  // k_nn_scan / k_nn_scan_merge run after every search)
  if (blockIdx.x == 0 && threadIdx.x == 0) *scan_cnt = 0;
  if (PREP && pp.dr.snap_dst && blockIdx.x == 0 && threadIdx.x == 0) {
    *pp.dr.snap_dst = *pp.dr.snap_src;
    *pp.dr.go_dst = gated(st, seq) ? 0u : 1u;
  }
  if (gated(st, seq)) {
    if (PREP && !pp.nt && blockIdx.x == pp.first_block && threadIdx.x == 0) st->n_validate = 0;
    return;
  }
  if (go && *go == 0u) return;  // a look-ahead search launched after the sequence stopped
  if (!PREP && *nq_dev <= small_max) return;  // k_nn_small has them
  // the next half's targets (k_targets' work); float heights only: with fp64
  // heights the state check's registers would cost the search an occupancy step
  if constexpr (PREP && std::is_same_v<ZT, float>) if ((int)blockIdx.x < pp.dr.draw_blocks) {
    const NhDraw &d = pp.dr;
    const int64_t i = blockIdx.x * (int64_t)NH_TB + threadIdx.x;
    // s_from / s_to are unused: draws ahead are never direction-biased (the
    // host refuses draw_blocks > 0 with state_flag set); zeroed all the same
    double q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t f = 0;
    if (i < d.n) {
      sample_state_cfg_try(pp.T, pp.cfg, q, q, pp.seed, d.stream, d.base + i, 0, q);  // not biased
      Acc acc{0, 0, 0};
      const bool v = is_valid_state(pp.T, q, GBP_STANCE, acc);  // rrt_connect.cpp:254
      f = acc.flags | (v ? GBP_F_VALID : 0u);
      copy8(d.cand + 8 * i, q);
      d.cflag[i] = f;
    }
    const bool keep = f & GBP_F_VALID;
    if (__ballot(f & GBP_F_FRAGILE) && (threadIdx.x & (WAVE - 1)) == 0) *d.frag = (uint32_t)d.half + 1;
    const uint32_t r = ordered_rank(keep, d.tiles, d.epoch, d.count, st, blockIdx.x,
                                    (uint32_t)d.draw_blocks);
    if (keep) {
      copy8(d.targets + 8 * (size_t)r, q);
      nn_put_hrow(d.tqh, nullptr, r, q, false);
    }
    return;
  }
  if (PREP && (int)blockIdx.x >= pp.first_block) {  // the extends' candidate actions
    const int64_t n = pp.nt ? *pp.nt : st->n_targets, m = n * GBP_NUM_GEN_STATES;
    const int64_t base = pp.nt ? st->ext_counter : st->ext_base;
    if (!pp.nt && blockIdx.x == pp.first_block && threadIdx.x == 0) st->n_validate = (int32_t)m;
    for (int64_t c = (blockIdx.x - pp.first_block) * (int64_t)NH_TB + threadIdx.x; c < m;
         c += (int64_t)(gridDim.x - pp.first_block) * NH_TB) {
      const int64_t i = c / GBP_NUM_GEN_STATES;
      const int j = (int)(c - i * GBP_NUM_GEN_STATES);
      double nrm[3], a[10];
      surface_normal(pp.T, q[8 * i], q[8 * i + 1], nrm);  // rrt.cpp:25
      sample_action_cfg(nrm, pp.cfg, pp.direction, q + 8 * i, q + 8 * i /* unused: not biased */,
                        pp.seed, GBP_EXTEND_STREAM, (base + i) * 8 + j, a);  // rrt.cpp:34, :49
      copy10(pp.ca + 10 * c, a);
    }
    return;
  }
  const int64_t nq = *nq_dev, nv = *nv_dev, q_off = q_off_dev ? *q_off_dev : 0;
  int64_t nqg, nseg, cps, nch;
  nh_geometry(nq, nv, bmax, n_items, nqg, nseg, cps, nch);
  const bool tree_bad = ((const uint32_t *)hm)[8] != 0u || nv <= 0;
  const int lane = threadIdx.x & (WAVE - 1), r = lane & 31, h = lane >> 5;
  const int mb = PREP ? pp.dr.draw_blocks : 0;  // the search's first workgroup
  const int waves = ((PREP ? pp.first_block : (int)gridDim.x) - mb) * (NH_TB / WAVE);
  const int items = (int)(nqg * nseg);
  for (int item = __builtin_amdgcn_readfirstlane(((int)blockIdx.x - mb) * (NH_TB / WAVE) + threadIdx.x / WAVE);
       item < items; item += waves) {
    // segment-major: a workgroup's waves score the same vertex rows against
    // consecutive query groups (their loads meet in the CU's L1): 215 vs 223 us
    // at 40k vertices, 43,690 queries (profiles/r05j_nn_ab*.txt)
    const int sg = item / (int)nqg, qg = item - sg * (int)nqg;
    const int c0 = sg * (int)cps, c1 = min((int)nch, c0 + (int)cps);
    nh8 b1[NT], b2[NT];
    NhTop t[NT];
    const nh8 ncst = {(_Float16)NH_NCONST, (_Float16)NH_NCONST, (_Float16)NH_NCONST, 0, 0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < NT; u++) {
      const int64_t qi = qg * (32 * NT) + 32 * u + r;
      const bool live = qi < nq;
      if (qh) {  // the queries' fp16 rows (nn_put_hrow layout: F_hi, F_lo)
        const nh8 *qr = (const nh8 *)(qh + (int64_t)NH_ROW * (q_off + (live ? qi : 0)));
        const nh8 zh = {}, hi = live ? qr[0] : zh, lo = live ? qr[1] : zh;
        b1[u] = hi * (_Float16)(-2.0f);
        b2[u] = h ? ncst : lo * (_Float16)(-2.0f);
      } else {
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const double x = live ? q[8 * (q_off + qi) + k] * NH_SCALE : 0.0;
          _Float16 hi, lo;
          nh_split(fabs(x) < NH_LIM ? x : 0.0, hi, lo);  // a bad query is scanned in fp64
          b1[u][k] = (_Float16)(-2.0f) * hi;
          b2[u][k] = h ? ncst[k] : (_Float16)(-2.0f) * lo;
        }
      }
    }
    if (!tree_bad) nh_sweep<NT>(vh, c0, c1, (int)nv, b1, b2, t);
    // the two lanes of a query (rows 4h + ...): merge to one entry, the three
    // smallest lane-units (id = 2 unit + h) and a lower bound on the rest:
    // the other lane's three inserted into this lane's list
    if (tree_bad) {
#pragma unroll
      for (int u = 0; u < NT; u++) {
        const int64_t qi = (int64_t)qg * (32 * NT) + 32 * u + r;
        if (h == 0 && qi < nq) {
          pm[(int64_t)sg * nq + qi] = float4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
          pid[(int64_t)sg * nq + qi] = int4{-1, -1, -1, -1};
        }
      }
      continue;
    }
#pragma unroll
    for (int u = 0; u < NT; u++) {
      NhTop e = t[u];
      e.i1 = e.i1 >= 0 ? 2 * e.i1 + h : -1;
      e.i2 = e.i2 >= 0 ? 2 * e.i2 + h : -1;
      e.i3 = e.i3 >= 0 ? 2 * e.i3 + h : -1;
      const float o1 = __shfl_xor(e.m1, 32), o2 = __shfl_xor(e.m2, 32), o3 = __shfl_xor(e.m3, 32);
      const float o4 = __shfl_xor(e.m4, 32);
      const int p1 = __shfl_xor(e.i1, 32), p2 = __shfl_xor(e.i2, 32), p3 = __shfl_xor(e.i3, 32);
      e.insert(o1, p1);
      e.insert(o2, p2);
      e.insert(o3, p3);
      e.m4 = fminf(e.m4, o4);
      const int64_t qi = (int64_t)qg * (32 * NT) + 32 * u + r;
      if (h == 0 && qi < nq) {
        pm[(int64_t)sg * nq + qi] = float4{e.m1, e.m2, e.m3, e.m4};
        pid[(int64_t)sg * nq + qi] = int4{e.i1, e.i2, e.i3, 0};
      }
    }
  }
}

constexpr int NSC_TB = 256;  // k_nn_scan's workgroup
constexpr int NSC_P = 8;     // ... workgroups per listed scan
constexpr int NSM_TB = 256;   // k_nn_scan_merge

// 16 lanes per query: B, T(B), the fp64 re-checks, lexicographic (distance,
// index) minimum; nothing < inf (a NaN query): index 0.  (Writing the six
// extend candidates from here instead of k_extend_prep was measured slower:
// the sampler's registers halved the reduce's occupancy, 16 + 15.9 -> 63 us.)
__global__ __launch_bounds__(NH_RTB) void k_nn_hreduce(gbp_plan_status *st,
                                                       const int32_t *__restrict__ nq_dev,
                                                       const double *__restrict__ q,
                                                       const int32_t *__restrict__ q_off_dev,
                                                       const double *__restrict__ v,
                                                       const float *__restrict__ hm,
                                                       const int32_t *__restrict__ nv_dev,
                                                       int64_t bmax, const float4 *__restrict__ pm,
                                                       const int4 *__restrict__ pid,
                                                       int32_t *__restrict__ out, uint64_t seq,
                                                       int stats, double *__restrict__ cs, int n_items,
                                                       const uint32_t *__restrict__ go, int small_max,
                                                       NsBuf sb) {
  if (gated(st, seq)) return;
  if (go && *go == 0u) return;  // (k_nn_mfma)
  if (*nq_dev <= small_max) return;  // (k_nn_mfma)
  const int64_t nq = *nq_dev, nv = *nv_dev, q_off = q_off_dev ? *q_off_dev : 0;
  int64_t nqg, nseg, cps, nch;
  nh_geometry(nq, nv, bmax, n_items, nqg, nseg, cps, nch);
  const bool tree_bad = ((const uint32_t *)hm)[8] != 0u || nv <= 0;
  const int sl = threadIdx.x & (NH_G - 1);
  const int64_t groups = (int64_t)gridDim.x * (NH_RTB / NH_G);
  const int64_t iters = (nq + groups - 1) / groups;  // whole groups iterate together
  for (int64_t it = 0; it < iters; it++) {
    const int64_t qi = it * groups + blockIdx.x * (int64_t)(NH_RTB / NH_G) + threadIdx.x / NH_G;
    const bool live = qi < nq;
    double qq[8], g2 = 0.0;
    bool qbad = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      qq[k] = live ? q[8 * (q_off + qi) + k] : 0.0;
      const double gk = qq[k] * NH_SCALE;
      qbad = qbad || !(fabs(gk) < NH_LIM);
      g2 += gk * gk;
    }
    // the group's entries, lane sl reading segments sl, sl + NH_G, ...
    constexpr int NK = NH_MAX_SEG / NH_G;
    float B = INFINITY, w4[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) {
      const int64_t s = sl + NH_G * k;
      const float4 e = live && s < nseg ? pm[s * nq + qi] : float4{INFINITY, INFINITY, INFINITY, INFINITY};
      B = fminf(B, e.x);
      w4[k] = e.w;
    }
#pragma unroll
    for (int off = NH_G / 2; off > 0; off >>= 1) B = fminf(B, __shfl_xor(B, off, NH_G));
    const float T = nh_threshold(B, nh_eps(qq, hm), g2);
    double best = INFINITY;
    int bi = 0x7FFFFFFF, nrc = 0, nsc = 0;
    bool full = live && (qbad || tree_bad || !(B < INFINITY));
    const int gbit = (threadIdx.x & (WAVE - 1)) & ~(NH_G - 1);
    constexpr uint32_t GM = NH_G == 32 ? 0xFFFFFFFFu : (1u << NH_G) - 1u;
    // segments with a fourth unit within T are scanned in full by k_nn_scan:
    // the query's entries listed contiguously (its group's leader reserves
    // them); a full list turns the query into a whole-tree fp64 scan here
    int qn = 0, qbase = 0;  // (group-uniform)
    {
      uint32_t bal[NK], tot = 0;
#pragma unroll
      for (int k = 0; k < NK; k++) {
        bal[k] = (uint32_t)(__ballot(live && !full && sl + NH_G * k < nseg && w4[k] <= T) >> gbit) & GM;
        tot += __popc(bal[k]);
      }
      nsc += sl == 0 ? (int)tot : 0;
      if (tot) {
        uint32_t base = 0;
        if (sl == 0) base = atomicAdd(sb.cnt, tot);
        base = (uint32_t)__shfl((int)base, gbit);
        const bool fits = base + tot <= sb.cap;
        uint32_t off = base;
#pragma unroll
        for (int k = 0; k < NK; k++) {
          if ((bal[k] >> sl) & 1u) {
            const uint32_t slot = off + __popc(bal[k] & ((1u << sl) - 1u));
            if (slot < sb.cap)  // (past a full list: reserved, unused)
              sb.list[slot] = fits ? int2{(int)qi, (int)(sl + NH_G * k)} : int2{-1, 0};
          }
          off += __popc(bal[k]);
        }
        if (fits) {
          qn = (int)tot;
          qbase = (int)base;
        } else {
          full = live;
        }
      }
    }
    if (full) {  // the whole tree in fp64
      for (int64_t j = sl; j < nv; j += NH_G) {
        const double d = nn_dist64(qq, v + 8 * j);
        if (d < best) {  // ascending per lane: the first index at its minimum
          best = d;
          bi = (int)j;
        }
      }
    }
    // the half-chunks to re-check go round the group: a half-chunk's 16 rows
    // one per lane
    const bool part = live && !full;
    for (int64_t s0 = 0; s0 < nseg; s0 += NH_G) {
      const int64_t s = s0 + sl;
      bool chk1 = false, chk2 = false, chk3 = false;
      int4 hid = {-1, -1, -1, 0};
      if (part && s < nseg) {
        const float4 e = pm[s * nq + qi];  // L2-warm since the first pass
        if (!(e.w <= T) && e.x <= T) {  // (a segment in full: listed above)
          hid = pid[s * nq + qi];
          chk1 = hid.x >= 0;
          chk2 = e.y <= T && hid.y >= 0;
          chk3 = e.z <= T && hid.z >= 0;
        }
      }
      uint32_t cmask = (uint32_t)(__ballot(chk1) >> gbit) & GM;
      uint32_t cmask2 = (uint32_t)(__ballot(chk2) >> gbit) & GM;
      uint32_t cmask3 = (uint32_t)(__ballot(chk3) >> gbit) & GM;
      nrc += sl == 0 ? __popc(cmask) + __popc(cmask2) + __popc(cmask3) : 0;
      while (__ballot((cmask | cmask2 | cmask3) != 0u)) {
        if (cmask | cmask2 | cmask3) {
          int h;
          if (cmask) {
            const int src = __ffs(cmask) - 1;
            cmask &= cmask - 1u;
            h = __shfl(hid.x, src, NH_G);
          } else if (cmask2) {
            const int src = __ffs(cmask2) - 1;
            cmask2 &= cmask2 - 1u;
            h = __shfl(hid.y, src, NH_G);
          } else {
            const int src = __ffs(cmask3) - 1;
            cmask3 &= cmask3 - 1u;
            h = __shfl(hid.z, src, NH_G);
          }
          // the lane-unit's 32 rows, 32 / NH_G per lane
#pragma unroll
          for (int r = 0; r < 32 / NH_G; r++) {
            const int x = sl + NH_G * r, b = x >> 4, i = x & 15;
            const int64_t j =
                (int64_t)(h >> 1) * 64 + 32 * b + 4 * (h & 1) + (i & 3) + 8 * (i >> 2);
            if (j < nv) {
              const double d = nn_dist64(qq, v + 8 * j);
              if (d < best || (d == best && j < bi)) {
                best = d;
                bi = (int)j;
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int off = NH_G / 2; off > 0; off >>= 1) {
      const double od = __shfl_xor(best, off, NH_G);
      const int oi = __shfl_xor(bi, off, NH_G);
      if (od < best || (od == best && oi < bi)) {
        best = od;
        bi = oi;
      }
    }
    if (live && sl == 0) out[qi] = bi == 0x7FFFFFFF ? 0 : bi;
    if (cs && live && sl < GBP_NUM_GEN_STATES)  // s_near of the six candidates (k_extend_prep)
      copy8(cs + 8 * (qi * GBP_NUM_GEN_STATES + sl), v + 8 * (int64_t)(bi == 0x7FFFFFFF ? 0 : bi));
    // a query with listed scans: its answer so far, for k_nn_scan_merge
    if (qn && sl == 0) {
      sb.hd[qi] = best;
      sb.hi[qi] = bi;
      sb.qh[qi] = int2{qbase, qn};
    }
    if (!stats) continue;  // diagnostics (GBP_OPT_NN_STATS): same-address atomics serialise
    for (int off = 32; off > 0; off >>= 1) {
      nrc += __shfl_xor(nrc, off);
      nsc += __shfl_xor(nsc, off);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0 && (nrc | nsc)) {
      atomicAdd((unsigned long long *)&st->stat_nn_rechecks, (unsigned long long)nrc);
      atomicAdd((unsigned long long *)&st->stat_nn_scans, (unsigned long long)nsc);
    }
  }
}

// the listed segment scans (a ~3k-row segment walked by one wave was the
// reduce's tail: 80 -> 31 us at 40k vertices without it), each over NSC_P
// workgroups: unit u = (scan u / NSC_P, part u % NSC_P) writes its rows'
// lexicographic (distance, index) minimum.  k_nn_scan_merge then folds, per
// query, its scans' units into the reduce's answer and rewrites out / the
// candidates' s_near where it changed.  Never gated: k_nn_mfma empties the
// list first thing, whatever the sequence does.
__global__ __launch_bounds__(NSC_TB) void k_nn_scan(const int32_t *__restrict__ nq_dev,
                                                    const double *__restrict__ q,
                                                    const int32_t *__restrict__ q_off_dev,
                                                    const double *__restrict__ v,
                                                    const int32_t *__restrict__ nv_dev, int64_t bmax,
                                                    int n_items, NsBuf sb) {
  const uint32_t n = min(*sb.cnt, sb.cap);
  if (n == 0) return;
  const int64_t nq = *nq_dev, nv = *nv_dev, q_off = q_off_dev ? *q_off_dev : 0;
  int64_t nqg, nseg, cps, nch;
  nh_geometry(nq, nv, bmax, n_items, nqg, nseg, cps, nch);
  __shared__ double sd[NSC_TB / WAVE];
  __shared__ int si[NSC_TB / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const uint32_t units = n * NSC_P;
  for (uint32_t e = blockIdx.x; e < units; e += gridDim.x) {
    const int2 L = sb.list[e / NSC_P];
    if (L.x < 0) continue;  // (workgroup-uniform)
    double qq[8];
#pragma unroll
    for (int k = 0; k < 8; k++) qq[k] = q[8 * (q_off + L.x) + k];
    const int64_t j0 = L.y * cps * 32, j1 = min(nv, min(nch, (L.y + 1) * cps) * 32);
    const int64_t len = (j1 - j0 + NSC_P - 1) / NSC_P, p0 = j0 + (e % NSC_P) * len;
    const int64_t p1 = min(j1, p0 + len);
    double d = INFINITY;
    int i = 0x7FFFFFFF;
    for (int64_t j = p0 + threadIdx.x; j < p1; j += NSC_TB) ns_min(d, i, nn_dist64(qq, v + 8 * j), (int)j);
    for (int off = WAVE / 2; off > 0; off >>= 1) ns_min(d, i, __shfl_xor(d, off), __shfl_xor(i, off));
    if (lane == 0) {
      sd[w] = d;
      si[w] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < NSC_TB / WAVE; k++) ns_min(d, i, sd[k], si[k]);
      sb.ed[e] = d;
      sb.ei[e] = i;
    }
    __syncthreads();
  }
}

// per listed query (its first entry): its units folded into the reduce's
// answer (hd / hi); out and the candidates' s_near rewritten where it changed
// (the list is emptied by the next search's k_nn_mfma)
__global__ __launch_bounds__(NSM_TB) void k_nn_scan_merge(NsBuf sb, const double *__restrict__ v,
                                                          int32_t *__restrict__ out,
                                                          double *__restrict__ cs) {
  const uint32_t n = min(*sb.cnt, sb.cap);
  for (uint32_t e = blockIdx.x * NSM_TB + threadIdx.x; e < n; e += gridDim.x * NSM_TB) {
    const int qx = sb.list[e].x;
    if (qx < 0) continue;
    const int2 h = sb.qh[qx];
    if (h.x != (int)e) continue;  // not the query's first entry
    double d = sb.hd[qx];
    int i = sb.hi[qx];
    const int i0 = i;
    for (int f = h.x; f < h.x + h.y; f++)
#pragma unroll
      for (int k = 0; k < NSC_P; k++) ns_min(d, i, sb.ed[f * NSC_P + k], sb.ei[f * NSC_P + k]);
    if (i == i0) continue;
    const int o = i == 0x7FFFFFFF ? 0 : i;
    out[qx] = o;
    if (cs)
      for (int k = 0; k < GBP_NUM_GEN_STATES; k++)
        copy8(cs + 8 * ((int64_t)qx * GBP_NUM_GEN_STATES + k), v + 8 * (int64_t)o);
  }
}

// A few queries (the connect stage's: the vertices one half added, ~1-10 at
// the planner's batch) against a tree of tens of thousands of vertices: the
// matrix-core search would give each query a few long-running waves and its
// reduce a latency chain (~25 + 18 us per half at 40k vertices); here every
// thread scores its vertices in fp64 for up to NS_GQ queries at a time
// (nn_dist64: the exact stage itself, nothing to re-check), workgroups reduce
// (distance, index) lexicographically (the lowest index among ties,
// planner_class.cpp:185-200; NaN never wins, so a NaN query gets index 0 as
// in k_nn_hreduce) and the last workgroup to finish reduces the partials.
// k_nn_mfma / k_nn_hreduce return at once when nq <= NS_MAXQ (small_max).
__global__ __launch_bounds__(NS_TB) void k_nn_small(gbp_plan_status *st, const int32_t *__restrict__ nq_dev,
                                                     const double *__restrict__ q,
                                                     const int32_t *__restrict__ q_off_dev,
                                                     const double *__restrict__ v,
                                                     const int32_t *__restrict__ nv_dev,
                                                     int32_t *__restrict__ out, double *__restrict__ pd,
                                                     int32_t *__restrict__ pi, uint32_t *fin, int64_t capq,
                                                     uint64_t seq) {
  if (gated(st, seq)) return;
  const int64_t nq = *nq_dev, nv = *nv_dev, q_off = q_off_dev ? *q_off_dev : 0;
  if (nq <= 0 || nq > capq) return;
  __shared__ double sd[NS_TB / WAVE][NS_GQ];
  __shared__ int si[NS_TB / WAVE][NS_GQ];
  __shared__ bool last;
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  for (int64_t k0 = 0; k0 < nq; k0 += NS_GQ) {
    double qq[NS_GQ][8], bd[NS_GQ];
    int bi[NS_GQ];
#pragma unroll
    for (int g = 0; g < NS_GQ; g++) {
      const int64_t k = min(k0 + g, nq - 1);
#pragma unroll
      for (int c = 0; c < 8; c++) qq[g][c] = q[8 * (q_off + k) + c];
      bd[g] = INFINITY;
      bi[g] = 0x7FFFFFFF;
    }
    for (int64_t j = blockIdx.x * (int64_t)NS_TB + threadIdx.x; j < nv; j += (int64_t)gridDim.x * NS_TB) {
#pragma unroll
      for (int g = 0; g < NS_GQ; g++) ns_min(bd[g], bi[g], nn_dist64(qq[g], v + 8 * j), (int)j);
    }
#pragma unroll
    for (int g = 0; g < NS_GQ; g++) {
      for (int off = WAVE / 2; off > 0; off >>= 1)
        ns_min(bd[g], bi[g], __shfl_xor(bd[g], off), __shfl_xor(bi[g], off));
      if (lane == 0) {
        sd[w][g] = bd[g];
        si[w][g] = bi[g];
      }
    }
    __syncthreads();
    if (threadIdx.x < NS_GQ && k0 + threadIdx.x < nq) {
      double d = sd[0][threadIdx.x];
      int i = si[0][threadIdx.x];
      for (int ww = 1; ww < NS_TB / WAVE; ww++) ns_min(d, i, sd[ww][threadIdx.x], si[ww][threadIdx.x]);
      pd[(k0 + threadIdx.x) * gridDim.x + blockIdx.x] = d;
      pi[(k0 + threadIdx.x) * gridDim.x + blockIdx.x] = i;
      __threadfence();  // (before this workgroup counts itself finished)
    }
    __syncthreads();
  }
  // the last workgroup to finish reduces every query's partials
  if (threadIdx.x == 0) {
    __threadfence();
    last = atomicAdd(fin, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  for (int64_t k = w; k < nq; k += NS_TB / WAVE) {
    double d = INFINITY;
    int i = 0x7FFFFFFF;
    for (int b = lane; b < (int)gridDim.x; b += WAVE)
      ns_min(d, i, __hip_atomic_load(&pd[k * gridDim.x + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
             __hip_atomic_load(&pi[k * gridDim.x + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    for (int off = WAVE / 2; off > 0; off >>= 1) ns_min(d, i, __shfl_xor(d, off), __shfl_xor(i, off));
    if (lane == 0) out[k] = i == 0x7FFFFFFF ? 0 : i;
  }
  if (threadIdx.x == 0) *fin = 0;  // reset for the next launch (stream-ordered)
}

// gbp_tree_nearest_dev: its queries' count where the searches read it
__global__ void k_set_queries(gbp_plan_status *st, int32_t n) {
  st->halt = 0;
  st->done = 0;
  st->gate_seq = ~0ull;
  st->n_targets = n;
}

}  // namespace

template <class ZT>
int nn_launch(gbp_plan_ws *w, const int32_t *nq_dev, const double *q, const int32_t *q_off_dev,
              const gbp_tree *tr, int32_t *out, int num_cus, hipStream_t s, const NnOpts<ZT> &opt) {
  NnWs &n = w->nnw;
  const _Float16 *qh = opt.qh;
  const NhPrep<ZT> *prep = opt.prep;
  double *cs = opt.cs;
  bool *prepped = opt.prepped;
  const NnSide *side = opt.side;
  const bool small = opt.small, small_any = opt.small_any;
  if (prepped) *prepped = false;
  // small: up to NS_MAXQ queries take the direct fp64 search (k_nn_small),
  // the matrix-core pair then returns at once (the count is on the device)
  const int small_max = small && !prep ? NS_MAXQ : 0;
  // ... and when k_nn_small's partials hold a whole batch of queries (the
  // workspace's max_batch, which bounds the count), it takes every count and
  // the other four launches are not made at all: in the steady state of the
  // planner and of config 5 they returned at once but cost ~21 us of the
  // caller's stream per half (the connects' queries are the half's new
  // vertices, a few; a large count is slower this way, never wrong)
  const bool direct_only = small_any && small_max && !side && n.ns_capq >= w->bmax;
  if (small_max)
    // one workgroup per CU of an XCD: in the planner the look-ahead search
    // holds the other seven (32 blocks 171.8 M extends/s, 64: 171.2, 128:
    // 169.3, 512: 160.8, the matrix-core pair alone 169.2; r05k_small_ab*.txt)
    hipLaunchKernelGGL(k_nn_small, dim3(n.ns_grid), dim3(NS_TB), 0, s, w->st, nq_dev, q, q_off_dev,
                       tr->v, side ? side->nv : tr->count, out, n.ns_d, n.ns_i, n.ns_fin,
                       direct_only ? n.ns_capq : (int64_t)NS_MAXQ, side ? 0 : ++w->seq);
  if (direct_only) return hipGetLastError() == hipSuccess ? GBP_OK : GBP_E_HIP;
  const int items = n.items;
  const int gm = items / (NH_TB / WAVE);  // the search's workgroups: one wave per item
  float4 *pm = (float4 *)(side ? n.d2 : n.d);
  int4 *pid = (int4 *)(side ? n.i2 : n.i);
  const int32_t *nv = side ? side->nv : tr->count;
  const uint32_t *go = side ? side->go : nullptr;
  if (prep) {
    NhPrep<ZT> pp = *prep;
    const int gd = pp.dr.draw_blocks;
    pp.first_block = gd + gm;
    const int gp = (int)grid_for(GBP_NUM_GEN_STATES * w->bmax, NH_TB, num_cus * 4);
    hipLaunchKernelGGL((k_nn_mfma<NH_NT, ZT, true>), dim3(gd + gm + gp), dim3(NH_TB), 0, s, w->st,
                       nq_dev, q, q_off_dev, qh, tr->vh, tr->hm, nv, w->bmax, pm, pid,
                       side ? 0 : ++w->seq, items, pp, go, 0, n.nsb[side ? 1 : 0].cnt);
    if (prepped) *prepped = true;
  } else {
    hipLaunchKernelGGL((k_nn_mfma<NH_NT, float, false>), dim3(gm), dim3(NH_TB), 0, s, w->st,
                       nq_dev, q, q_off_dev, qh, tr->vh, tr->hm, nv, w->bmax, pm, pid,
                       side ? 0 : ++w->seq, items, NhPrep<float>{}, go, small_max, n.nsb[side ? 1 : 0].cnt);
  }
  hipLaunchKernelGGL(k_nn_hreduce, dim3(grid_for(NH_G * w->bmax, NH_RTB, num_cus * 8)),
                     dim3(NH_RTB), 0, s, w->st, nq_dev, q, q_off_dev, tr->v, tr->hm, nv, w->bmax,
                     (const float4 *)pm, (const int4 *)pid, out, side ? 0 : ++w->seq, n.stats,
                     prep ? cs : nullptr, items, go, small_max, n.nsb[side ? 1 : 0]);
  hipLaunchKernelGGL(k_nn_scan, dim3(num_cus * 4), dim3(NSC_TB), 0, s, nq_dev, q, q_off_dev, tr->v, nv,
                     w->bmax, items, n.nsb[side ? 1 : 0]);
  hipLaunchKernelGGL(k_nn_scan_merge, dim3(16), dim3(NSM_TB), 0, s, n.nsb[side ? 1 : 0], tr->v, out,
                     prep ? cs : nullptr);
  return hipGetLastError() == hipSuccess ? GBP_OK : GBP_E_HIP;
}
template int nn_launch<float>(gbp_plan_ws *, const int32_t *, const double *, const int32_t *,
                              const gbp_tree *, int32_t *, int, hipStream_t, const NnOpts<float> &);
template int nn_launch<double>(gbp_plan_ws *, const int32_t *, const double *, const int32_t *,
                               const gbp_tree *, int32_t *, int, hipStream_t, const NnOpts<double> &);

void nn_ws_init(NnWs &n, int64_t bmax, int num_cus) {
  // 4096 items: 3072 (the waves resident at 162 VGPRs), 2048 and 6144 measured
  // slower in the planner (profiles/r04l_nn_items.txt)
  n.items = NH_ITEMS;
  {
    const char *e = getenv("GBP_NN_ITEMS");  // (A/B sweeps; whole workgroups of NH_TB / WAVE waves)
    if (e && *e) n.items = std::max(NH_TB / WAVE, std::min(1 << 16, atoi(e))) & ~(NH_TB / WAVE - 1);
  }
  // k_nn_small's partials: NS_MAXQ queries per workgroup, or a whole batch
  // when that stays within 2^22 slots (~48 MB; bench's planner: 92,749 x 32)
  n.ns_grid = std::max(1, std::min(NS_BLOCKS, num_cus / 8));
  {
    const char *e = getenv("GBP_NS_GRID");  // (A/B sweeps)
    if (e && *e) n.ns_grid = std::max(1, std::min(1024, atoi(e)));
  }
  n.ns_capq = (int64_t)n.ns_grid * bmax <= ((int64_t)1 << 22) ? std::max<int64_t>(bmax, NS_MAXQ) : NS_MAXQ;
  for (auto &sb : n.nsb) {
    const char *cenv = getenv("GBP_NSC_CAP");  // (a small list: the fallback's test)
    sb.cap = (uint32_t)std::max(1, std::min(NSC_CAP, cenv && *cenv ? atoi(cenv) : NSC_CAP));
  }
}

void nn_ws_carve(NnWs &n, Stage &S, int64_t bmax) {
  const int64_t b = bmax;
  S.take(n.d, 2 * NN_MAX_CHUNKS * b);   // k_nn_mfma: float4 per slot
  S.take(n.i, 4 * NN_MAX_CHUNKS * b);   // k_nn_mfma: int4 per slot
  S.take(n.d2, 2 * NN_MAX_CHUNKS * b);
  S.take(n.i2, 4 * NN_MAX_CHUNKS * b);
  S.take(n.ns_d, n.ns_grid * n.ns_capq);
  S.take(n.ns_i, n.ns_grid * n.ns_capq);
  S.take(n.ns_fin, 64);
  for (auto &sb : n.nsb) {
    S.take(sb.list, NSC_CAP);
    S.take(sb.ed, NSC_UNITS);
    S.take(sb.ei, NSC_UNITS);
    S.take(sb.cnt, 64);
    // the last arrays of the block: each read and written at a query's
    // index < bmax only (k_nn_hreduce, k_nn_scan_merge), so nothing pads them
    S.take(sb.hd, b);
    S.take(sb.hi, b);
    S.take(sb.qh, b);
  }
}

int nn_ws_zero(NnWs &n) {
  return hipMemset(n.ns_fin, 0, 4 * 64) == hipSuccess &&
                 hipMemset(n.nsb[0].cnt, 0, 4 * 64) == hipSuccess &&
                 hipMemset(n.nsb[1].cnt, 0, 4 * 64) == hipSuccess
             ? GBP_OK
             : GBP_E_HIP;
}

extern "C" {

int gbp_tree_nearest_dev(gbp_plan_ws *w, gbp_tree *T, int64_t n, const double *queries,
                         int32_t *index, gbp_stream stream) {
  if (!w || !tree_ok(T)) return GBP_E_BAD_HANDLE;
  if (n < 0 || n > w->bmax || (n > 0 && (!queries || !index))) return GBP_E_INVALID_ARG;
  if (n == 0) return GBP_OK;
  DeviceGuard g(w->device);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_set_queries, dim3(1), dim3(1), 0, s, w->st, (int32_t)n);
  // fp64 queries (rows converted in the search), the direct search for a few
  NnOpts<float> opt;
  opt.small = true;
  return nn_launch<float>(w, &w->st->n_targets, queries, nullptr, T, index, w->num_cus, s, opt);
}

}  // extern "C"
