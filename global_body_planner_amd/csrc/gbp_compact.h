// gbp_compact.h — the order-preserving compactions.  Device only; not part of
// the C ABI.
//
// The look-back form, one launch (ordered_rank, at the end of this file): the
// workgroups chain their counts with a decoupled look-back.  The planner's
// appends (gbp_plan.hip) and the targets drawn inside a search (gbp_nn.hip)
// use it; RRT*'s item counts (gbp_star.hip) are published as its tile words.
//
// The two-pass form, the pieces of the compaction without a wait
// between workgroups, for workgroups of CB threads: a tile of CB
// elements counts its kept elements with wave ballots (tile_count), one
// workgroup scans the tiles' counts (tile_scan), then every tile ranks its
// elements again from its offset, from the same ballots (tile_rank).  The
// prune and the re-root of a device tree (gbp_tree_maint.hip) and the remap of
// RRT*'s kept connections (gbp_replan.hip) are built from them.
//
// A tile's record holds K 32-bit components: [0] the kept elements, which the
// scan turns into offsets, then side sums; with MAXLAST the last component is a
// maximum instead of a sum.  Its size follows K (8 B for two components, 16 B
// for four), one store and one load per tile.
#pragma once

#include "gbp_internal.h"

template <int K>
struct alignas(4 * K) TileRec {
  uint32_t c[K];
};

// Every thread of the workgroup gives its element's K predicates (K - 1 and a
// value to maximise with MAXLAST); thread 0's result is the tile's record.  A
// workgroup that calls this again puts a barrier in between.
template <int K, bool MAXLAST = false>
__device__ __forceinline__ TileRec<K> tile_count(const bool (&pred)[K - (MAXLAST ? 1 : 0)],
                                                 uint32_t val = 0u) {
  constexpr int NP = K - (MAXLAST ? 1 : 0);
  __shared__ uint32_t sw[K][CB / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  uint32_t mine[K];
#pragma unroll
  for (int c = 0; c < NP; c++) mine[c] = (uint32_t)__popcll(__ballot(pred[c]));
  if constexpr (MAXLAST) {
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) val = max(val, (uint32_t)__shfl_xor(val, s, WAVE));
    mine[K - 1] = val;
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < K; c++) sw[c][wv] = mine[c];
  }
  __syncthreads();
  TileRec<K> t{};
  if (threadIdx.x == 0) {
    for (int q = 0; q < CB / WAVE; q++) {
#pragma unroll
      for (int c = 0; c < K; c++)
        t.c[c] = MAXLAST && c == K - 1 ? max(t.c[c], sw[c][q]) : t.c[c] + sw[c][q];
    }
  }
  return t;
}

// One workgroup over the records load(b), b in [0, ntile), in passes of CB:
// toff[b] = start + the kept elements of the tiles before b.  Every thread
// gets the totals: [0] start + all kept elements, the side sums, the maximum.
template <int K, bool MAXLAST = false, class Load>
__device__ __forceinline__ TileRec<K> tile_scan(Load load, int64_t ntile, uint32_t start,
                                                uint32_t *__restrict__ toff) {
  __shared__ uint32_t sw[K][CB / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  TileRec<K> tot{};  // the same in every thread
  tot.c[0] = start;
  for (int64_t base = 0; base < ntile; base += CB) {
    const int64_t b = base + threadIdx.x;
    const TileRec<K> rec = b < ntile ? load(b) : TileRec<K>{};
    uint32_t x[K];  // [0]: inclusive scan over the wave; the others its sum / maximum
#pragma unroll
    for (int c = 0; c < K; c++) x[c] = rec.c[c];
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) {
      const uint32_t up = __shfl_up(x[0], s, WAVE);
      if (lane >= s) x[0] += up;
#pragma unroll
      for (int c = 1; c < K; c++) {
        const uint32_t o = (uint32_t)__shfl_xor(x[c], s, WAVE);
        x[c] = MAXLAST && c == K - 1 ? max(x[c], o) : x[c] + o;
      }
    }
    if (lane == WAVE - 1) sw[0][wv] = x[0];
    if (lane == 0) {
#pragma unroll
      for (int c = 1; c < K; c++) sw[c][wv] = x[c];
    }
    __syncthreads();
    uint32_t woff = 0, all = 0;
    for (int q = 0; q < CB / WAVE; q++) {
      if (q < wv) woff += sw[0][q];
      all += sw[0][q];
#pragma unroll
      for (int c = 1; c < K; c++)
        tot.c[c] = MAXLAST && c == K - 1 ? max(tot.c[c], sw[c][q]) : tot.c[c] + sw[c][q];
    }
    if (b < ntile) toff[b] = tot.c[0] + woff + x[0] - rec.c[0];
    tot.c[0] += all;
    __syncthreads();
  }
  return tot;
}

// The output index of the thread's element when `keep` is set: off (the
// tile's offset) + the kept elements before it in the tile.  Every thread of
// the workgroup calls it; a workgroup that calls this again puts a barrier in
// between.
__device__ __forceinline__ uint32_t tile_rank(bool keep, uint32_t off) {
  __shared__ uint32_t sk[CB / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) sk[wv] = (uint32_t)__popcll(m);
  __syncthreads();
  for (int q = 0; q < wv; q++) off += sk[q];
  return off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

constexpr uint32_t LOOKBACK_SPIN_LIMIT = 1u << 24;

// ---- ordered compaction across the grid ---------------------------------------
// Block b of a CB-thread grid keeps the items whose `keep` is set; returns the
// item's rank among all kept items of the grid (blocks in order, threads in
// order within a block).  Tile states are 64-bit words (epoch | flag | count),
// published and polled with agent-scope atomic RMW operations (executed at
// memory, coherent across the XCDs' L2s).  Every block of the grid must call
// this exactly once.  The grid must be resident at once (callers launch at
// most a few hundred 1024-thread blocks).  *total gets the grid's total
// (written by the last block).
__device__ __forceinline__ unsigned long long tile_word(uint32_t epoch, uint32_t flag, uint32_t v) {
  return ((unsigned long long)epoch << 32) | ((unsigned long long)flag << 30) | (v & 0x3FFFFFFFu);
}

static __device__ uint32_t ordered_rank(bool keep, unsigned long long *tiles, uint32_t epoch,
                                        int32_t *total, gbp_plan_status *st, uint32_t tile,
                                        uint32_t ntile) {
  __shared__ uint32_t wsum[CB / WAVE];
  __shared__ uint32_t s_excl;
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const unsigned long long m = __ballot(keep);
  const uint32_t wr = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[w] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t woff = 0, bsum = 0;
  for (int i = 0; i < (int)(blockDim.x / WAVE); i++) {
    if (i < w) woff += wsum[i];
    bsum += wsum[i];
  }
  if (threadIdx.x == 0) {
    const uint32_t b = tile;
    uint32_t excl = 0;
    if (b > 0) {
      __hip_atomic_exchange(&tiles[b], tile_word(epoch, 1, bsum), __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT);
      int j = (int)b - 1;
      uint32_t spins = 0;
      for (;;) {
        const unsigned long long x =
            __hip_atomic_fetch_add(&tiles[j], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t flag = (uint32_t)(x >> 30) & 3u;
        if ((uint32_t)(x >> 32) != epoch || flag == 0) {
          if (++spins > LOOKBACK_SPIN_LIMIT) {  // bounded: report, never hang
            atomicOr(&st->error, 1u);
            break;
          }
          __builtin_amdgcn_s_sleep(2);
          continue;
        }
        excl += (uint32_t)(x & 0x3FFFFFFFu);
        if (flag == 2 || j == 0) break;
        --j;
      }
    }
    __hip_atomic_exchange(&tiles[b], tile_word(epoch, 2, excl + bsum), __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
    s_excl = excl;
    if (b == ntile - 1) *total = (int32_t)(excl + bsum);
  }
  __syncthreads();
  return s_excl + woff + wr;
}
__device__ __forceinline__ uint32_t ordered_rank(bool keep, unsigned long long *tiles, uint32_t epoch,
                                                 int32_t *total, gbp_plan_status *st) {
  return ordered_rank(keep, tiles, epoch, total, st, blockIdx.x, gridDim.x);
}
