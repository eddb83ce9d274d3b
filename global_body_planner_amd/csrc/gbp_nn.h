// gbp_nn.h — what the planner loop (gbp_plan.hip) hands the nearest-neighbour
// search of gbp_nn.hip: the work a search launch carries beside its own (the
// extends' candidate actions, the next half's targets), a search's options,
// its launch, and its share of the workspace.  Not part of the C ABI.
#pragma once

#include "gbp_internal.h"

// stateDistance(q, vertex j) exactly as the reference evaluates it
// (planning_utils.cpp:116-127): the exact stage of every search, and of the
// look-ahead search's completion in k_la_commit (gbp_plan.hip)
__device__ __forceinline__ double nn_dist64(const double qq[8], const double *vj) {
  double sum = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const double d = vj[k] - qq[k];
    sum = sum + 1.0 * d * d;
  }
  return sqrt(sum);
}

// newConfig's candidate actions for the extends (rrt.cpp:25 surface normal,
// :34 the six draws of the extend stream) do not depend on the nearest vertex
// unless the draws are direction-biased, so stage 2 computes them in extra
// workgroups of the search's launch (PREP): they run beside the MFMA waves
// (VALU and transcendental work next to matrix-core work) instead of as a
// launch of their own after the search (k_extend_prep); the reduce then
// copies s_near into the candidates (k_nn_hreduce cs).
// The next half's targets, drawn ahead in the same launch (draw_blocks > 0;
// gbp_plan_halves_dev, sampling not direction-biased: an inline search draws
// the next half's, the look-ahead search of half h + 1 those of half h + 2):
// blocks [0, draw_blocks) draw them into that half's target set and rank them
// (ordered_rank over those blocks on the look-ahead tiles: their count in
// gbp_plan_la::nt; a FRAGILE draw sets gbp_plan_la::frag = half + 1, and the
// half halts at its start in k_la_commit).  They come first in the grid so
// that their latency-bound work overlaps the matrix-core waves.
struct NhDraw {
  int draw_blocks;
  int32_t half;  // the half the draws are for
  int64_t n, base;
  uint64_t stream;
  double *cand, *targets;
  uint32_t *cflag;
  _Float16 *tqh;
  unsigned long long *tiles;
  uint32_t epoch;
  int32_t *count;   // the valid draws' total (gbp_plan_la::nt of the half)
  uint32_t *frag;   // set to half + 1 on a FRAGILE draw (gbp_plan_la::frag)
  // an inline search launching the look-ahead one: the next search's tree
  // snapshot and whether the sequence still runs (gbp_plan_la::nv / go)
  const int32_t *snap_src;
  int32_t *snap_dst;
  uint32_t *go_dst;
};
template <class ZT>
struct NhPrep {
  gbp::TerrainView<ZT> T;
  uint64_t seed;
  double *ca;
  gbp_sampling cfg;
  int direction;
  int first_block;  // blocks [first_block, gridDim.x) draw the actions
  NhDraw dr;        // blocks [0, dr.draw_blocks): the next half's targets
  // the look-ahead search (nt set): the half's count is *nt (its drawn-ahead
  // total), its extend base the counter after the current half's commit
  // (commit_targets), and n_validate is left to k_la_commit
  const int32_t *nt;
};

constexpr int NH_TB = 256;             // k_nn_mfma: 4 independent waves per workgroup
                                       // (the draws ahead: NH_TB targets per block)

struct NnSide {
  const int32_t *nv;   // the searched tree's vertex count at the snapshot
  const uint32_t *go;  // 0: idle
};
// what a search asks for beyond its queries and its tree (the default: the
// matrix-core search of fp64 queries, nothing drawn beside it)
template <class ZT = float>
struct NnOpts {
  const _Float16 *qh = nullptr;      // the queries' fp16 rows (nn_put_hrow layout, same offsets
                                     // as q); null: converted in the search
  const NhPrep<ZT> *prep = nullptr;  // the extends' candidates are drawn inside the search ...
  double *cs = nullptr;              // ... and their s_near written by the reduce
  bool *prepped = nullptr;           // out: the candidates were drawn (prep was taken)
  const NnSide *side = nullptr;      // the look-ahead search's launch: its own partial slots,
                                     // never gated, the tree's snapshot count
  bool small = false;                // up to NS_MAXQ queries take the direct fp64 search
  bool small_any = false;            // ... and any count, when its partials hold a whole batch
};
// instantiated for float and double heights (gbp_nn.hip)
template <class ZT = float>
GBP_INTERNAL int nn_launch(gbp_plan_ws *w, const int32_t *nq_dev, const double *q,
                           const int32_t *q_off_dev, const gbp_tree *tr, int32_t *out, int num_cus,
                           hipStream_t s, const NnOpts<ZT> &opt = NnOpts<ZT>{});

// the search's share of a workspace of batch bmax: its sizes and its three
// env knobs (GBP_NN_ITEMS, GBP_NS_GRID, GBP_NSC_CAP); its arrays, in order, in
// the workspace's carve list; its counters zeroed once carved
GBP_INTERNAL void nn_ws_init(NnWs &n, int64_t bmax, int num_cus);
GBP_INTERNAL void nn_ws_carve(NnWs &n, Stage &S, int64_t bmax);
GBP_INTERNAL int nn_ws_zero(NnWs &n);
