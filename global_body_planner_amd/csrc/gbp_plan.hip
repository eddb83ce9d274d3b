// gbp_plan.hip — the batch-synchronous RRT-Connect half-iteration on device
// trees as one stream-ordered kernel sequence (SURVEY §8(f) row 1, §8(b) items
// 4-5), and its workspace.
//
// One half-iteration of RRTConnectClass::runRRTConnect at batch B
// (rrt_connect.cpp:246-312, the batched form of csrc/host/gbp_planner.cpp
// RRTConnectClass::extendBatch + connectBatch), tree T extended toward B
// random targets, every new vertex connected to the other tree O:
//
//   stage 0-1 k_targets         B draws of PlannerClass::randomState
//                               (planner_class.cpp:38-76) + isValidState(STANCE),
//                               the valid ones compacted in draw order (and their
//                               fp16 rows) in the same launch; a FRAGILE draw
//                               halts the sequence here (resumed at stage 1:
//                               k_compact_targets alone)
//   stage 2  k_nn_mfma/k_nn_hreduce    getNearestNeighbor in T on the matrix cores
//                               (planner_class.cpp:185-200); extra workgroups of the
//                               same launch draw newConfig's 6 candidate actions
//                               (rrt.cpp:25-50; k_extend_prep when they are
//                               direction-biased), the reduce copies s_near
//            k_validate_persistent (gbp_engine.hip)  the candidates' pair checks
//            k_select           newConfig's first valid candidate + acceptance (rrt.cpp:52-68)
//   stage 3  k_append          non-TRAPPED successors appended to T in target order
//                               (rrt.cpp:86-92; graph_class.cpp:28-42)
//   stage 4  k_nn_mfma/k_nn_hreduce    the new vertices' nearest vertex in O
//            k_connect          RRTConnectClass::attemptConnect (rrt_connect.cpp:20-91),
//                               one wave per connection, the wave's 64 lanes
//                               evaluating the pair check's samples together
//   stage 5  k_append          non-TRAPPED connections appended to O in order;
//                               the first REACHED one ends the search
//
// RRT*-Connect (gbp_plan_star_config) inserts T's new vertices between
// stages 3 and 4 (rrt_star_connect.cpp:18-66):
//   stage 6  k_star_count       neighbourhoods in the vertex map's order, chunked
//                               (its last workgroup scans the items' offsets)
//            k_star_fill        the neighbour lists
//            k_star_check       one wave per connect check: its action and pair check
//   stage 7  k_star_replay      (own stream) the ordered choose-parent / rewire replay
// and stage 5's append also lists every REACHED connection (the ranking,
// k_star_rank, follows Tb's halves on the replay's stream).
//
// Every count (targets, candidates, appended vertices) stays on the device:
// the host enqueues many half-iterations and reads one small status record
// per group.  The appends are ordered compactions: a wave ballot + popcount
// ranks a workgroup's kept items, the workgroups chain their counts with a
// decoupled look-back (Merrill & Garland, "Single-pass parallel prefix scan
// with decoupled look-back", 2016; ordered_rank, gbp_compact.h), so vertices
// land in exactly the order of the host planner's insertion loop.
//
// The other units of the planner: the searches of stages 2 and 4
// (k_nn_*, nn_launch): gbp_nn.hip; stages 6 and 7 and the ranking, their
// launches (star_enqueue_*) and the RRT* block: gbp_star.hip; the tree handle
// (gbp_tree_*): gbp_tree.hip; the connect table of found paths: gbp_shortcut.hip;
// the gate and the pair check by a whole wave they share: gbp_plan_dev.h.
// A tree pruned against a changed terrain or re-rooted at one of its vertices:
// gbp_tree_maint.hip.  The fp16 rows' writer both share with the searches:
// gbp_hrow.h; a tree's allocations: gbp_internal.h.
//
// FRAGILE decisions (gbp.h) stop the sequence at the next gate: the kernel
// that meets one sets status.halt; every later kernel of the group returns at
// once; the host re-decides the flagged items with glibc
// (gbp_plan_resolve_host), patches the stage's outputs, and resumes.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "gbp.h"
#include "gbp_device.h"
#include "gbp_internal.h"
#include "gbp_lane.h"
#include "gbp_plan_dev.h"
#include "gbp_compact.h"
#include "gbp_nn.h"

using namespace gbp;
static_assert(sizeof(gbp_plan_status) == 216, "engine.PlanStatus mirrors this layout");

// ============================================================================
// handles
// ============================================================================
// gbp_tree, NsBuf, NnWs, gbp_plan_la and gbp_plan_ws, a tree's allocations and
// the block sizes WAVE / TB / CB: gbp_internal.h (every planner unit shares them)

namespace {

// ============================================================================
// stages 0-1: targets and their ordered compaction
// ============================================================================
// the extend stream of a half: RRTClass::extend_counter_ advances by the
// number of extends (csrc/host/gbp_planner.cpp extendBatch); the re-run of a
// compaction that halted on a FRAGILE draw (the host resumes the half at
// stage 1, gbp_plan_resolve_host) starts from the same counters.  Called by
// the compaction's last workgroup once the grid's total is known.
__device__ __forceinline__ void commit_targets(gbp_plan_status *st, int32_t half, bool resumed) {
  const int64_t base = resumed ? st->ext_prev : st->ext_counter;
  const int64_t tg = resumed ? st->stat_targets_prev : st->stat_targets;
  st->ext_half = half;
  st->ext_prev = base;
  st->stat_targets_prev = tg;
  st->ext_base = base;
  st->ext_counter = base + st->n_targets;
  st->stat_targets = tg + st->n_targets;
}

// stages 0-1 of a fresh half in one launch: thread i draws target i of T's
// randomState stream (planner_class.cpp:38-76) and checks isValidState(STANCE)
// (rrt_connect.cpp:254), then the workgroups rank the valid draws in draw order
// (ordered_rank: ballot + popcount, decoupled look-back) and write them with
// their fp16 query rows.  A FRAGILE draw halts the sequence here; the host
// re-decides it with glibc and resumes the half at stage 1, the compaction
// alone (k_compact_targets on the patched flags).
template <class ZT>
__global__ __launch_bounds__(TB) void k_targets(TerrainView<ZT> T, gbp_plan_status *st, int64_t n,
                                                uint64_t seed, uint64_t stream_id, int64_t base,
                                                double *__restrict__ cand,
                                                uint32_t *__restrict__ cflag,
                                                double *__restrict__ targets,
                                                _Float16 *__restrict__ tqh,
                                                unsigned long long *tiles, uint32_t epoch,
                                                int32_t half, uint64_t seq, gbp_sampling cfg,
                                                const double *__restrict__ tv,
                                                const int32_t *__restrict__ tcount,
                                                const double *__restrict__ ov, int direction) {
  if (gated(st, seq)) return;
  // direction-biased draws (rrt_connect.cpp:248-252, :283-287): s_from / s_to
  // are T's last vertex and O's root (FORWARD half, T = Ta), or O's root and
  // T's last vertex (REVERSE half, T = Tb), as the trees stand when the half
  // starts (the batch-synchronous snapshot; batch 1 is the reference's loop)
  const double *t_last = tv + 8 * (int64_t)(*tcount - 1);
  const double *s_from = direction == GBP_FORWARD ? t_last : ov;
  const double *s_to = direction == GBP_FORWARD ? ov : t_last;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  double q[8];
  uint32_t f = 0;
  if (i < n) {
    sample_state_cfg_try(T, cfg, s_from, s_to, seed, stream_id, base + i, 0, q);  // randomState
    Acc acc{0, 0, 0};
    const bool v = is_valid_state(T, q, GBP_STANCE, acc);   // rrt_connect.cpp:254
    f = acc.flags | (v ? GBP_F_VALID : 0u);
    copy8(cand + 8 * i, q);
    cflag[i] = f;
  }
  const bool keep = f & GBP_F_VALID;
  if (__ballot(f & GBP_F_FRAGILE) && (threadIdx.x & (WAVE - 1)) == 0) {  // the targets stage halts
    atomicOr(&st->halt, (uint32_t)GBP_PLAN_HALT_TARGETS);
    st->halt_half = half;
    raise_gate(st, seq);
  }
  const uint32_t r = ordered_rank(keep, tiles, epoch, &st->n_targets, st);
  if (keep) {
    copy8(targets + 8 * (size_t)r, q);
    nn_put_hrow(tqh, nullptr, r, q, false);  // the search's query rows
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) commit_targets(st, half, false);
}

// k_targets with the handle's ellipse active (gbp.h gbp_informed): the same
// stages, the draws through sample_state_informed_cfg_try.  A kernel of its
// own, so that k_targets' code stays what it was for every search that does
// not use the ellipse (one inlined body for both cost k_targets 34 VGPRs and a
// wave per SIMD): a change to either kernel's stages belongs in both.
template <class ZT>
__global__ __launch_bounds__(TB) void k_targets_informed(
    TerrainView<ZT> T, gbp_plan_status *st, int64_t n, uint64_t seed, uint64_t stream_id,
    int64_t base, double *__restrict__ cand, uint32_t *__restrict__ cflag,
    double *__restrict__ targets, _Float16 *__restrict__ tqh, unsigned long long *tiles,
    uint32_t epoch, int32_t half, uint64_t seq, gbp_sampling cfg, gbp_informed inf,
    const double *__restrict__ tv, const int32_t *__restrict__ tcount,
    const double *__restrict__ ov, int direction) {
  if (gated(st, seq)) return;
  // direction-biased draws (rrt_connect.cpp:248-252, :283-287): s_from / s_to
  // are T's last vertex and O's root (FORWARD half, T = Ta), or O's root and
  // T's last vertex (REVERSE half, T = Tb), as the trees stand when the half
  // starts (the batch-synchronous snapshot; batch 1 is the reference's loop)
  const double *t_last = tv + 8 * (int64_t)(*tcount - 1);
  const double *s_from = direction == GBP_FORWARD ? t_last : ov;
  const double *s_to = direction == GBP_FORWARD ? ov : t_last;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  double q[8];
  uint32_t f = 0;
  if (i < n) {
    // randomState with x, y inside the ellipse where the direction coin does not land
    sample_state_informed_cfg_try(T, cfg, inf, s_from, s_to, seed, stream_id, base + i, 0, q);
    Acc acc{0, 0, 0};
    const bool v = is_valid_state(T, q, GBP_STANCE, acc);   // rrt_connect.cpp:254
    f = acc.flags | (v ? GBP_F_VALID : 0u);
    copy8(cand + 8 * i, q);
    cflag[i] = f;
  }
  const bool keep = f & GBP_F_VALID;
  if (__ballot(f & GBP_F_FRAGILE) && (threadIdx.x & (WAVE - 1)) == 0) {  // the targets stage halts
    atomicOr(&st->halt, (uint32_t)GBP_PLAN_HALT_TARGETS);
    st->halt_half = half;
    raise_gate(st, seq);
  }
  const uint32_t r = ordered_rank(keep, tiles, epoch, &st->n_targets, st);
  if (keep) {
    copy8(targets + 8 * (size_t)r, q);
    nn_put_hrow(tqh, nullptr, r, q, false);  // the search's query rows
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) commit_targets(st, half, false);
}

// stage 1 alone (a half resumed after a FRAGILE draw, on the host-patched
// flags): the compacted targets in draw order and their fp16 query rows
__global__ __launch_bounds__(CB) void k_compact_targets(gbp_plan_status *st, int64_t n,
                                                        const double *__restrict__ cand,
                                                        const uint32_t *__restrict__ cflag,
                                                        double *__restrict__ targets,
                                                        _Float16 *__restrict__ tqh,
                                                        unsigned long long *tiles, uint32_t epoch,
                                                        int32_t half, int resumed, uint64_t seq) {
  if (gated(st, seq)) return;
  const int64_t i = blockIdx.x * (int64_t)CB + threadIdx.x;
  const uint32_t f = i < n ? cflag[i] : 0u;
  const bool keep = f & GBP_F_VALID;
  if (__ballot(f & GBP_F_FRAGILE) && (threadIdx.x & (WAVE - 1)) == 0) {  // the targets stage halts
    atomicOr(&st->halt, (uint32_t)GBP_PLAN_HALT_TARGETS);
    st->halt_half = half;
    raise_gate(st, seq);
  }
  const uint32_t r = ordered_rank(keep, tiles, epoch, &st->n_targets, st);
  if (keep) {
    copy8(targets + 8 * (size_t)r, cand + 8 * i);
    nn_put_hrow(tqh, nullptr, r, cand + 8 * i, false);  // the search's query rows
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) commit_targets(st, half, resumed != 0);
}

// stages 0-1 of a half whose targets were drawn ahead and searched by the
// look-ahead search (gbp_plan_halves_dev), the half's first launch on the
// caller's stream: the count and the counters, the FRAGILE halt at the half's
// start (what k_targets' last workgroup and its FRAGILE wave would have done),
// n_validate; then the search's answer completed: it saw T's first
// la->nv[half & 1] vertices (the count when it was launched), so every
// target compares its nearest with the vertices appended since (the previous
// half's connections) in fp64 — a later vertex wins only when strictly closer,
// as its index is higher (planner_class.cpp:185-200) — and rewrites its
// candidates' s_near.  Block 0 also records the next look-ahead search's
// snapshot of O (the tree the next half extends: unchanged until this half's
// connects) and whether it should run.
__global__ __launch_bounds__(TB) void k_la_commit(gbp_plan_status *st, gbp_plan_la *la, int32_t half,
                                                  const double *__restrict__ targets,
                                                  const double *__restrict__ tv,
                                                  const int32_t *__restrict__ tcount,
                                                  int32_t *__restrict__ nn, double *__restrict__ cs,
                                                  const int32_t *__restrict__ ocount, uint64_t seq) {
  const int slot = half % 3, p = half & 1;
  const bool g = gated(st, seq);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    la->nv[p ^ 1] = *ocount;
    bool go = !g;
    if (g) {
      st->n_validate = 0;  // the validate launch idles
    } else {
      const int32_t n = la->nt[slot];
      st->n_targets = n;
      commit_targets(st, half, false);
      const bool frag = la->frag[slot] == (uint32_t)half + 1;
      la->frag[slot] = 0;
      if (frag) {  // the targets stage halts
        atomicOr(&st->halt, (uint32_t)GBP_PLAN_HALT_TARGETS);
        st->halt_half = half;
        raise_gate(st, seq);
        go = false;
      }
      st->n_validate = frag ? 0 : n * GBP_NUM_GEN_STATES;
    }
    la->go[p ^ 1] = go ? 1u : 0u;
  }
  if (g) return;
  const int64_t n = la->nt[slot], v0 = la->nv[p], v1 = *tcount;
  if (v1 <= v0) return;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    double q[8];
    copy8(q, targets + 8 * i);
    const int32_t j0 = nn[i];
    int32_t bi = j0;
    double best = nn_dist64(q, tv + 8 * (int64_t)j0);
    for (int64_t j = v0; j < v1; j++) {
      const double d = nn_dist64(q, tv + 8 * j);
      if (d < best) {
        best = d;
        bi = (int32_t)j;
      }
    }
    if (bi != j0) {
      nn[i] = bi;
      for (int k = 0; k < GBP_NUM_GEN_STATES; k++)
        copy8(cs + 8 * (i * GBP_NUM_GEN_STATES + k), tv + 8 * (int64_t)bi);
    }
  }
}

// ============================================================================
// stage 2: newConfig (rrt.cpp:20-70)
// ============================================================================
template <class ZT>
__global__ __launch_bounds__(TB) void k_extend_prep(TerrainView<ZT> T, gbp_plan_status *st,
                                                    const double *__restrict__ targets,
                                                    const int32_t *__restrict__ nn,
                                                    const double *__restrict__ tv, uint64_t seed,
                                                    double *__restrict__ cs,
                                                    double *__restrict__ ca, uint64_t seq,
                                                    gbp_sampling cfg, int direction) {
  if (gated(st, seq)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) st->n_validate = 0;  // the validate launch idles
    return;
  }
  const int64_t n = st->n_targets, m = n * GBP_NUM_GEN_STATES, base = st->ext_base;
  if (blockIdx.x == 0 && threadIdx.x == 0) st->n_validate = (int32_t)m;
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < m;
       c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = c / GBP_NUM_GEN_STATES;
    const int j = (int)(c - i * GBP_NUM_GEN_STATES);
    double nv[3];
    surface_normal(T, targets[8 * i], targets[8 * i + 1], nv);  // rrt.cpp:25
    double a[10];
    sample_action_cfg(nv, cfg, direction, targets + 8 * i, tv + 8 * (int64_t)nn[i], seed,
                      GBP_EXTEND_STREAM, (base + i) * 8 + j, a);  // rrt.cpp:34, :49
    copy10(ca + 10 * c, a);
    copy8(cs + 8 * c, tv + 8 * (int64_t)nn[i]);
  }
}

// the first valid candidate (rrt.cpp:36-50) and the closer-than-s_near
// acceptance (rrt.cpp:52-68, :84-101)
__global__ __launch_bounds__(TB) void k_select(gbp_plan_status *st, const double *__restrict__ targets,
                                               const int32_t *__restrict__ nn,
                                               const double *__restrict__ tv,
                                               const double *__restrict__ ca,
                                               const double *__restrict__ csn,
                                               const uint32_t *__restrict__ cf,
                                               int32_t *__restrict__ eres,
                                               int32_t *__restrict__ echo,
                                               double *__restrict__ esn, double *__restrict__ ean,
                                               uint32_t *__restrict__ ef, int32_t half,
                                               uint64_t seq) {
  if (gated(st, seq)) return;
  const int64_t n = st->n_targets;
  bool frag = false;
  unsigned long long executed = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    double sn[8], tg[8], sv[8];
    copy8(sn, tv + 8 * (int64_t)nn[i]);
    copy8(tg, targets + 8 * i);
    int found = -1;
    uint32_t fl = 0;
    for (int j = 0; j < GBP_NUM_GEN_STATES; j++) {
      const uint32_t f = cf[i * GBP_NUM_GEN_STATES + j];
      fl |= f & (GBP_F_VALID | GBP_F_OOD | GBP_F_NAN | GBP_F_FRAGILE | GBP_F_LIMIT);
      if (f & GBP_F_VALID) {
        found = j;
        break;
      }
    }
    executed += found >= 0 ? found + 1 : GBP_NUM_GEN_STATES;
    const double d0 = state_distance(sn, tg);
    double best = d0;
    int r = GBP_TRAPPED;
    if (found >= 0) {
      const int64_t c = i * GBP_NUM_GEN_STATES + found;
      copy8(sv, csn + 8 * c);
      const double cur = state_distance(sv, tg);
      if (cur < best) {
        best = cur;
        copy8(esn + 8 * i, sv);
        copy10(ean + 10 * i, ca + 10 * c);
        r = (cur <= GOAL_BOUNDS) ? GBP_REACHED : GBP_ADVANCED;  // isWithinBounds(s_new, s)
      }
    }
    eres[i] = r;
    echo[i] = found;
    ef[i] = fl;
    frag = frag || (fl & GBP_F_FRAGILE);
  }
  // one atomic per workgroup for the statistics (same-address atomics
  // serialise: one per wave cost ~2 us a launch), one per wave for the gate
  const int lane = threadIdx.x & (WAVE - 1);
  for (int off = WAVE / 2; off > 0; off >>= 1) executed += __shfl_down(executed, off);
  __shared__ unsigned long long s_exec[TB / WAVE];
  if (lane == 0) s_exec[threadIdx.x / WAVE] = executed;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long e = 0;
    for (int k = 0; k < TB / WAVE; k++) e += s_exec[k];
    if (e) atomicAdd((unsigned long long *)&st->stat_attempts, e);
  }
  if (__ballot(frag) && lane == 0) {
    atomicOr(&st->halt, (uint32_t)GBP_PLAN_HALT_EXTEND);
    st->halt_half = half;
    raise_gate(st, seq);
  }
}

// ============================================================================
// stages 3 and 5: ordered appends (rrt.cpp:86-92, rrt_connect.cpp:107-116)
// ============================================================================
// RRT*'s list of the connections kept (rrt_star_connect.cpp:136-175:
// shared_a / shared_b), built by the stage-5 append itself when `list` is
// set (round 6; a one-workgroup launch after it before): the REACHED
// connections that were appended, in connection order, after the n_shared
// listed before — a second ordered look-back over tiles of their own
// (tiles2, epoch2; the grid's total in *tot2), the last tile publishing
// n_shared and meta[3] (the list's length for the ranking after Tb's half)
struct StarShared {
  int32_t *list = nullptr;
  int64_t max_shared = 0;
  int64_t *meta = nullptr;
  unsigned long long *tiles2 = nullptr;
  uint32_t epoch2 = 0;
  int32_t *tot2 = nullptr;
  int t_is_a = 0;
};

// mode 0: extend successors of the current targets into T (parent = nn[i]);
// mode 1: connections of the new vertices into O (parent = nno[k]), the first
// REACHED one in order recorded as the meeting point.
__global__ __launch_bounds__(CB) void k_append(gbp_plan_status *st, int mode,
                                               const int32_t *__restrict__ res,
                                               const int32_t *__restrict__ par,
                                               const double *__restrict__ sn,
                                               const double *__restrict__ an, double *__restrict__ tv,
                                               _Float16 *__restrict__ tvh, float *__restrict__ thm,
                                               double *__restrict__ ta, double *__restrict__ tg,
                                               int32_t *__restrict__ tp, int32_t *__restrict__ tcount,
                                               int32_t *__restrict__ vtx, unsigned long long *tiles,
                                               uint32_t epoch, int32_t half, int64_t cap,
                                               uint64_t seq, int32_t *tch,
                                               int32_t *tsib, int32_t *tprev, int star,
                                               StarShared sh = StarShared{}) {
  if (gated(st, seq)) return;
  __shared__ int32_t s_base;
  if (threadIdx.x == 0) s_base = *tcount;  // read before this block publishes its count
  __syncthreads();
  const int32_t base = s_base;
  const int64_t n = mode == 0 ? st->n_targets : st->n_added;
  const int64_t i = blockIdx.x * (int64_t)CB + threadIdx.x;
  const bool live = i < n;
  const int32_t r = live ? res[i] : GBP_TRAPPED;
  const bool keep = live && r != GBP_TRAPPED;
  int32_t *total = mode == 0 ? &st->n_added : &st->n_conn_added;
  const uint32_t rank = ordered_rank(keep, tiles, epoch, total, st);
  if (keep && (int64_t)base + rank >= cap) {
    // the caller reserved too little: drop, report, and gate every later
    // launch (a search over rows past cap would read out of bounds)
    atomicOr(&st->error, 2u);
    raise_gate(st, seq);
    if (vtx) vtx[i] = -1;
  } else if (keep) {
    const int32_t idx = base + (int32_t)rank, p = par[i];
    double s[8], pv[8];
    copy8(s, sn + 8 * i);
    copy8(pv, tv + 8 * (int64_t)p);
    copy8(tv + 8 * (int64_t)idx, s);
    nn_put_hrow(tvh, thm, idx, s, false);
    copy10(ta + 10 * (int64_t)idx, an + 10 * i);
    tp[idx] = p;
    tg[idx] = tg[p] + pose_distance(pv, s);  // graph_class.cpp:36-42 addEdge
    tch[idx] = -1;
    // the successor list: RRT*'s extends are joined by the insertion replay
    // (k_star_replay: choose-parent), everything else here.  A vertex is its
    // parent's first child once linked: its previous-sibling slot is cleared
    // before the exchange publishes it, and the next vertex linked to the same
    // parent (the only one the exchange returns it to) sets it afterwards.
    tprev[idx] = -1;
    if (mode == 0 && star) {
      tsib[idx] = -1;
    } else {
      __threadfence();
      const int32_t h = atomicExch(&tch[p], idx);
      tsib[idx] = h;
      if (h >= 0) tprev[h] = idx;
    }
    if (vtx) vtx[i] = idx;
    if (mode == 1 && r == GBP_REACHED && !star) {  // RRT*: every REACHED one is kept (StarShared)
      atomicMin((unsigned long long *)&st->meet,
                ((unsigned long long)i << 32) | (unsigned long long)(uint32_t)idx);
      st->meet_half = half;
      atomicOr(&st->done, 1u);
      raise_gate(st, seq);
    }
  } else if (live && vtx) {
    vtx[i] = -1;
  }
  if (sh.list) {  // (mode 1, RRT*: every block reaches here; ns read before any publishes)
    const int64_t ns = st->n_shared;
    const bool hit = keep && r == GBP_REACHED && (int64_t)base + rank < cap;
    const uint32_t r2 = ordered_rank(hit, sh.tiles2, sh.epoch2, sh.tot2, st);
    if (hit && ns + (int64_t)r2 < sh.max_shared) {
      // connection i joins T's new vertex added_base + i to O's appended row
      const int32_t tv_ = (int32_t)(st->added_base + i), ov = (int32_t)(base + rank);
      sh.list[2 * (ns + r2)] = sh.t_is_a ? tv_ : ov;
      sh.list[2 * (ns + r2) + 1] = sh.t_is_a ? ov : tv_;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
      const int64_t tot = ns + *sh.tot2;
      if (tot > sh.max_shared) {
        atomicOr(&st->error, 4u);
        raise_gate(st, seq);
      } else {
        st->n_shared = (int32_t)tot;
        sh.meta[3] = tot;
      }
    }
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    // the rows actually written (the appended count is clamped at cap)
    const int32_t added = (int32_t)min<int64_t>(*total, cap - (int64_t)base);
    *total = added;
    *tcount = base + added;
    if (mode == 0) {
      st->added_base = base;
      st->stat_added += added;
    } else {
      st->stat_conn_added += added;
    }
  }
}

// ============================================================================
// stage 4: RRTConnectClass::attemptConnect (rrt_connect.cpp:20-91)
// ============================================================================
// (connect_action, wave_pair_check: gbp_plan_dev.h)

// one wave per new vertex k of T: connect it to its nearest vertex of O with
// the recursion as a loop over levels (engine conventions of gbp.h: an
// unassigned t_new / s_new is TRAPPED; GBP_CONNECT_MAX_DEPTH levels)
template <class ZT, bool ADAPTIVE, int CM>
__global__ __launch_bounds__(TB) void k_connect(TerrainView<ZT> T, gbp_plan_status *st, int cdir,
                                                const double *__restrict__ tv,
                                                const double *__restrict__ ov,
                                                const int32_t *__restrict__ nno,
                                                int32_t *__restrict__ kres,
                                                double *__restrict__ ksn,
                                                double *__restrict__ kan,
                                                uint32_t *__restrict__ kf, int32_t half,
                                                uint64_t seq) {
  if (gated(st, seq)) return;
  const int64_t n = st->n_added, base = st->added_base;
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / WAVE);
  bool frag = false;
  unsigned long long capped = 0, checks = 0;
  for (int64_t k = blockIdx.x * (int64_t)(blockDim.x / WAVE) + threadIdx.x / WAVE; k < n;
       k += waves) {
    double se[8], s[8], sn[8], an[10];
    copy8(se, ov + 8 * (int64_t)nno[k]);  // s_near in O (rrt_connect.cpp:101-102)
    copy8(s, tv + 8 * (base + k));
    double t_s = pose_distance(s, se) / V_NOM;  // rrt_connect.cpp:89
    int res = GBP_TRAPPED;
    uint32_t cf = 0;
    for (int depth = 0;; depth++) {
      if (depth > GBP_CONNECT_MAX_DEPTH) {
        cf |= GBP_F_DEPTH_CAPPED;
        break;
      }
      if (t_s <= KINEMATICS_RES) break;  // :23-24
      const double *s_start = cdir == GBP_FORWARD ? se : s;
      const double *s_goal = cdir == GBP_FORWARD ? s : se;
      connect_action(s_start, s_goal, t_s, an);
      if (!is_valid_action(an)) break;  // :66
      double psn[8], ptn = 0;
      uint32_t pf = 0;
      checks++;  // one pair check per level (BatchStats::attempts_checked)
      const bool ok = wave_pair_check<ZT, ADAPTIVE, CM>(T, cdir == GBP_FORWARD ? s_start : s_goal,
                                                        an, cdir, psn, ptn, pf);
      cf |= pf & (GBP_F_OOD | GBP_F_NAN | GBP_F_FRAGILE | GBP_F_LIMIT);
      if (pf & GBP_F_SNEW_SET) copy8(sn, psn);
      if (ok) {
        res = depth == 0 ? GBP_REACHED : GBP_ADVANCED;  // :74-80
        break;
      }
      if (!(pf & GBP_F_TNEW_SET) || !(pf & GBP_F_SNEW_SET)) break;
      copy8(s, psn);  // :77 recurse toward the returned state with t_s = t_new
      t_s = ptn;
    }
    if (lane == 0) {
      kres[k] = res;
      if (res != GBP_TRAPPED) copy8(ksn + 8 * k, sn);
      copy10(kan + 10 * k, an);
      kf[k] = cf;
    }
    frag = frag || (cf & GBP_F_FRAGILE);
    capped += (cf & GBP_F_DEPTH_CAPPED) ? 1 : 0;
  }
  if (lane == 0) {
    if (checks) atomicAdd((unsigned long long *)&st->stat_attempts, checks);
    if (capped) atomicAdd((unsigned long long *)&st->stat_depth_capped, capped);
    if (frag) {
      atomicOr(&st->halt, (uint32_t)GBP_PLAN_HALT_CONNECT);
      st->halt_half = half;
      raise_gate(st, seq);
    }
  }
}

__global__ void k_plan_reset(gbp_plan_status *st, int64_t ext_counter, gbp_plan_la *la) {
  *la = gbp_plan_la{};  // no drawn-ahead targets, empty snapshots
  gbp_plan_status z;
  memset(&z, 0, sizeof z);
  z.meet = ~0ull;
  z.gate_seq = ~0ull;
  z.halt_half = -1;
  z.ext_half = -1;
  z.meet_half = -1;
  z.ext_counter = ext_counter;
  z.best_a = z.best_b = -1;
  z.best_cost = INFINITY;
  *st = z;
}

// standalone gbp_extend_tree_dev: the batch becomes stage 2's targets
__global__ void k_extend_setup(gbp_plan_status *st, int64_t n, const int32_t *n_dev,
                               int64_t extend_base, const double *__restrict__ src,
                               double *__restrict__ targets, _Float16 *__restrict__ tqh) {
  const int64_t m = n_dev ? *n_dev : n;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->halt = 0;
    st->done = 0;
    st->gate_seq = ~0ull;
    st->n_targets = (int32_t)m;
    st->ext_base = extend_base;
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 8 * m;
       i += (int64_t)gridDim.x * blockDim.x)
    targets[i] = src[i];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x)
    nn_put_hrow(tqh, nullptr, i, src + 8 * i, false);  // the search's query rows
}

__global__ void k_extend_out(const gbp_plan_status *st, int64_t n, const int32_t *__restrict__ eres,
                             const int32_t *__restrict__ evtx, int32_t *__restrict__ result,
                             int32_t *__restrict__ new_vertex) {
  if (st->halt) return;  // FRAGILE: gbp_extend_tree_finish_dev after the resolution
  const int64_t m = st->n_targets;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (result) result[i] = eres[i];
    if (new_vertex) new_vertex[i] = eres[i] != GBP_TRAPPED ? evtx[i] : -1;
  }
}

// the target set of half `half` (its parity)
void select_targets(gbp_plan_ws *w, int32_t half) {
  const auto &ts = w->tset[half % 3];
  w->cand = ts.cand;
  w->cflag = ts.cflag;
  w->targets = ts.targets;
  w->tqh = ts.tqh;
  w->nn = w->nnp[half & 1];
  w->cs = w->csp[half & 1];
  w->ca = w->cap[half & 1];
}

uint32_t next_epoch(gbp_plan_ws *w) {
  if (++w->epoch == 0) w->epoch = 1;
  return w->epoch;
}

unsigned tiles_for(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + CB - 1) / CB); }

// (a search's options and its launch, NnSide / NnOpts / nn_launch: gbp_nn.h)

// the look-ahead search of gbp_plan_halves_dev (targets not direction-biased,
// float heights, RRT-Connect): half h + 1's targets are drawn ahead (by half
// h's own search launch, or by half h's look-ahead search) and searched in
// O — the tree half h + 1 extends, unchanged until half h's connects — on
// la_stream while half h validates, selects, appends and connects on the
// caller's stream; half h + 1 then starts with k_la_commit (the commit and
// the vertices O gained since).  Same draws, ranks, nearest vertices and
// counters as the inline sequence.
struct LaHalf {
  bool searched = false;     // this half's targets and search came from the look-ahead
  bool launch_next = false;  // launch half + 1's look-ahead search
  bool draw_after = false;   // ... which draws half + 2's targets
  uint64_t stream_a = 0, stream_b = 0;  // the halves' target streams
};

// the targets of half h drawn ahead into their set (la->nt / frag count them)
NhDraw la_draw(gbp_plan_ws *w, int32_t h, int64_t batch, const LaHalf &L) {
  NhDraw d{};
  const auto &set = w->tset[h % 3];
  d.half = h;
  d.n = batch;
  d.base = (int64_t)(h >> 1) * batch;
  d.stream = (h & 1) ? L.stream_b : L.stream_a;
  d.cand = set.cand;
  d.targets = set.targets;
  d.cflag = set.cflag;
  d.tqh = set.tqh;
  d.draw_blocks = (int)((batch + NH_TB - 1) / NH_TB);
  d.tiles = w->la_tiles;
  d.epoch = next_epoch(w);
  d.count = &w->la->nt[h % 3];
  d.frag = &w->la->frag[h % 3];
  return d;
}

// enqueue half h1's look-ahead search on la_stream after everything the
// caller's stream holds so far; X: the tree h1 extends
int la_launch(gbp_terrain *t, gbp_plan_ws *w, const gbp_tree *X, int32_t h1, int64_t batch,
              uint64_t seed, const LaHalf &L, hipStream_t s) {
  HIPCHK(hipEventRecord(w->la_go, s));
  HIPCHK(hipStreamWaitEvent(w->la_stream, w->la_go, 0));
  const int slot = h1 % 3, p = h1 & 1;
  const auto &set = w->tset[slot];
  NhPrep<float> prep{view<float>(t), seed, w->cap[p], t->sampling,
                     (h1 & 1) ? GBP_REVERSE : GBP_FORWARD, 0, NhDraw{}, &w->la->nt[slot]};
  if (L.draw_after) prep.dr = la_draw(w, h1 + 1, batch, L);
  const NnSide side{&w->la->nv[p], &w->la->go[p]};
  // the look-ahead search: the set's fp16 rows, the candidates drawn inside,
  // the side slots and X's snapshot
  NnOpts<float> opt;
  opt.qh = set.tqh;
  opt.prep = &prep;
  opt.cs = w->csp[p];
  opt.side = &side;
  int rc = nn_launch<float>(w, &w->la->nt[slot], set.targets, nullptr, X, w->nnp[p], t->num_cus,
                            w->la_stream, opt);
  if (rc) return rc;
  HIPCHK(hipEventRecord(w->la_done, w->la_stream));
  return GBP_OK;
}

// gbp_plan_stage_timing: fold every completed timed half into the sums
void timing_collect(gbp_plan_ws *w, bool wait) {
  for (size_t i = 0; i < w->ntring; i++) {
    auto &h = w->tring[i];
    if (!h.pending) continue;
    if (wait) (void)hipEventSynchronize(h.ev[5]);
    if (hipEventQuery(h.ev[5]) != hipSuccess) continue;
    float ms[7] = {0, 0, 0, 0, 0, 0, 0};
    (void)hipEventElapsedTime(&ms[0], h.ev[0], h.ev[5]);
    (void)hipEventElapsedTime(&ms[1], h.ev[0], h.ev[1]);
    if (h.star) {
      (void)hipEventElapsedTime(&ms[2], h.ev[1], h.ev[2]);
      (void)hipEventElapsedTime(&ms[3], h.ev[3], h.ev[4]);
      (void)hipEventElapsedTime(&ms[4], h.ev[2], h.ev[5]);
      (void)hipEventElapsedTime(&ms[5], h.ev[1], h.ev[6]);
      (void)hipEventElapsedTime(&ms[6], h.ev[6], h.ev[7]);
    } else {
      (void)hipEventElapsedTime(&ms[4], h.ev[1], h.ev[5]);
    }
    for (int k = 0; k < 7; k++) w->tsum[k] += 1e3 * (double)ms[k];
    w->tcount++;
    h.pending = false;
  }
}

// the next timing slot (its previous half folded in first), or nullptr
gbp_plan_ws::TimedHalf *timing_slot(gbp_plan_ws *w) {
  if (!w->timing || !w->ntring) return nullptr;
  gbp_plan_ws::TimedHalf *h = &w->tring[w->tnext];
  w->tnext = (w->tnext + 1) % w->ntring;
  if (h->pending) timing_collect(w, true);
  return h;
}

// (the <ADAPTIVE, CM> instantiation for a run, with_adaptive_cm: gbp_plan_dev.h)

template <class ZT>
int enqueue_stages(gbp_terrain *t, gbp_plan_ws *w, gbp_tree *T, gbp_tree *O, int32_t half,
                   int direction, int64_t batch, uint64_t seed, uint64_t target_stream,
                   int64_t target_base, int adaptive, int first_stage, int last_stage,
                   hipStream_t s, const LaHalf *la = nullptr) {
  const TerrainView<ZT> V = view<ZT>(t);
  const int cus = t->num_cus;
  gbp_plan_status *st = w->st;
  w->nnw.stats = t->opt_nn_stats;
  select_targets(w, half);
  // stage order: 0 1 2 3 (RRT*: 6 7) 4 5 — the RRT* insertion runs between
  // the extends' append and the connects
  auto ord = [](int x) { return x == 6 ? 31 : x == 7 ? 32 : 10 * x; };
  auto run = [&](int x) { return ord(first_stage) <= ord(x) && ord(x) <= ord(last_stage); };
  const bool searched = la && la->searched;  // stages 0-2's draws and search done ahead
  if (searched && first_stage != 0) return GBP_E_INVALID_ARG;
  // whole halves only (a resumed one is not timed)
  gbp_plan_ws::TimedHalf *th = (O && first_stage == 0 && last_stage == 5) ? timing_slot(w) : nullptr;
  if (th) {
    th->star = w->star != 0;
    th->half = half;
    HIPCHK(hipEventRecord(th->ev[0], s));
  }
  if (searched && (!std::is_same_v<ZT, float> || t->sampling.state_flag || t->sampling.action_flag ||
                   t->informed.active))
    return GBP_E_INVALID_ARG;
  if (searched) {
    HIPCHK(hipStreamWaitEvent(s, w->la_done, 0));
    hipLaunchKernelGGL(k_la_commit, dim3(grid_for(batch, TB, cus * 4)), dim3(TB), 0, s, st, w->la, half,
                       w->targets, T->v, T->count, w->nn, w->cs, O->count, ++w->seq);
    if (la->launch_next) {
      const int rc = la_launch(t, w, O, half + 1, batch, seed, *la, s);
      if (rc) return rc;
    }
  } else if (run(0) && run(1) && t->informed.active)  // ... drawn inside the handle's ellipse
    hipLaunchKernelGGL(k_targets_informed<ZT>, dim3((unsigned)((batch + TB - 1) / TB)), dim3(TB), 0,
                       s, V, st, batch, seed, target_stream, target_base, w->cand, w->cflag,
                       w->targets, w->tqh, w->tiles, next_epoch(w), half, ++w->seq, t->sampling,
                       t->informed, T->v, T->count, O ? O->v : T->v, direction);
  else if (run(0) && run(1))  // a fresh half: draws + compaction, one launch
    hipLaunchKernelGGL(k_targets<ZT>, dim3((unsigned)((batch + TB - 1) / TB)), dim3(TB), 0, s, V,
                       st, batch, seed, target_stream, target_base, w->cand, w->cflag, w->targets,
                       w->tqh, w->tiles, next_epoch(w), half, ++w->seq, t->sampling, T->v, T->count,
                       O ? O->v : T->v, direction);
  else if (first_stage == 1 && run(1))  // resumed after a FRAGILE draw
    hipLaunchKernelGGL(k_compact_targets, dim3(tiles_for(batch)), dim3(CB), 0, s, st, batch,
                       w->cand, w->cflag, w->targets, w->tqh, w->tiles, next_epoch(w), half, 1,
                       ++w->seq);
  if (run(2)) {
    // the candidates' actions inside the search unless they are direction-biased
    // (then they depend on s_near: k_extend_prep after the search)
    NhPrep<ZT> prep{V, seed, w->ca, t->sampling, direction, 0, NhDraw{}, nullptr};
    const bool early = !t->sampling.action_flag;
    const bool launch = !searched && la && la->launch_next;
    if (launch) {
      // the next half's targets drawn beside this search (never direction-biased:
      // s_from / s_to unset) and O's snapshot for its look-ahead search
      if (!early || t->sampling.state_flag || t->informed.active || !O ||
          !std::is_same_v<ZT, float>)
        return GBP_E_INVALID_ARG;
      prep.dr = la_draw(w, half + 1, batch, *la);
      prep.dr.snap_src = O->count;
      prep.dr.snap_dst = &w->la->nv[(half + 1) & 1];
      prep.dr.go_dst = &w->la->go[(half + 1) & 1];
    }
    bool prepped = searched;
    int rc = GBP_OK;
    if (!searched) {
      // the extends' search: the targets' fp16 rows, the candidates drawn
      // inside when they may be
      NnOpts<ZT> opt;
      opt.qh = w->tqh;
      opt.prep = early ? &prep : nullptr;
      opt.cs = w->cs;
      opt.prepped = &prepped;
      rc = nn_launch<ZT>(w, &st->n_targets, w->targets, nullptr, T, w->nn, cus, s, opt);
    }
    if (!rc && launch) rc = la_launch(t, w, O, half + 1, batch, seed, *la, s);
    if (rc) return rc;
    const int64_t mmax = batch * GBP_NUM_GEN_STATES;
    if (!prepped)
      hipLaunchKernelGGL(k_extend_prep<ZT>, dim3(grid_for(mmax, TB, cus * 8)), dim3(TB), 0, s, V, st,
                         w->targets, w->nn, T->v, seed, w->cs, w->ca, ++w->seq, t->sampling,
                         direction);
    rc = gbp_internal_validate_dev_n(t, mmax, &st->n_validate, w->cs, w->ca, nullptr, direction,
                                     adaptive, nullptr, w->csn, nullptr, w->cf, w->cc, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_select, dim3(grid_for(batch, TB, cus * 4)), dim3(TB), 0, s, st, w->targets,
                       w->nn, T->v, w->ca, w->csn, w->cf, w->eres, w->echo, w->esn, w->ean, w->ef,
                       half, ++w->seq);
  }
  if (run(3))
    hipLaunchKernelGGL(k_append, dim3(tiles_for(batch)), dim3(CB), 0, s, st, 0, w->eres, w->nn,
                       w->esn, w->ean, T->v, T->vh, T->hm, T->a, T->g, T->parent, T->count, w->evtx,
                       w->tiles,
                       next_epoch(w), half, T->cap, ++w->seq, T->child, T->sibling, T->prev, w->star);
  if (th) HIPCHK(hipEventRecord(th->ev[1], s));
  const int kT = direction == GBP_FORWARD ? 0 : 1;  // T's tree index (Ta 0, Tb 1)
  gbp_plan_ws::StarSet &S = w->ss[half & 1];
  if (w->star && run(6)) {  // RRT* insertion, stage 6 (gbp_star.hip)
    const int rc = star_enqueue_checks<ZT>(t, w, T, half, direction, adaptive, th, s);
    if (rc) return rc;
  }
  if (w->star && run(7)) {  // stage 7, the ordered replay, on star_stream
    const int rc = star_enqueue_replay(w, T, half, kT, th, s);
    if (rc) return rc;
  }
  if (!O) return hipGetLastError() == hipSuccess ? GBP_OK : GBP_E_HIP;
  const int cdir = direction == GBP_FORWARD ? GBP_REVERSE : GBP_FORWARD;
  if (run(4)) {
    // queries: T's new vertices, rows [added_base, added_base + n_added)
    // the connects' search: T's fp16 rows, the direct search for any count
    NnOpts<float> opt;
    opt.qh = T->vh;
    opt.small = opt.small_any = true;
    int rc = nn_launch<float>(w, &st->n_added, T->v, &st->added_base, O, w->nno, cus, s, opt);
    if (rc) return rc;
    const int cm = (t->opt_affine && t->affine) ? 2 : 0;
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cus * GBP_CONNECT_GC, (batch + 3) / 4));
    const uint64_t kseq = ++w->seq;
    with_adaptive_cm(adaptive, cm, [&](auto ad, auto c) {
      hipLaunchKernelGGL((k_connect<ZT, decltype(ad)::value, decltype(c)::value>), dim3(g), dim3(TB), 0,
                         s, V, st, cdir, T->v, O->v, w->nno, w->kres, w->ksn, w->kan, w->kf, half,
                         kseq);
    });
  }
  if (run(5)) {
    // O's last replay (half h - 1's, on star_stream) before appending into O
    if (w->star) HIPCHK(hipStreamWaitEvent(s, w->star_rdone[1 - kT], 0));
    const bool t_is_a = direction == GBP_FORWARD;
    StarShared ssh;
    if (w->star) {  // the REACHED connections kept, listed by the append itself
      ssh.list = w->sshared;
      ssh.max_shared = w->star_max_shared;
      ssh.meta = S.meta;
      ssh.tiles2 = w->tiles + tiles_for(batch);
      ssh.tot2 = (int32_t *)(S.sfin + 8);
      ssh.t_is_a = t_is_a ? 1 : 0;
    }
    const uint32_t ep1 = next_epoch(w);
    if (w->star) ssh.epoch2 = next_epoch(w);
    hipLaunchKernelGGL(k_append, dim3(tiles_for(batch)), dim3(CB), 0, s, st, 1, w->kres, w->nno,
                       w->ksn, w->kan, O->v, O->vh, O->hm, O->a, O->g, O->parent, O->count,
                       w->star ? w->kvtx : nullptr, w->tiles, ep1, half, O->cap, ++w->seq,
                       O->child, O->sibling, O->prev, w->star, ssh);
    if (w->star && (half & 1)) {  // after Tb's half the best connection ranked
      const int rc = star_enqueue_rank(w, half, kT, t_is_a ? T->g : O->g, t_is_a ? O->g : T->g, s);
      if (rc) return rc;
    }
  }
  if (th) {
    if (th->star) HIPCHK(hipEventRecord(th->ev[4], w->star_stream));
    HIPCHK(hipEventRecord(th->ev[5], s));
    th->pending = true;
  }
  return hipGetLastError() == hipSuccess ? GBP_OK : GBP_E_HIP;
}

// enqueue_stages for the terrain's height storage
template <class... Args>
int enqueue_stages_of(gbp_terrain *t, Args... args) {
  return t->storage == GBP_STORAGE_F32 ? enqueue_stages<float>(t, args...)
                                       : enqueue_stages<double>(t, args...);
}

// the end of a planner call: nothing of it stays on la_stream or star_stream
// past the caller's stream (a host that reads the status, reserves or
// destroys after the call sees it finished).  la_done already follows the
// call's last look-ahead launch (re-recording it on the device-wide la_stream
// would also wait for other workspaces' searches: ADVICE r05); the replay and
// the ranking on star_stream end before the caller's stream goes on
int join_side_streams(gbp_plan_ws *w, hipStream_t s, bool la_used) {
  if (la_used) HIPCHK(hipStreamWaitEvent(s, w->la_done, 0));
  if (w->star) {
    HIPCHK(hipEventRecord(w->star_sdone, w->star_stream));
    HIPCHK(hipStreamWaitEvent(s, w->star_sdone, 0));
  }
  return GBP_OK;
}

}  // namespace

// ============================================================================
// C ABI (include/gbp.h "device trees and the device planner loop")
// ============================================================================
extern "C" {

// the look-ahead stream: its search launches would otherwise hold every CU's
// registers for their whole duration (3 waves per SIMD at 162 VGPRs), and the
// caller's stream's short latency-bound launches (select, appends, the
// connects' search) would wait for them; the stream is masked to all XCDs
// but the last (CUs [0, 7/8 n)), which keeps one XCD for those.  Measured on
// the planner (config-3 pair, 4-s runs): 170 M extends/s unmasked, 180 M with
// 224 of 256 CUs, 176 M with 208 or 240; spreading the excluded CUs over the
// XCDs instead was slower (profiles/r05h_la_knobs*.txt).  GBP_LA_CUS
// overrides the count (0 or >= n: unmasked, lowest priority).  One stream per
// device for the process (creating a masked queue takes milliseconds: a
// planner's time to first solution must not pay it; gbp_terrain_create
// creates it ahead), shared by the device's workspaces.
extern "C++" __attribute__((visibility("hidden"))) hipStream_t gbp_internal_la_stream(int device,
                                                                             int num_cus) {
  static std::mutex mu;
  static std::map<int, hipStream_t> streams;
  std::lock_guard<std::mutex> lk(mu);
  auto it = streams.find(device);
  if (it != streams.end()) return it->second;
  int prev = -1;
  if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  if (prev != device && hipSetDevice(device) != hipSuccess) return nullptr;
  const char *env = getenv("GBP_LA_CUS");
  // the last XCD's CUs left out (from the device's XCC count, not
  // an assumed 8; one XCC or an unknown count: unmasked)
  int xcc = 0;
  if (hipDeviceGetAttribute(&xcc, hipDeviceAttributeNumberOfXccs, device) != hipSuccess) xcc = 0;
  const int n = num_cus, cus = env && *env ? atoi(env) : (xcc >= 2 ? n - n / xcc : n);
  hipStream_t st = nullptr;
  hipError_t e;
  if (cus > 0 && cus < n) {
    std::vector<uint32_t> mask((n + 31) / 32, 0u);
    for (int c = 0; c < cus; c++) mask[c / 32] |= 1u << (c % 32);
    e = hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data());
  } else {
    int lo = 0, hi = 0;
    e = hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, lo);
  }
  if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
  if (e != hipSuccess) return nullptr;
  if (streams.empty()) {
    // destroyed before the HIP runtime's own exit handlers run (registered
    // earlier, so they run later): a profiler's teardown walking the
    // process's queues at exit found this one still alive and faulted
    std::atexit([] {
      for (auto &kv : streams) (void)hipStreamDestroy(kv.second);
      streams.clear();
    });
  }
  streams[device] = st;
  return st;
}

static void ws_free(gbp_plan_ws *w) {
  if (w->ntring) {
    (void)hipDeviceSynchronize();
    for (size_t i = 0; i < w->ntring; i++)
      for (auto &e : w->tring[i].ev)
        if (e) (void)hipEventDestroy(e);
    delete[] w->tring;
  }
  if (w->la_go) (void)hipEventDestroy(w->la_go);
  if (w->la_done) (void)hipEventDestroy(w->la_done);
  star_stream_destroy(w);
  if (w->block) (void)hipFree(w->block);
  if (w->star_block) (void)hipFree(w->star_block);
  if (w->replan) (void)hipFree(w->replan);
  delete w;
}

int gbp_plan_ws_create(gbp_terrain *t, int64_t max_batch, gbp_plan_ws **out) {
  if (!t || !out) return GBP_E_INVALID_ARG;
  if (max_batch < 1 || max_batch > (1 << 24)) return GBP_E_INVALID_ARG;
  *out = nullptr;
  DeviceGuard g(t->device);
  gbp_plan_ws *w = new (std::nothrow) gbp_plan_ws();
  if (!w) return GBP_E_ALLOC;
  w->device = t->device;
  w->num_cus = t->num_cus;
  w->nnw.stats = t->opt_nn_stats;
  w->bmax = max_batch;
  nn_ws_init(w->nnw, max_batch, t->num_cus);
  w->ntiles = (max_batch + TB - 1) / TB + 1;  // k_targets' 256-draw tiles (k_compact_targets: 1024)
  const int64_t b = max_batch, m = GBP_NUM_GEN_STATES * max_batch;
  // the block's arrays, in order; the list sizes the allocation (Stage)
  auto arrays = [w, b, m](Stage &S) {
    S.take(w->st, 1);
    S.take(w->la, 1);
    S.take(w->tiles, w->ntiles);
    S.take(w->la_tiles, w->ntiles);
    for (auto &ts : w->tset) {
      S.take(ts.cand, 8 * b);
      S.take(ts.cflag, b);
      S.take(ts.targets, 8 * b);
      S.take(ts.tqh, NH_ROW * b);
    }
    for (int k = 0; k < 2; k++) {
      S.take(w->nnp[k], b);
      S.take(w->csp[k], 8 * m);
      S.take(w->cap[k], 10 * m);
    }
    S.take(w->csn, 8 * m);
    S.take(w->cf, m);
    S.take(w->cc, m);
    S.take(w->eres, b);
    S.take(w->echo, b);
    S.take(w->esn, 8 * b);
    S.take(w->ean, 10 * b);
    S.take(w->ef, b);
    S.take(w->evtx, b);
    S.take(w->nno, b);
    S.take(w->kres, b);
    S.take(w->ksn, 8 * b);
    S.take(w->kan, 10 * b);
    S.take(w->kf, b);
    nn_ws_carve(w->nnw, S, b);  // the searches' arrays: the last of the block
  };
  const size_t bytes = stage_bytes_of(arrays);
  if (hipMalloc(&w->block, bytes) != hipSuccess) {
    delete w;
    return GBP_E_ALLOC;
  }
  if (stage_carve(w->block, bytes, arrays) != GBP_OK) {
    ws_free(w);
    return GBP_E_ALLOC;
  }
  select_targets(w, 0);
  bool ok = nn_ws_zero(w->nnw) == GBP_OK &&
            hipMemset(w->tiles, 0, 8 * w->ntiles) == hipSuccess &&
            hipMemset(w->la_tiles, 0, 8 * w->ntiles) == hipSuccess &&
            (w->la_stream = gbp_internal_la_stream(w->device, w->num_cus)) != nullptr &&
            hipEventCreateWithFlags(&w->la_go, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&w->la_done, hipEventDisableTiming) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_plan_reset, dim3(1), dim3(1), 0, nullptr, w->st, (int64_t)0, w->la);
    ok = hipDeviceSynchronize() == hipSuccess;
  }
  if (!ok) {
    ws_free(w);
    return GBP_E_HIP;
  }
  *out = w;
  return GBP_OK;
}

int gbp_plan_ws_destroy(gbp_plan_ws *w) {
  if (!w) return GBP_E_BAD_HANDLE;
  DeviceGuard g(w->device);
  (void)hipDeviceSynchronize();
  ws_free(w);
  return GBP_OK;
}

int gbp_plan_stage_timing(gbp_plan_ws *w, int enable) {
  if (!w) return GBP_E_BAD_HANDLE;
  DeviceGuard g(w->device);
  if (enable && !w->ntring) {
    w->tring = new (std::nothrow) gbp_plan_ws::TimedHalf[256];
    if (!w->tring) return GBP_E_ALLOC;
    w->ntring = 256;
    for (size_t i = 0; i < w->ntring; i++)
      for (auto &e : w->tring[i].ev)
        if (hipEventCreate(&e) != hipSuccess) return GBP_E_HIP;
  }
  w->timing = enable != 0;
  return GBP_OK;
}

int gbp_plan_stage_times(gbp_plan_ws *w, double *us, int n, int64_t *halves, int reset) {
  if (!w) return GBP_E_BAD_HANDLE;
  if (!us || n < 5) return GBP_E_INVALID_ARG;
  DeviceGuard g(w->device);
  timing_collect(w, false);
  for (int k = 0; k < std::min(n, 7); k++) us[k] = w->tsum[k];
  if (halves) *halves = w->tcount;
  if (reset) {
    for (double &x : w->tsum) x = 0;
    w->tcount = 0;
  }
  return GBP_OK;
}

int gbp_plan_reset(gbp_plan_ws *w, int64_t extend_counter, gbp_stream stream) {
  if (!w) return GBP_E_BAD_HANDLE;
  DeviceGuard g(w->device);
  hipLaunchKernelGGL(k_plan_reset, dim3(1), dim3(1), 0, (hipStream_t)stream, w->st, extend_counter,
                     w->la);
  HIPCHK(hipGetLastError());
  return GBP_OK;
}

int gbp_plan_status_read(gbp_plan_ws *w, gbp_plan_status *out, gbp_stream stream) {
  if (!w) return GBP_E_BAD_HANDLE;
  if (!out) return GBP_E_INVALID_ARG;
  DeviceGuard g(w->device);
  HIPCHK(hipMemcpyAsync(out, w->st, sizeof *out, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return GBP_OK;
}

int gbp_plan_half_dev(gbp_terrain *t, gbp_plan_ws *w, gbp_tree *T, gbp_tree *O, int32_t half,
                      int direction, int64_t batch, uint64_t seed, uint64_t target_stream,
                      int64_t target_index_base, int adaptive, int first_stage,
                      gbp_stream stream) {
  if (!t || !w || !tree_ok(T) || !tree_ok(O)) return GBP_E_BAD_HANDLE;
  if (batch < 1 || batch > w->bmax || first_stage < 0 || first_stage > (w->star ? 7 : 5) ||
      (direction != GBP_FORWARD && direction != GBP_REVERSE) || T == O)
    return GBP_E_INVALID_ARG;
  DeviceGuard g(t->device);
  hipStream_t s = (hipStream_t)stream;
  const int rc = enqueue_stages_of(t, w, T, O, half, direction, batch, seed, target_stream,
                                   target_index_base, adaptive, first_stage, 5, s, nullptr);
  const int jrc = join_side_streams(w, s, false);
  return jrc ? jrc : rc;
}

int gbp_plan_halves_dev(gbp_terrain *t, gbp_plan_ws *w, gbp_tree *Ta, gbp_tree *Tb,
                        int32_t first_half, int32_t n_halves, int64_t batch, uint64_t seed,
                        uint64_t stream_a, uint64_t stream_b, int adaptive, int first_stage,
                        gbp_stream stream) {
  if (!t || !w || !tree_ok(Ta) || !tree_ok(Tb)) return GBP_E_BAD_HANDLE;
  if (batch < 1 || batch > w->bmax || first_stage < 0 || first_stage > (w->star ? 7 : 5) ||
      n_halves < 0 || first_half < 0 || Ta == Tb)
    return GBP_E_INVALID_ARG;
  DeviceGuard g(t->device);
  hipStream_t s = (hipStream_t)stream;
  // the look-ahead search (LaHalf, la_launch): half h+1's draws do not depend
  // on the trees unless the sampling is direction-biased, and its search
  // needs only O as it stands before half h's connects, so both run on
  // la_stream beside half h; half h+1 starts with k_la_commit
  static const bool la_off = [] {  // GBP_LA_OFF=1: the inline sequence (A/B, diagnostics)
    const char *e = getenv("GBP_LA_OFF");
    return e && *e && *e != '0';
  }();
  // (RRT* too: its insertion rewires the extended tree's parents and g, not
  // its vertices, and the connects still append to O after the snapshot)
  // (informed targets are drawn by k_targets_informed alone: the search launch's draws
  // are the plain sampler's, so an active ellipse runs the inline sequence)
  const bool ahead = !la_off && !t->sampling.state_flag && !t->sampling.action_flag &&
                     !t->informed.active &&
                     t->storage == GBP_STORAGE_F32;  // (k_nn_mfma<float> draws)
  bool searched = false, used = false;
  int rc = GBP_OK;
  if (first_stage != 0)  // a resume: the halted half and the gated ones after it ran nothing
    for (size_t i = 0; i < w->ntring; i++)
      if (w->tring[i].pending && w->tring[i].half >= first_half) w->tring[i].pending = false;
  for (int32_t i = 0; i < n_halves && !rc; i++) {
    const int32_t h = first_half + i;
    const int k = h & 1;
    gbp_tree *T = k ? Tb : Ta, *O = k ? Ta : Tb;
    const int dir = k ? GBP_REVERSE : GBP_FORWARD;
    const uint64_t ts = k ? stream_b : stream_a;
    const int64_t tb = (int64_t)(h >> 1) * batch;
    const int fs = i == 0 ? first_stage : 0;
    LaHalf L;
    L.searched = searched;
    L.launch_next = ahead && i + 1 < n_halves && (searched || fs <= 2);
    L.draw_after = ahead && i + 2 < n_halves;
    L.stream_a = stream_a;
    L.stream_b = stream_b;
    rc = enqueue_stages_of(t, w, T, O, h, dir, batch, seed, ts, tb, adaptive, fs, 5, s, &L);
    searched = L.launch_next;
    used = used || L.launch_next;
  }
  const int jrc = join_side_streams(w, s, used);
  return jrc ? jrc : rc;
}

int gbp_extend_tree_dev(gbp_terrain *t, gbp_plan_ws *w, gbp_tree *T, int64_t n,
                        const double *targets, const int32_t *n_dev, int direction, int adaptive,
                        uint64_t seed, int64_t extend_base, int32_t *result, int32_t *new_vertex,
                        gbp_stream stream) {
  if (!t || !w || !tree_ok(T)) return GBP_E_BAD_HANDLE;
  if (n < 0 || n > w->bmax || (n > 0 && !targets) ||
      (direction != GBP_FORWARD && direction != GBP_REVERSE))
    return GBP_E_INVALID_ARG;
  if (n == 0) return GBP_OK;
  DeviceGuard g(t->device);
  hipStream_t s = (hipStream_t)stream;
  select_targets(w, 0);
  hipLaunchKernelGGL(k_extend_setup, dim3(grid_for(8 * n, TB, t->num_cus * 4)), dim3(TB), 0, s,
                     w->st, n, n_dev, extend_base, targets, w->targets, w->tqh);
  int rc = enqueue_stages_of(t, w, T, nullptr, 0, direction, n, seed, 0, 0, adaptive, 2, 3, s, nullptr);
  if (rc) return rc;
  hipLaunchKernelGGL(k_extend_out, dim3(grid_for(n, TB, t->num_cus * 4)), dim3(TB), 0, s, w->st, n,
                     w->eres, w->evtx, result, new_vertex);
  HIPCHK(hipGetLastError());
  return GBP_OK;
}

int gbp_extend_tree_finish_dev(gbp_terrain *t, gbp_plan_ws *w, gbp_tree *T, int64_t n,
                               int direction, int32_t *result, int32_t *new_vertex,
                               gbp_stream stream) {
  if (!t || !w || !tree_ok(T)) return GBP_E_BAD_HANDLE;
  if (n < 0 || n > w->bmax) return GBP_E_INVALID_ARG;
  if (n == 0) return GBP_OK;
  DeviceGuard g(t->device);
  hipStream_t s = (hipStream_t)stream;
  int rc = enqueue_stages_of(t, w, T, nullptr, 0, direction, n, 0, 0, 0, 0, 3, 3, s, nullptr);
  if (rc) return rc;
  hipLaunchKernelGGL(k_extend_out, dim3(grid_for(n, TB, t->num_cus * 4)), dim3(TB), 0, s, w->st, n,
                     w->eres, w->evtx, result, new_vertex);
  HIPCHK(hipGetLastError());
  return GBP_OK;
}

int gbp_extend_tree_host(gbp_terrain *t, gbp_plan_ws *w, gbp_tree *T, int64_t n,
                         const double *targets, int direction, int adaptive, uint64_t seed,
                         int64_t extend_base, int32_t *result, int32_t *new_vertex,
                         int64_t *n_resolved) {
  if (!t || !w || !tree_ok(T)) return GBP_E_BAD_HANDLE;
  if (n < 0 || n > w->bmax || (n > 0 && (!targets || !result))) return GBP_E_INVALID_ARG;
  if (n_resolved) *n_resolved = 0;
  if (n == 0) return GBP_OK;
  DeviceGuard g(t->device);
  hipStream_t s = t->host_stream;
  int64_t cnt = 0;
  int rc = gbp_tree_size(T, &cnt, s);
  if (!rc && cnt + n > T->cap) rc = gbp_tree_reserve(T, std::max<int64_t>(2 * T->cap, cnt + n), s);
  if (rc) return rc;
  DevBuf buf;
  double *dt;
  int32_t *dr, *dv;
  rc = stage_buf(buf, [&](Stage &S) { S.take(dt, 8 * n); S.take(dr, n); S.take(dv, n); });
  if (rc) return rc;
  rc = h2d(dt, targets, 8 * n, s);
  if (!rc) rc = gbp_plan_reset(w, 0, s);
  if (!rc)
    rc = gbp_extend_tree_dev(t, w, T, n, dt, nullptr, direction, adaptive, seed, extend_base, dr,
                             dv, s);
  gbp_plan_status st;
  if (!rc) rc = gbp_plan_status_read(w, &st, s);
  if (!rc && st.halt) {
    int resume = -1;
    rc = gbp_plan_resolve_host(t, w, T, nullptr, direction, n, adaptive, &resume, n_resolved, s);
    if (!rc) rc = gbp_extend_tree_finish_dev(t, w, T, n, direction, dr, dv, s);
  }
  if (!rc) rc = d2h(result, dr, n, s);
  if (!rc && new_vertex) rc = d2h(new_vertex, dv, n, s);
  if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = GBP_E_HIP;
  return rc;
}

// gbp_plan_resolve_host's re-decisions, one per halted stage: the stage's
// FRAGILE items decided again on the host with glibc and its outputs patched
// on the device, item by item (a group has a handful); *k counts them

// isValidState(s_rand, STANCE) of the half's draws (rrt_connect.cpp:254)
static int resolve_targets(gbp_terrain *t, gbp_plan_ws *w, int64_t batch, hipStream_t s, int64_t *k) {
  if (batch < 1 || batch > w->bmax) return GBP_E_INVALID_ARG;
  int rc;
  std::vector<uint32_t> fl(batch);
  const gbp_host::Terrain *H = host_mirror(t);
  if (!H) return GBP_E_HIP;
  if ((rc = d2h(fl.data(), w->cflag, batch, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  for (int64_t i = 0; i < batch; i++) {
    if (!(fl[i] & GBP_F_FRAGILE)) continue;
    double q[8];
    if ((rc = d2h(q, w->cand + 8 * i, 8, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    gbp_host::Acc acc;
    const bool v = gbp_host::is_valid_state(*H, q, GBP_STANCE, acc);
    fl[i] = acc.flags | (v ? GBP_F_VALID : 0u) | GBP_F_RESOLVED;
    if ((rc = h2d(w->cflag + i, &fl[i], 1, s))) return rc;
    ++*k;
  }
  return GBP_OK;
}

// newConfig + acceptance (rrt.cpp:20-101) of every extend with a FRAGILE
// executed candidate, on the device's own candidate actions
static int resolve_extend(gbp_terrain *t, gbp_plan_ws *w, const gbp_tree *T, int64_t n, int direction,
                          int adaptive, hipStream_t s, int64_t *k) {
  int rc;
  std::vector<uint32_t> ef(n);
  const gbp_host::Terrain *H = host_mirror(t);
  if (!H) return GBP_E_HIP;
  if ((rc = d2h(ef.data(), w->ef, n, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  for (int64_t i = 0; i < n; i++) {
    if (!(ef[i] & GBP_F_FRAGILE)) continue;
    int32_t nn = 0;
    double tg[8], sn0[8], act[10 * GBP_NUM_GEN_STATES];
    if ((rc = d2h(&nn, w->nn + i, 1, s)) || (rc = d2h(tg, w->targets + 8 * i, 8, s)) ||
        (rc = d2h(act, w->ca + 10 * GBP_NUM_GEN_STATES * i, 10 * GBP_NUM_GEN_STATES, s)))
      return rc;
    HIPCHK(hipStreamSynchronize(s));
    if ((rc = d2h(sn0, T->v + 8 * (int64_t)nn, 8, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    const double best0 = gbp_host::state_distance(sn0, tg);
    double best = best0, s_test[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t_test = 0, s_new[8];
    uint32_t fl = 0;
    int found = -1;
    for (int j = 0; j < GBP_NUM_GEN_STATES; j++) {
      uint32_t f = 0;
      const bool v = gbp_host::pair_check(*H, sn0, act + 10 * j, direction, adaptive, s_test,
                                          &t_test, &f, nullptr);
      fl |= f & (GBP_F_VALID | GBP_F_OOD | GBP_F_NAN | GBP_F_LIMIT);
      if (v) {
        found = j;
        break;
      }
    }
    int32_t r = GBP_TRAPPED;
    if (found >= 0) {
      const double cur = gbp_host::state_distance(s_test, tg);
      if (cur < best) {
        best = cur;
        memcpy(s_new, s_test, sizeof s_new);
        r = cur <= GOAL_BOUNDS ? GBP_REACHED : GBP_ADVANCED;
        if ((rc = h2d(w->esn + 8 * i, s_new, 8, s)) ||
            (rc = h2d(w->ean + 10 * i, act + 10 * found, 10, s)))
          return rc;
      }
    }
    const uint32_t fr = fl | GBP_F_RESOLVED;
    if ((rc = h2d(w->eres + i, &r, 1, s)) || (rc = h2d(w->echo + i, &found, 1, s)) ||
        (rc = h2d(w->ef + i, &fr, 1, s)))
      return rc;
    HIPCHK(hipStreamSynchronize(s));
    ++*k;
  }
  return GBP_OK;
}

// RRTConnectClass::attemptConnect (rrt_connect.cpp:20-91) of every
// connection with a FRAGILE level, recursion replayed on the host
static int resolve_connect(gbp_terrain *t, gbp_plan_ws *w, const gbp_tree *T, const gbp_tree *O,
                           const gbp_plan_status &st, int direction, int adaptive, hipStream_t s,
                           int64_t *k) {
  if (!tree_ok(O)) return GBP_E_BAD_HANDLE;
  int rc;
  const int64_t n = st.n_added, base = st.added_base;
  const gbp_host::Terrain *H = host_mirror(t);
  if (!H) return GBP_E_HIP;
  const int cdir = direction == GBP_FORWARD ? GBP_REVERSE : GBP_FORWARD;
  std::vector<uint32_t> kf(n);
  if ((rc = d2h(kf.data(), w->kf, n, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  for (int64_t i = 0; i < n; i++) {
    if (!(kf[i] & GBP_F_FRAGILE)) continue;
    int32_t j = 0;
    double se[8], sq[8], sn[8] = {0, 0, 0, 0, 0, 0, 0, 0}, an[10];
    if ((rc = d2h(&j, w->nno + i, 1, s)) || (rc = d2h(sq, T->v + 8 * (base + i), 8, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    if ((rc = d2h(se, O->v + 8 * (int64_t)j, 8, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    const double t_s = gbp_host::pose_distance(sq, se) / V_NOM;
    uint32_t f = 0;
    const int32_t r = gbp_host::attempt_connect(*H, se, sq, t_s, sn, an, cdir, adaptive,
                                                GBP_CONNECT_MAX_DEPTH, &f);
    const uint32_t fr = f | GBP_F_RESOLVED;
    if ((rc = h2d(w->kres + i, &r, 1, s)) || (rc = h2d(w->kan + 10 * i, an, 10, s)) ||
        (rc = h2d(w->kf + i, &fr, 1, s)))
      return rc;
    if (r != GBP_TRAPPED && (rc = h2d(w->ksn + 8 * i, sn, 8, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    ++*k;
  }
  return GBP_OK;
}

// the RRT* insertion's connect checks (their pair checks, rows of stage 6)
static int resolve_star(gbp_terrain *t, gbp_plan_ws *w, const gbp_plan_status &st, int direction,
                        int adaptive, hipStream_t s, int64_t *k) {
  int rc;
  const int64_t n = st.star_rows;
  const gbp_host::Terrain *H = host_mirror(t);
  if (!H) return GBP_E_HIP;
  std::vector<uint32_t> rf(n);
  const gbp_plan_ws::StarSet &S = w->ss[st.halt_half & 1];
  if (n && (rc = d2h(rf.data(), S.srf, n, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  for (int64_t i = 0; i < n; i++) {
    if (!(rf[i] & GBP_F_FRAGILE)) continue;
    double sv[8], av[10], sn[8], tn = 0;
    if ((rc = d2h(sv, S.srs + 8 * i, 8, s)) || (rc = d2h(av, S.sra + 10 * i, 10, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    uint32_t f = 0;
    const bool v = gbp_host::pair_check(*H, sv, av, direction, adaptive, sn, &tn, &f, nullptr);
    const uint32_t fr = (f & ~GBP_F_FRAGILE) | (v ? GBP_F_VALID : 0u) | GBP_F_RESOLVED;
    if ((rc = h2d(S.srf + i, &fr, 1, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    ++*k;
  }
  return GBP_OK;
}

// nothing to re-decide: the caller has grown the insertion sets
// (gbp_plan_star_config); the half redoes its stage 6
static int resolve_star_pairs(const gbp_plan_ws *w, const gbp_plan_status &st) {
  return 2 * (int64_t)st.star_pairs > 2 * w->star_max_pairs ? GBP_E_SHAPE : GBP_OK;
}

int gbp_plan_resolve_host(gbp_terrain *t, gbp_plan_ws *w, gbp_tree *T, gbp_tree *O, int direction,
                          int64_t batch, int adaptive, int *resume_stage, int64_t *n_resolved,
                          gbp_stream stream) {
  if (!t || !w || !tree_ok(T)) return GBP_E_BAD_HANDLE;
  if (!resume_stage) return GBP_E_INVALID_ARG;
  DeviceGuard g(t->device);
  hipStream_t s = (hipStream_t)stream;
  gbp_plan_status st;
  int rc = gbp_plan_status_read(w, &st, stream);
  if (rc) return rc;
  *resume_stage = -1;
  int64_t k = 0;
  select_targets(w, st.halt_half >= 0 ? st.halt_half : 0);  // the halted half's target set
  int resume = -1;  // the stage the half resumes at
  if (st.halt & GBP_PLAN_HALT_STAR_PAIRS) {
    rc = resolve_star_pairs(w, st);
    resume = 6;
  } else if (st.halt & GBP_PLAN_HALT_TARGETS) {
    rc = resolve_targets(t, w, batch, s, &k);
    resume = 1;
  } else if (st.halt & GBP_PLAN_HALT_EXTEND) {
    rc = resolve_extend(t, w, T, st.n_targets, direction, adaptive, s, &k);
    resume = 3;
  } else if (st.halt & GBP_PLAN_HALT_CONNECT) {
    rc = resolve_connect(t, w, T, O, st, direction, adaptive, s, &k);
    resume = 5;
  } else if (st.halt & GBP_PLAN_HALT_STAR) {
    rc = resolve_star(t, w, st, direction, adaptive, s, &k);
    resume = 7;
  }
  if (rc) return rc;
  *resume_stage = resume;
  if (resume >= 0) {
    st.halt = 0;
    if (!st.done) st.gate_seq = ~0ull;
    st.stat_fragile_resolved += k;
    if ((rc = h2d(w->st, &st, 1, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
  }
  if (n_resolved) *n_resolved = k;
  return GBP_OK;
}

}  // extern "C"
