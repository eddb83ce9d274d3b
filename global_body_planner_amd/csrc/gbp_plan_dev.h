// gbp_plan_dev.h — what the planner's translation units share on the device
// (gbp_plan.hip, gbp_nn.hip, gbp_star.hip, gbp_shortcut.hip) and the graft's
// checks (gbp_tree_graft.hip): the launch gate,
// the connect action and the pair check by a whole wave, and the host's pick
// of their <ADAPTIVE, CM> instantiation.  Device only; not part of the C ABI.
#pragma once

#include <type_traits>

#include "gbp_closed_forms.h"
#include "gbp_internal.h"
#include "gbp_lane.h"

namespace gbp {

// the gate every planner kernel checks first: a FRAGILE halt or a found
// connection raised by an EARLIER launch makes the rest of the enqueued
// sequence a no-op.  Each launch carries its sequence number `seq`
// (gbp_plan_ws::seq); the launch that raises the gate records its own
// (gate_seq, atomicMin), so a workgroup dispatched after another workgroup of
// the same launch raised it still computes its items — the host's
// resolution and resume rely on every item of the halted stage being final.
__device__ __forceinline__ bool gated(const gbp_plan_status *st, uint64_t seq) {
  return __hip_atomic_load(&st->gate_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < seq;
}
__device__ __forceinline__ void raise_gate(gbp_plan_status *st, uint64_t seq) {
  atomicMin((unsigned long long *)&st->gate_seq, (unsigned long long)seq);
}

// ============================================================================
// RRTConnectClass::attemptConnect (rrt_connect.cpp:20-91): what stage 4's
// k_connect, RRT*'s k_star_check, k_shortcut_pairs and k_graft_check share
// ============================================================================
#ifndef GBP_STAR_GC
#define GBP_STAR_GC 2  // k_star_check workgroups (4 waves) per CU
#endif
#ifndef GBP_CONNECT_GC
#define GBP_CONNECT_GC 4  // k_connect workgroups (4 waves, one connection each) per CU
#endif
#ifndef GBP_SHORTCUT_GC
#define GBP_SHORTCUT_GC 4  // k_shortcut_pairs workgroups (4 waves, one pair each) per CU
#endif

// connect_action (rrt_connect.cpp:53-63): gbp_closed_forms.h

// One pair check (planning_utils.cpp:645-881) by a whole wave: every lane
// holds the same Lane state (wave-uniform); per step, lane j evaluates the
// sample j positions ahead on the all-pass path (advance_on_success), then
// every lane replays the reference's transitions on the ballot of results in
// order, stopping at the first failure or decision (the all-pass path crosses
// stage boundaries deterministically) — exactly the reference's samples are
// counted.  Connect actions run t_s / 0.05 + 1
// stance samples (dozens to hundreds): a wave covers 64 of them per step.
template <class ZT, bool ADAPTIVE, int CM>
static __device__ bool wave_pair_check(const TerrainView<ZT> &T, const double *s_in, const double *a_in,
                                       int dir, double *s_new, double &t_new, uint32_t &flags) {
  const int lane = threadIdx.x & (WAVE - 1);
  double sv[8], av[10];
  copy8(sv, s_in);
  copy10(av, a_in);
  Lane L;
  L.s = sv;
  L.a = av;
  L.f = 0;
  L.acc = Acc{0, 0, 0};
  L.snew_kind = SN_NONE;
  L.tnew_set = 0;
  enter_stage(L, dir == GBP_FORWARD ? ST_FWD_STANCE : ST_REV_FLIGHT);
  bool decided = false;
  while (!decided) {
    int stg = L.stage;
    double t = L.t, ts = L.ts;
    bool has = true;
    for (int k = 0; k < lane && has; k++) has = advance_on_success<ADAPTIVE>(stg, av, t, ts);
    const double t_eval = lane == 0 ? stage_time(L) : sample_time(stg, av, t);
    Acc acc{0, L.acc.V + (uint32_t)lane, 0};
    bool ok = false;
    if (has) {
      double sc[8];
      sample_state(sv, av, stg, t_eval, sc);
      ok = is_valid_state<ZT, CM>(T, sc, stage_phase(stg), acc);
    }
    const unsigned long long okm = __ballot(ok), hasm = __ballot(has);
    // The replay in parallel.  hasm is a prefix of the lanes (a lane past a
    // deciding sample has none); the run [0, j0) of passing samples ends at
    // the first failing or LIMIT one.  Each lane of the run applies its own
    // sample's success transition to its speculated pre-state (stg, t, ts:
    // the same arithmetic the in-order replay performs), so the attempt's
    // state after the run is the last run lane's; s_new / t_new are the last
    // ones a run lane set; G, flags and V add up over the run.  Then the
    // stop lane's sample, if any, goes through the in-order transition.
    const unsigned long long limm = __ballot(has && (acc.flags & GBP_F_LIMIT));
    const unsigned long long stopm = hasm & (~okm | limm);
    const int j0 = stopm ? __builtin_ctzll(stopm) : __popcll(hasm);
    const bool inrun = lane < j0;
    Lane P = L;
    P.stage = stg;
    P.t = t;
    P.ts = ts;
    P.f = stage_bits((uint32_t)stg);
    P.snew_kind = SN_NONE;
    P.tnew_set = 0;
    bool dec = false;
    if (inrun) dec = transition<ADAPTIVE>(P, true);
    uint32_t g = inrun ? acc.G : 0u, fl = inrun ? acc.flags : 0u;
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
      g += __shfl_xor(g, o);
      fl |= __shfl_xor(fl, o);
    }
    L.acc.G += g;
    L.acc.flags |= fl;
    L.acc.V += (uint32_t)j0;
    if (j0 > 0) {
      const int jl = j0 - 1;
      L.stage = __shfl(P.stage, jl);
      L.t = __shfl(P.t, jl);
      L.ts = __shfl(P.ts, jl);
      L.tpre = __shfl(P.tpre, jl);
      L.f = __shfl(P.f, jl);
      decided = __shfl((int)dec, jl) != 0;
      const unsigned long long sm = __ballot(inrun && P.snew_kind != SN_NONE);
      if (sm) {
        const int js = 63 - __builtin_clzll(sm);
        L.snew_kind = __shfl(P.snew_kind, js);
        L.snew_p = __shfl(P.snew_p, js);
      }
      const unsigned long long tm = __ballot(inrun && P.tnew_set);
      if (tm) {
        const int jt = 63 - __builtin_clzll(tm);
        L.tnew = __shfl(P.tnew, jt);
        L.tnew_set = 1;
      }
    }
    if (!decided && stopm) {
      const uint32_t fj = __shfl(acc.flags, j0), gj = __shfl(acc.G, j0);
      L.acc.G += gj;
      L.acc.flags |= fj;
      if (fj & GBP_F_LIMIT) {
        decided = true;
      } else {
        L.acc.V += 1;
        decided = transition<ADAPTIVE>(L, ((okm >> j0) & 1ull) != 0);
      }
    }
  }
  uint32_t f = L.f | L.acc.flags;
  if (L.snew_kind != SN_NONE) {
    f |= GBP_F_SNEW_SET;
    sample_state(sv, av,
                 L.snew_kind == SN_STANCE_S ? ST_FWD_STANCE
                                            : (L.snew_kind == SN_FLIGHT_B ? ST_FWD_LAND : ST_REV_STANCE),
                 L.snew_p, s_new);
  }
  if (L.tnew_set) {
    f |= GBP_F_TNEW_SET;
    t_new = L.tnew;
  }
  flags = f;
  return (f & GBP_F_VALID) != 0;
}

// the <ADAPTIVE, CM> instantiation of k_connect / k_star_check /
// k_shortcut_pairs for the run's (adaptive, cm):
// f(bool_constant<AD>, integral_constant<int, CM>), CM 2 (the verified affine
// coordinates) or 0 — those four and no others
template <class F>
static void with_adaptive_cm(bool adaptive, int cm, F f) {
  using CM0 = std::integral_constant<int, 0>;
  using CM2 = std::integral_constant<int, 2>;
  if (adaptive) {
    if (cm == 2) f(std::true_type{}, CM2{}); else f(std::true_type{}, CM0{});
  } else {
    if (cm == 2) f(std::false_type{}, CM2{}); else f(std::false_type{}, CM0{});
  }
}

}  // namespace gbp
