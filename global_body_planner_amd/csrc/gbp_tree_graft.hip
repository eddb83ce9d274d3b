// gbp_tree_graft.hip — which vertices of a device tree a new root state
// attaches (gbp_tree_graft_check_dev, stage A of the graft): the
// distance test, the connect action and its pair check, one wave per vertex.
// The pair check by a whole wave it shares with the planner's connects
// (gbp_plan_dev.h); the graft itself is gbp_tree_maint.hip's.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "gbp.h"
#include "gbp_device.h"
#include "gbp_internal.h"
#include "gbp_plan_dev.h"

using namespace gbp;

namespace {

#ifndef GBP_GRAFT_GC
#define GBP_GRAFT_GC 2  // k_graft_check workgroups (4 waves) per CU, as k_star_check
#endif

struct GraftRoot {  // the root state travels as the kernel's argument
  double s[8];
};

// Vertex j of the tree against the root r, one wave per vertex, grid-stride
// over all n (no compaction first: a vertex outside the radius costs its wave
// one 64-B row and eight subtractions, a candidate a pair check of tens of
// samples; striding spreads the candidates over the waves whatever their
// indices).  Every lane holds the same row and forms the same action; the
// check is attemptConnect(s_existing = r, s = v[j]) at depth 0
// (rrt_connect.cpp:20-75), star_row's rewire form: the action leads from r to
// v[j] (FORWARD) or from v[j] to r (REVERSE), and the pair check starts from r
// in both.  flags as gbp_validate's (no s_new / t_new kept).
template <class ZT, bool ADAPTIVE, int CM>
__global__ __launch_bounds__(TB) void k_graft_check(TerrainView<ZT> T, const double *__restrict__ tv,
                                                    int32_t n, GraftRoot R, double radius, int dir,
                                                    uint8_t *__restrict__ attach,
                                                    double *__restrict__ actions,
                                                    uint32_t *__restrict__ flags) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int64_t nw = (int64_t)gridDim.x * blockDim.x / WAVE;
  double r[8];
  copy8(r, R.s);
  for (int64_t j = wv; j < n; j += nw) {
    double sj[8], a[10];
    copy8(sj, tv + 8 * j);
    uint32_t f = 0;
    bool ok = false;
    if (pose_distance(r, sj) <= radius) {  // (NaN: no candidate)
      f = GBP_F_GRAFT_CANDIDATE;
      const double t_s = pose_distance(sj, r) / V_NOM;
      if (t_s > KINEMATICS_RES) {  // :23-24
        connect_action(dir == GBP_FORWARD ? r : sj, dir == GBP_FORWARD ? sj : r, t_s, a);
        if (is_valid_action(a)) {  // :66
          double sn[8], tn = 0;
          uint32_t pf = 0;
          ok = wave_pair_check<ZT, ADAPTIVE, CM>(T, r, a, dir, sn, tn, pf);  // :74
          f |= pf | GBP_F_GRAFT_CHECKED;
        }
      }
    }
    if (lane == 0) {
      attach[j] = ok ? 1 : 0;
      flags[j] = f;
      if (f & GBP_F_GRAFT_CHECKED) copy10(actions + 10 * j, a);
    }
  }
}

template <class ZT>
int graft_check_launch(gbp_terrain *t, const gbp_tree *tree, int64_t n, const double *root,
                       double radius, int direction, int adaptive, uint8_t *attach, double *actions,
                       uint32_t *flags, hipStream_t s) {
  const TerrainView<ZT> V = view<ZT>(t);
  const int cm = (t->opt_affine && t->affine) ? 2 : 0;
  GraftRoot R;
  std::copy(root, root + 8, R.s);
  const int64_t g = std::max<int64_t>(1, std::min<int64_t>((int64_t)t->num_cus * GBP_GRAFT_GC,
                                                           (n + TB / WAVE - 1) / (TB / WAVE)));
  with_adaptive_cm(adaptive != 0, cm, [&](auto ad, auto c) {
    hipLaunchKernelGGL((k_graft_check<ZT, decltype(ad)::value, decltype(c)::value>), dim3((unsigned)g),
                       dim3(TB), 0, s, V, tree->v, (int32_t)n, R, radius, direction, attach, actions,
                       flags);
  });
  return hipGetLastError() == hipSuccess ? GBP_OK : GBP_E_HIP;
}

}  // namespace

extern "C" {

int gbp_tree_graft_check_dev(gbp_terrain *t, gbp_tree *tree, int64_t n, const double *root,
                             double radius, int direction, int adaptive, uint8_t *attach,
                             double *actions, uint32_t *flags, gbp_stream stream) {
  if (!t || !tree_ok(tree)) return GBP_E_BAD_HANDLE;
  if (n < 1 || !root || !attach || !actions || !flags) return GBP_E_INVALID_ARG;
  if (direction != GBP_FORWARD && direction != GBP_REVERSE) return GBP_E_INVALID_ARG;
  if (!(radius >= 0.0)) return GBP_E_INVALID_ARG;
  for (int k = 0; k < 8; k++)
    if (std::isnan(root[k])) return GBP_E_INVALID_ARG;
  if (n > tree->cap) return GBP_E_SHAPE;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GBP_E_NO_DEVICE;
  if (!t->d_z) return GBP_E_BAD_HANDLE;
  if (t->device != tree->device) return GBP_E_INVALID_ARG;
  int64_t have = 0;
  const int rc = gbp_tree_size(tree, &have, stream);  // synchronises
  if (rc) return rc;
  if (have != n) return GBP_E_SHAPE;
  DeviceGuard g(tree->device);
  hipStream_t s = (hipStream_t)stream;
  return t->storage == GBP_STORAGE_F32
             ? graft_check_launch<float>(t, tree, n, root, radius, direction, adaptive, attach, actions,
                                         flags, s)
             : graft_check_launch<double>(t, tree, n, root, radius, direction, adaptive, attach,
                                          actions, flags, s);
}

}  // extern "C"
