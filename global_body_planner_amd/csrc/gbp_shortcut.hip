// gbp_shortcut.hip — the connect decisions of postProcessPath for found paths
// (rrt_connect.cpp:139-227): one launch decides every pair of every path of a
// call (k_shortcut_pairs, gbp_shortcut_table_dev) and the host replays the
// walk over the table (gbp_shortcut_paths_host, host/gbp_shortcut_walk.cpp).
// Touches no planner workspace and no tree; the pair check by a whole wave it
// shares with the planner's connects: gbp_plan_dev.h.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "gbp.h"
#include "gbp_device.h"
#include "gbp_internal.h"
#include "gbp_plan_dev.h"
#include "host/gbp_shortcut_walk.h"

using namespace gbp;

namespace {

// ============================================================================
// RRTConnectClass::postProcessPath's connect decisions (rrt_connect.cpp:139-227)
// ============================================================================
// The walk asks attemptConnect(state[i], state[j], FORWARD) == REACHED for
// pairs i < j of a found path; the answer depends on the two states and the
// terrain alone, so one launch decides every pair of every path of the call
// and the host replays the walk over the table (host/gbp_shortcut_walk.cpp).
// REACHED is the recursion's depth 0: t_s > KINEMATICS_RES, a valid connect
// action and a valid pair check.  Path p of n states holds its pairs packed
// row-major over the upper triangle from pair_off[p]:
//   item(i, j) = pair_off[p] + i (2n - i - 1) / 2 + (j - i - 1).
constexpr int SC_MAXP = 64;  // paths per launch (their offsets travel as the kernel's argument)
struct ShortcutPaths {
  int32_t n;                       // paths of this launch
  int64_t path_off[SC_MAXP + 1];   // first state of path p (rows of `states`)
  int64_t pair_off[SC_MAXP + 1];   // first item of path p
};
// (GBP_SHORTCUT_GC, k_shortcut_pairs' workgroups per CU: gbp_plan_dev.h)
#ifndef GBP_SHORTCUT_ORDER
// 1: a path's longest spans first; 0: as packed.  Measured on the 5,886-pair
// table: 120 µs against 131 µs median (profiles/shortcut_ab.txt)
#define GBP_SHORTCUT_ORDER 1
#endif

// the largest m with m (m - 1) / 2 <= k (k >= 0): sqrt's guess, settled on integers
__device__ __forceinline__ int64_t tri_root(int64_t k) {
  int64_t m = (int64_t)((1.0 + sqrt(1.0 + 8.0 * (double)k)) * 0.5);
  while (m * (m - 1) / 2 > k) m--;
  while ((m + 1) * m / 2 <= k) m++;
  return m;
}

// one wave per pair, grid-stride over the launch's pairs.  order 0 takes a
// path's pairs as they are packed; order 1 by span j - i, longest first (their
// pair checks run the most 64-sample steps) — the outputs are the same.
template <class ZT, bool ADAPTIVE, int CM>
__global__ __launch_bounds__(TB) void k_shortcut_pairs(TerrainView<ZT> T, ShortcutPaths P,
                                                       const double *__restrict__ states,
                                                       int order, uint8_t *__restrict__ reached,
                                                       uint32_t *__restrict__ flags) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / WAVE);
  const int64_t first = P.pair_off[0], total = P.pair_off[P.n] - first;
  for (int64_t w = blockIdx.x * (int64_t)(blockDim.x / WAVE) + threadIdx.x / WAVE; w < total;
       w += waves) {
    int p = 0;
    while (P.pair_off[p + 1] - first <= w) p++;  // w < total: ends at p < P.n
    const int64_t n = P.path_off[p + 1] - P.path_off[p];
    const int64_t k = w - (P.pair_off[p] - first);  // 0 <= k < n (n - 1) / 2
    int64_t i, j;
    if (order == 0) {
      // row i from the end: rows n-2, n-3, ... hold 1, 2, ... pairs
      const int64_t r = n * (n - 1) / 2 - 1 - k;  // pairs after this one
      const int64_t m = tri_root(r);               // rows after row i hold m (m - 1) / 2 <= r
      i = n - 1 - m;
      j = n - 1 - (r - m * (m - 1) / 2);
    } else {
      // spans n-1, n-2, ... hold 1, 2, ... pairs
      const int64_t m = tri_root(k);
      i = k - m * (m - 1) / 2;
      j = i + (n - m);
    }
    const int64_t item = P.pair_off[p] + i * (2 * n - i - 1) / 2 + (j - i - 1);
    double si[8], sj[8], an[10];
    copy8(si, states + 8 * (P.path_off[p] + i));
    copy8(sj, states + 8 * (P.path_off[p] + j));
    const double t_s = pose_distance(sj, si) / V_NOM;  // rrt_connect.cpp:89
    bool ok = false;
    uint32_t cf = 0;
    if (!(t_s <= KINEMATICS_RES)) {  // :23-24
      connect_action(si, sj, t_s, an);
      if (is_valid_action(an)) {  // :66
        double psn[8], ptn = 0;
        uint32_t pf = 0;
        ok = wave_pair_check<ZT, ADAPTIVE, CM>(T, si, an, GBP_FORWARD, psn, ptn, pf);  // :74
        cf = pf & (GBP_F_OOD | GBP_F_NAN | GBP_F_FRAGILE | GBP_F_LIMIT);
      }
    }
    if (lane == 0) {
      reached[item] = ok ? 1 : 0;
      flags[item] = cf;
    }
  }
}

// the argument checks of the shortcut entries, before any device work: path p
// is the states [path_off[p], path_off[p + 1]), at least two of them, path_off[0] = 0
int shortcut_args(const gbp_terrain *t, int64_t n_paths, const int64_t *path_off, bool arrays) {
  if (!t) return GBP_E_BAD_HANDLE;
  if (n_paths < 0) return GBP_E_INVALID_ARG;
  if (n_paths == 0) return GBP_OK;
  if (!path_off || !arrays || path_off[0] != 0) return GBP_E_INVALID_ARG;
  for (int64_t p = 0; p < n_paths; p++)
    if (path_off[p + 1] - path_off[p] < 2) return GBP_E_INVALID_ARG;
  return GBP_OK;
}

// the pairs of paths [p0, p0 + SC_MAXP) per launch, all of them for a call of
// up to SC_MAXP paths; pair_off[p] counted from the call's first path
template <class ZT>
int shortcut_launch(gbp_terrain *t, int64_t n_paths, const int64_t *path_off, const double *states,
                    int adaptive, uint8_t *reached, uint32_t *flags, hipStream_t s) {
  const TerrainView<ZT> V = view<ZT>(t);
  const int cm = (t->opt_affine && t->affine) ? 2 : 0;
  int64_t grid_env = 0;  // tests: a tiny grid gives every wave many items
  if (const char *e = getenv("GBP_SHORTCUT_GRID")) grid_env = atoll(e);
  int order = GBP_SHORTCUT_ORDER;  // A/B: tools/shortcut_ab.py
  if (const char *e = getenv("GBP_SHORTCUT_ORDER")) order = atoi(e) != 0;
  int64_t item0 = 0;
  for (int64_t p0 = 0; p0 < n_paths; p0 += SC_MAXP) {
    ShortcutPaths P;
    P.n = (int32_t)std::min<int64_t>(SC_MAXP, n_paths - p0);
    for (int q = 0; q <= SC_MAXP; q++) {  // the unused tail repeats the end
      const int64_t p = p0 + std::min<int64_t>(q, P.n);
      P.path_off[q] = path_off[p];
      if (q > 0 && q <= P.n) {
        const int64_t n = path_off[p] - path_off[p - 1];
        item0 += n * (n - 1) / 2;
      }
      P.pair_off[q] = item0;
    }
    const int64_t items = P.pair_off[P.n] - P.pair_off[0];
    int64_t g = std::min<int64_t>((int64_t)t->num_cus * GBP_SHORTCUT_GC, (items + 3) / 4);
    if (grid_env > 0) g = std::min(g, grid_env);
    with_adaptive_cm(adaptive != 0, cm, [&](auto ad, auto c) {
      hipLaunchKernelGGL((k_shortcut_pairs<ZT, decltype(ad)::value, decltype(c)::value>),
                         dim3((unsigned)std::max<int64_t>(1, g)), dim3(TB), 0, s, V, P, states, order,
                         reached, flags);
    });
  }
  return hipGetLastError() == hipSuccess ? GBP_OK : GBP_E_HIP;
}

}  // namespace

extern "C" {

int gbp_shortcut_table_dev(gbp_terrain *t, int64_t n_paths, const int64_t *path_off,
                           const double *states, int adaptive, uint8_t *reached, uint32_t *flags,
                           gbp_stream stream) {
  const int rc = shortcut_args(t, n_paths, path_off, states && reached && flags);
  if (rc || n_paths == 0) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GBP_E_NO_DEVICE;
  if (!t->d_z) return GBP_E_BAD_HANDLE;
  DeviceGuard g(t->device);
  hipStream_t s = (hipStream_t)stream;
  return t->storage == GBP_STORAGE_F32
             ? shortcut_launch<float>(t, n_paths, path_off, states, adaptive, reached, flags, s)
             : shortcut_launch<double>(t, n_paths, path_off, states, adaptive, reached, flags, s);
}

int gbp_shortcut_paths_host(gbp_terrain *t, int64_t n_paths, const int64_t *path_off,
                            const double *states, const double *actions, int adaptive,
                            int cost_add_yaw_flag, double length_weight, double yaw_weight,
                            int64_t *out_off, double *out_states, double *out_actions,
                            double *path_length, double *path_yaw, double *path_cost,
                            int64_t *n_resolved) {
  int rc = shortcut_args(t, n_paths, path_off,
                         states && actions && out_off && out_states && out_actions &&
                             path_length && path_yaw && path_cost);
  if (n_resolved) *n_resolved = 0;
  if (rc || n_paths == 0) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GBP_E_NO_DEVICE;
  if (!t->d_z) return GBP_E_BAD_HANDLE;
  DeviceGuard g(t->device);
  hipStream_t s = t->host_stream;
  const int64_t total = path_off[n_paths];
  int64_t items = 0;
  for (int64_t p = 0; p < n_paths; p++)
    items += gbp_shortcut::pair_count(path_off[p + 1] - path_off[p]);
  // the table's two arrays back to back: one read-back
  const size_t fl_at = ((size_t)items + 255) & ~(size_t)255;
  const size_t tab_bytes = fl_at + (size_t)items * sizeof(uint32_t);
  DevBuf buf;
  double *ds;
  uint8_t *dtab;
  rc = stage_buf(buf, [&](Stage &S) { S.take(ds, 8 * total); S.take(dtab, tab_bytes); });
  if (rc) return rc;
  if ((rc = h2d(ds, states, 8 * total, s))) return rc;
  rc = gbp_shortcut_table_dev(t, n_paths, path_off, ds, adaptive, dtab, (uint32_t *)(dtab + fl_at), s);
  if (rc) return rc;
  std::vector<uint8_t> tab(tab_bytes);
  if ((rc = d2h(tab.data(), dtab, tab_bytes, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  uint8_t *reached = tab.data();
  const uint32_t *fl = (const uint32_t *)(tab.data() + fl_at);
  const gbp_host::Terrain *H = host_mirror(t);
  if (!H) return GBP_E_HIP;
  const gbp_shortcut::CostWeights cw{cost_add_yaw_flag, length_weight, yaw_weight};
  int64_t item = 0, resolved = 0, kept = 0;
  for (int64_t p = 0; p < n_paths; p++) {
    const int64_t n = path_off[p + 1] - path_off[p];
    const double *ps = states + 8 * path_off[p];
    // the FRAGILE pairs again with glibc (host/gbp_host_check.cpp): the depth-0
    // level of attemptConnect(state[i], state[j], FORWARD), rrt_connect.cpp:20-91
    for (int64_t i = 0; i < n; i++)
      for (int64_t j = i + 1; j < n; j++) {
        const int64_t it = item + gbp_shortcut::pair_index(n, i, j);
        if (!(fl[it] & GBP_F_FRAGILE)) continue;
        const double *si = ps + 8 * i, *sj = ps + 8 * j;
        const double t_s = gbp_host::pose_distance(sj, si) / V_NOM;
        bool ok = false;
        double an[10], sn[8], tn = 0;
        uint32_t f = 0;
        if (!(t_s <= KINEMATICS_RES)) {
          gbp_host::connect_action(si, sj, t_s, an);
          if (gbp_host::is_valid_action(an))
            ok = gbp_host::pair_check(*H, si, an, GBP_FORWARD, adaptive, sn, &tn, &f, nullptr);
        }
        reached[it] = ok ? 1 : 0;
        resolved++;
      }
    // a path's n - 1 edge actions follow those of the paths before it, in and out
    out_off[p] = kept;
    const int64_t m = gbp_shortcut::walk(n, ps, actions + 10 * (path_off[p] - p), reached + item, cw,
                                         out_states + 8 * kept, out_actions + 10 * (kept - p),
                                         path_length + p, path_yaw + p, path_cost + p);
    if (m < 0) return GBP_E_INVALID_ARG;
    kept += m;
    item += gbp_shortcut::pair_count(n);
  }
  out_off[n_paths] = kept;
  if (n_resolved) *n_resolved = resolved;
  return GBP_OK;
}

}  // extern "C"
