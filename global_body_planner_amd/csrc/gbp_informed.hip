// gbp_informed.hip — informed sampling's entries (gbp.h gbp_informed): the
// handle's ellipse and the target sampler that draws inside it.  The ellipse
// itself is host/gbp_informed.cpp's; the draw is gbp_device.h's
// sample_state_informed_cfg_try, which the planner loop's
// k_targets_informed (gbp_plan.hip) calls as well.
#include <cmath>
#include <cstring>

#include "gbp_internal.h"

using namespace gbp;

namespace {

// s_from / s_to of the direction-biased draws, by value
struct DirPair {
  double from[8], to[8];
};

// one lane per draw, grid-stride: index i of the stream, one try
template <class ZT>
__global__ __launch_bounds__(TB) void k_sample_informed(TerrainView<ZT> T, int64_t n, uint64_t seed,
                                                        uint64_t stream_id, int64_t index_base,
                                                        double *__restrict__ states,
                                                        gbp_sampling cfg, gbp_informed inf,
                                                        DirPair dp) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    double q[8];
    sample_state_informed_cfg_try(T, cfg, inf, dp.from, dp.to, seed, stream_id, index_base + i, 0,
                                  q);
    copy8(states + 8 * i, q);
  }
}

bool handle_ok(const gbp_terrain *t) { return t != nullptr && t->d_z != nullptr; }

// what the draw reads of an active ellipse is a number
bool informed_ok(const gbp_informed &e) {
  if (!e.active) return true;
  return !(std::isnan(e.cx) || std::isnan(e.cy) || std::isnan(e.ux) || std::isnan(e.uy) ||
           std::isnan(e.a) || std::isnan(e.b)) &&
         e.a >= 0 && e.b >= 0;
}

}  // namespace

extern "C" {

int gbp_terrain_set_informed(gbp_terrain *t, const gbp_informed *inf) {
  if (!handle_ok(t)) return GBP_E_BAD_HANDLE;
  if (inf && !informed_ok(*inf)) return GBP_E_INVALID_ARG;
  t->informed = inf ? *inf : gbp_informed{};
  return GBP_OK;
}

int gbp_terrain_get_informed(const gbp_terrain *t, gbp_informed *inf) {
  if (!handle_ok(t)) return GBP_E_BAD_HANDLE;
  if (!inf) return GBP_E_INVALID_ARG;
  *inf = t->informed;
  return GBP_OK;
}

int gbp_sample_states_informed_dev(gbp_terrain *t, int64_t n, uint64_t seed, uint64_t stream_id,
                                   int64_t index_base, const gbp_sampling *cfg,
                                   const gbp_informed *inf, const double *s_from,
                                   const double *s_to, double *states, gbp_stream stream) {
  if (!handle_ok(t)) return GBP_E_BAD_HANDLE;
  const gbp_sampling c = cfg ? *cfg : t->sampling;
  const gbp_informed e = inf ? *inf : t->informed;
  if (n < 0 || (n > 0 && !states)) return GBP_E_INVALID_ARG;
  if (c.state_flag && (std::isnan(c.state_p) || !s_from || !s_to)) return GBP_E_INVALID_ARG;
  if (!informed_ok(e)) return GBP_E_INVALID_ARG;
  if (n == 0) return GBP_OK;
  DirPair dp{};
  if (s_from) memcpy(dp.from, s_from, sizeof dp.from);
  if (s_to) memcpy(dp.to, s_to, sizeof dp.to);
  DeviceGuard g(t->device);
  const unsigned grid = grid_for(n, TB, t->num_cus * 16);  // the samplers' capped grid
  if (t->storage == GBP_STORAGE_F32)
    hipLaunchKernelGGL(k_sample_informed<float>, dim3(grid), dim3(TB), 0, (hipStream_t)stream,
                       view<float>(t), n, seed, stream_id, index_base, states, c, e, dp);
  else
    hipLaunchKernelGGL(k_sample_informed<double>, dim3(grid), dim3(TB), 0, (hipStream_t)stream,
                       view<double>(t), n, seed, stream_id, index_base, states, c, e, dp);
  HIPCHK(hipGetLastError());
  return GBP_OK;
}

int gbp_sample_states_informed_host(gbp_terrain *t, int64_t n, uint64_t seed, uint64_t stream_id,
                                    int64_t index_base, const gbp_sampling *cfg,
                                    const gbp_informed *inf, const double *s_from,
                                    const double *s_to, double *states) {
  if (!handle_ok(t)) return GBP_E_BAD_HANDLE;
  if (n <= 0) return n == 0 ? GBP_OK : GBP_E_INVALID_ARG;
  if (!states) return GBP_E_INVALID_ARG;
  DeviceGuard g(t->device);
  hipStream_t st = t->host_stream;
  // the handle's grow-only workspace, as the other _host samplers stage theirs
  int rc = ensure_ws(&t->ws, &t->ws_bytes, (size_t)n * 64);
  if (rc) return rc;
  double *ds = (double *)t->ws;
  rc = gbp_sample_states_informed_dev(t, n, seed, stream_id, index_base, cfg, inf, s_from, s_to,
                                      ds, st);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(states, ds, (size_t)n * 64, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return GBP_OK;
}

}  // extern "C"
