// gbp_slopes.hip — a terrain handle's slope layers derived from its heights on
// the device (gbp_terrain_derive_slopes_dev / _host, gbp_terrain_read_slopes_host)
// and the launch gbp_terrain.hip's upkeep under GBP_OPT_DERIVE_SLOPES calls.  The
// rule is gbp_slopes.h's.  A translation unit of its own: no other unit's device
// code depends on it.
//
// k_derive_slopes is a streaming stencil, one thread per node of the launch
// rectangle, lanes along iy.  Heights come from the x-pairs (gbp_device.h
// TerrainView): pair (ix, iy) holds z[ix][iy] and z[ix + 1][iy], one load; z[ix -
// 1][iy] is slot 0 of pair ix - 1; row nx - 1 has no pair of its own and reads
// both from pair nx - 2.  The y neighbours are slot reads of pairs (ix, iy -+ 1),
// which the neighbouring lanes load as their own centre.  Each layer is written
// with one 8-byte store a lane, consecutive lanes consecutive addresses.  No
// atomics, no LDS.  The grid is 1-D over (row, 256-lane column block): no cap,
// no stride.

#include "gbp_internal.h"
#include "gbp_slopes.h"

namespace {

constexpr int SLOPES_BLOCK = 256;

struct SlopeArgs {
  const void *zp;       // x-pairs
  const double *x, *y;  // coordinates [NX], [NY]
  double *lay[3];       // dx, dy, dz [NX][NY]
  int NX, NY;
  int lx0, ly0, lnx, lny;  // the launch rectangle: every node of it is written
  int ix0, iy0, ix1, iy1;  // derived inside [ix0, ix1) x [iy0, iy1), (0, 0, 1) outside
  int nyb;                 // column blocks per row
  int flags;
  const int32_t *status;  // null, or an update's check word: 1 = write nothing
};

template <class ZT>
struct Pair2;
template <>
struct Pair2<float> {
  using type = float2;
};
template <>
struct Pair2<double> {
  using type = double2;
};

// z[ix][iy] from slot 0 of pair ix, row NX - 1 from slot 1 of pair NX - 2
template <class ZT>
__device__ __forceinline__ double z_at(const ZT *zp, int NX, int NY, int ix, int iy) {
  const int p = ix < NX - 1 ? ix : NX - 2;
  return (double)zp[2 * ((int64_t)p * NY + iy) + (ix < NX - 1 ? 0 : 1)];
}

template <class ZT>
__global__ __launch_bounds__(SLOPES_BLOCK) void k_derive_slopes(const SlopeArgs A) {
  using P = typename Pair2<ZT>::type;
  if (A.status && *A.status) return;  // the update was rejected: heights and layers stay
  const int row = (int)(blockIdx.x / (unsigned)A.nyb);
  const int j = ((int)blockIdx.x - row * A.nyb) * SLOPES_BLOCK + (int)threadIdx.x;
  if (j >= A.lny) return;
  const int ix = A.lx0 + row, iy = A.ly0 + j;
  const int64_t cell = (int64_t)ix * A.NY + iy;
  double n[3] = {0.0, 0.0, 1.0};
  if (ix >= A.ix0 && ix < A.ix1 && iy >= A.iy0 && iy < A.iy1) {
    const ZT *zp = (const ZT *)A.zp;
    const bool xm = ix > 0, xp = ix + 1 < A.NX, ym = iy > 0, yp = iy + 1 < A.NY;
    double zc, zxm = 0.0, zxp = 0.0;
    if (xp) {
      const P v = *(const P *)(zp + 2 * cell);
      zc = (double)v.x;
      zxp = (double)v.y;
      if (xm) zxm = (double)zp[2 * (cell - A.NY)];
    } else {  // ix = NX - 1 >= 1: pair NX - 2 holds z[NX - 2] and z[NX - 1]
      const P v = *(const P *)(zp + 2 * (cell - A.NY));
      zxm = (double)v.x;
      zc = (double)v.y;
    }
    const double zym = ym ? z_at(zp, A.NX, A.NY, ix, iy - 1) : 0.0;
    const double zyp = yp ? z_at(zp, A.NX, A.NY, ix, iy + 1) : 0.0;
    const double gx = gbp::slope_gradient(xm, xp, zxm, zc, zxp, xm ? A.x[ix - 1] : 0.0, A.x[ix],
                                          xp ? A.x[ix + 1] : 0.0);
    const double gy = gbp::slope_gradient(ym, yp, zym, zc, zyp, ym ? A.y[iy - 1] : 0.0, A.y[iy],
                                          yp ? A.y[iy + 1] : 0.0);
    gbp::slope_normal(zc, gx, gy, A.flags, n);
  }
  A.lay[0][cell] = n[0];
  A.lay[1][cell] = n[1];
  A.lay[2][cell] = n[2];
}

bool valid_handle(const gbp_terrain *t) { return t != nullptr && t->d_z != nullptr; }

// `rows` runs of `width` bytes, `spitch` apart on the device, packed on the host
int read_rows(void *dst, const void *src, size_t width, size_t spitch, size_t rows, hipStream_t st) {
  if (spitch == width || rows == 1)
    HIPCHK(hipMemcpyAsync(dst, src, width * rows, hipMemcpyDeviceToHost, st));
  else
    HIPCHK(hipMemcpy2DAsync(dst, width, src, spitch, width, rows, hipMemcpyDeviceToHost, st));
  return GBP_OK;
}

}  // namespace

GBP_INTERNAL int gbp_internal_derive_slopes(const gbp_terrain *t, const void *zp, const double *x,
                                            const double *y, double *const lay[3],
                                            const gbp_patch::Rect &launch,
                                            const gbp_patch::Rect &inner, int flags,
                                            const int32_t *status, hipStream_t st) {
  SlopeArgs A;
  A.zp = zp;
  A.x = x;
  A.y = y;
  for (int k = 0; k < 3; k++) A.lay[k] = lay[k];
  A.NX = t->nx;
  A.NY = t->ny;
  A.lx0 = launch.ix0;
  A.ly0 = launch.iy0;
  A.lnx = launch.nx;
  A.lny = launch.ny;
  A.ix0 = inner.ix0;
  A.iy0 = inner.iy0;
  A.ix1 = inner.ix0 + inner.nx;
  A.iy1 = inner.iy0 + inner.ny;
  A.nyb = (launch.ny + SLOPES_BLOCK - 1) / SLOPES_BLOCK;
  A.flags = flags;
  A.status = status;
  const int64_t blocks = (int64_t)launch.nx * A.nyb;
  if (blocks < 1 || blocks > 0x7fffffffLL) return GBP_E_SHAPE;
  if (t->storage == GBP_STORAGE_F32)
    k_derive_slopes<float><<<(unsigned)blocks, SLOPES_BLOCK, 0, st>>>(A);
  else
    k_derive_slopes<double><<<(unsigned)blocks, SLOPES_BLOCK, 0, st>>>(A);
  HIPCHK(hipGetLastError());
  return GBP_OK;
}

extern "C" {

int gbp_terrain_derive_slopes_dev(gbp_terrain *t, const gbp_rect *r, int flags, gbp_stream stream) {
  if (!valid_handle(t)) return GBP_E_BAD_HANDLE;
  gbp_patch::Rect q;
  int rc = gbp_patch::resolve_rect(t->nx, t->ny, r, &q);
  if (rc) return rc;
  if ((flags & ~GBP_SLOPES_F32) || !t->d_dx) return GBP_E_INVALID_ARG;
  DeviceGuard g(t->device);
  double *const lay[3] = {t->d_dx, t->d_dy, t->d_dz};
  return gbp_internal_derive_slopes(t, t->d_z, t->d_x, t->d_y, lay, q, q, flags, nullptr,
                                    (hipStream_t)stream);
}

int gbp_terrain_derive_slopes_host(gbp_terrain *t, const gbp_rect *r, int flags) {
  if (!valid_handle(t)) return GBP_E_BAD_HANDLE;
  gbp_patch::Rect q;
  int rc = gbp_patch::resolve_rect(t->nx, t->ny, r, &q);
  if (rc) return rc;
  if (flags & ~GBP_SLOPES_F32) return GBP_E_INVALID_ARG;
  DeviceGuard g(t->device);
  hipStream_t st = t->host_stream;
  for (auto &u : t->pending) HIPCHK(hipStreamWaitEvent(st, u.done, 0));
  if (t->d_dx) {
    double *const lay[3] = {t->d_dx, t->d_dy, t->d_dz};
    if ((rc = gbp_internal_derive_slopes(t, t->d_z, t->d_x, t->d_y, lay, q, q, flags, nullptr, st)))
      return rc;
    HIPCHK(hipStreamSynchronize(st));
    return GBP_OK;
  }
  // a handle created without layers: new ones, (0, 0, 1) outside the
  // rectangle, the handle's only once the launch is through
  struct Fresh {
    double *lay[3] = {nullptr, nullptr, nullptr};
    ~Fresh() {
      for (double *p : lay)
        if (p) (void)hipFree(p);
    }
  } fresh;
  const size_t cells = (size_t)t->nx * t->ny;
  for (int k = 0; k < 3; k++)
    if (hipMalloc((void **)&fresh.lay[k], cells * sizeof(double)) != hipSuccess) {
      fresh.lay[k] = nullptr;
      return GBP_E_ALLOC;
    }
  gbp_patch::Rect whole;
  whole.nx = t->nx;
  whole.ny = t->ny;
  if ((rc = gbp_internal_derive_slopes(t, t->d_z, t->d_x, t->d_y, fresh.lay, whole, q, flags, nullptr,
                                       st))) {
    (void)hipStreamSynchronize(st);  // nothing in flight when the buffers go
    return rc;
  }
  HIPCHK(hipStreamSynchronize(st));
  std::swap(t->d_dx, fresh.lay[0]);
  std::swap(t->d_dy, fresh.lay[1]);
  std::swap(t->d_dz, fresh.lay[2]);
  return GBP_OK;
}

int gbp_terrain_read_slopes_host(gbp_terrain *t, const gbp_rect *r, double *dx, double *dy,
                                 double *dz) {
  if (!valid_handle(t)) return GBP_E_BAD_HANDLE;
  gbp_patch::Rect q;
  int rc = gbp_patch::resolve_rect(t->nx, t->ny, r, &q);
  if (rc) return rc;
  if (!dx || !dy || !dz || !t->d_dx) return GBP_E_INVALID_ARG;
  DeviceGuard g(t->device);
  hipStream_t st = t->host_stream;
  for (auto &u : t->pending) HIPCHK(hipStreamWaitEvent(st, u.done, 0));
  const double *lay[3] = {t->d_dx, t->d_dy, t->d_dz};
  double *out[3] = {dx, dy, dz};
  for (int k = 0; k < 3; k++)
    if ((rc = read_rows(out[k], lay[k] + (size_t)q.ix0 * t->ny + q.iy0, (size_t)q.ny * sizeof(double),
                        (size_t)t->ny * sizeof(double), (size_t)q.nx, st))) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
  HIPCHK(hipStreamSynchronize(st));
  return GBP_OK;
}

}  // extern "C"
