// gbp_terrain.hip — a terrain handle's heights updated in place
// (gbp_terrain_update_dev / _host, gbp_terrain_read_host) and the lazy host
// mirror behind host_mirror (gbp_internal.h).  A translation unit of its own:
// the objects of gbp_engine.hip and gbp_plan.hip do not depend on it.
//
// Heights lie in HBM as x-pairs (gbp_device.h TerrainView): zp[2 (ix ny + iy)
// + {0, 1}] = z[ix][iy], z[ix + 1][iy] for ix < nx - 1, so a cell's height is
// held by slot 0 of pair row ix and by slot 1 of pair row ix - 1.  The patch
// kernel is output-centric: one thread per (pair row, iy) writes the slots of
// that pair the rectangle covers, both in one 2-element store, a single slot
// at the rectangle's first and last pair row.  No two threads write one
// address.  The engine-free index rules are host/gbp_terrain_patch.{h,cpp}.
//
// gbp_terrain_move_host moves the handle's window by whole cells: the shift
// kernel copies the overlap from the old x-pairs and slope layers into a second
// set of buffers (in place, one workgroup would overwrite pairs another has not
// read yet), the patch kernel writes the uncovered strips behind it on the same
// stream, and the buffers are swapped once both are through.

#include "gbp_internal.h"

namespace {

constexpr int PATCH_BLOCK = 256;
constexpr int PATCH_TILE = 64;  // GBP_SRC_F32_GRIDMAP: 64 x 64 outputs from a 64 x 65 tile

struct PatchArgs {
  void *zp;             // the handle's x-pairs
  double *lay[3];       // its slope layers [nx][ny]
  const void *src[4];   // z, dx, dy, dz in the source layout (dx..dz null: not given)
  int64_t ld, off;      // a cell's element = the layout's index (gbp_patch::src_index) - off
  int NX, NY;
  int ix0, iy0, pnx, pny;
  int r0, r1;           // rows [r0, r1) = [max(ix0 - 1, 0), ix0 + pnx): pair rows of the
                        // heights (those below NX - 1), cell rows of the layers (from ix0)
  const int32_t *status;  // null, or the check launch's word: 1 = write nothing
};

template <class ZT>
struct Pair;
template <>
struct Pair<float> {
  using type = float2;
};
template <>
struct Pair<double> {
  using type = double2;
};

// gbp_patch::src_index on the device
template <int SRC>
__device__ __forceinline__ int64_t src_at(const PatchArgs &A, int ix, int iy) {
  return (SRC == GBP_SRC_F32_GRIDMAP
              ? (int64_t)(A.NX - 1 - ix) + (int64_t)(A.NY - 1 - iy) * A.ld
              : (int64_t)(ix - A.ix0) * A.ld + (int64_t)(iy - A.iy0)) -
         A.off;
}

// pair row p at iy: slot 0 = z[p][iy] when row p is in the rectangle, slot 1 =
// z[p + 1][iy] when row p + 1 is; the other slot keeps its value
template <class ZT>
__device__ __forceinline__ void put_pair(const PatchArgs &A, int p, int iy, bool lo, bool hi,
                                         double v0, double v1) {
  ZT *q = (ZT *)A.zp + 2 * ((int64_t)p * A.NY + iy);
  if (lo && hi) {
    typename Pair<ZT>::type v;
    v.x = (ZT)v0;
    v.y = (ZT)v1;
    *(typename Pair<ZT>::type *)q = v;
  } else if (lo) {
    q[0] = (ZT)v0;
  } else if (hi) {
    q[1] = (ZT)v1;
  }
}

// blockIdx.z = 0: the heights; 1..3: slope layer dx / dy / dz (launched only
// when given).  GBP_SRC_F64_XMAJOR: lanes along iy on both sides, rows by
// blockIdx.y.  GBP_SRC_F32_GRIDMAP is contiguous along x and reversed on both
// axes, the destination contiguous along y: a workgroup loads rows [rt, rt +
// 65) x 64 columns with lanes along x into LDS (pitch 65: the transposed read
// is conflict-free), then writes 64 pair rows with lanes along y.
template <class ZT, int SRC>
__global__ __launch_bounds__(PATCH_BLOCK) void k_terrain_patch(const PatchArgs A) {
  if (A.status && *A.status) return;  // rejected by k_terrain_check
  const int which = blockIdx.z;
  const int xe = A.ix0 + A.pnx, ye = A.iy0 + A.pny;
  if constexpr (SRC == GBP_SRC_F32_GRIDMAP) {
    __shared__ float tile[PATCH_TILE][PATCH_TILE + 1];
    const float *src = (const float *)A.src[which];
    const int rt = A.r0 + (int)blockIdx.y * PATCH_TILE, jt = A.iy0 + (int)blockIdx.x * PATCH_TILE;
    for (int e = threadIdx.x; e < PATCH_TILE * (PATCH_TILE + 1); e += PATCH_BLOCK) {
      const int li = e % (PATCH_TILE + 1), lj = e / (PATCH_TILE + 1);
      const int ix = rt + li, iy = jt + lj;
      if (ix >= A.ix0 && ix < xe && iy < ye) tile[lj][li] = src[src_at<SRC>(A, ix, iy)];
    }
    __syncthreads();
    const int lj = threadIdx.x % PATCH_TILE, iy = jt + lj;
    if (iy >= ye) return;
    for (int li = threadIdx.x / PATCH_TILE; li < PATCH_TILE; li += PATCH_BLOCK / PATCH_TILE) {
      const int r = rt + li;
      if (r >= A.r1) break;
      if (which == 0) {
        if (r >= A.NX - 1) break;
        const bool lo = r >= A.ix0, hi = r + 1 < xe;
        put_pair<ZT>(A, r, iy, lo, hi, lo ? (double)tile[lj][li] : 0.0,
                     hi ? (double)tile[lj][li + 1] : 0.0);
      } else if (r >= A.ix0) {
        A.lay[which - 1][(int64_t)r * A.NY + iy] = (double)tile[lj][li];
      }
    }
  } else {
    const double *src = (const double *)A.src[which];
    const int iy = A.iy0 + (int)(blockIdx.x * PATCH_BLOCK + threadIdx.x);
    if (iy >= ye) return;
    for (int r = A.r0 + (int)blockIdx.y; r < A.r1; r += (int)gridDim.y) {
      if (which == 0) {
        if (r >= A.NX - 1) break;
        const bool lo = r >= A.ix0, hi = r + 1 < xe;
        put_pair<ZT>(A, r, iy, lo, hi, lo ? src[src_at<SRC>(A, r, iy)] : 0.0,
                     hi ? src[src_at<SRC>(A, r + 1, iy)] : 0.0);
      } else if (r >= A.ix0) {
        A.lay[which - 1][(int64_t)r * A.NY + iy] = src[src_at<SRC>(A, r, iy)];
      }
    }
  }
}

// an fp64 patch for an fp32 handle: status[0] = 1 when a height is neither
// NaN nor float-representable (status[0] was zeroed on the stream before)
__global__ __launch_bounds__(PATCH_BLOCK) void k_terrain_check(const double *src, int64_t ld,
                                                               int pnx, int pny,
                                                               int32_t *status) {
  const int64_t n = (int64_t)pnx * pny;
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * PATCH_BLOCK + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * PATCH_BLOCK) {
    const double v = src[(e / pny) * ld + (e % pny)];
    bad |= !(v != v) && (double)(float)v != v;
  }
  if (bad) status[0] = 1;
}

// out[i][j] = z[ix0 + i][iy0 + j] from the chosen copy (gbp_terrain_read_host)
template <class ZT>
__global__ __launch_bounds__(PATCH_BLOCK) void k_terrain_read(const ZT *zp, double *out, int NX,
                                                              int NY, int ix0, int iy0, int rnx,
                                                              int rny, int copy) {
  const int j = (int)(blockIdx.x * PATCH_BLOCK + threadIdx.x);
  if (j >= rny) return;
  const int iy = iy0 + j;
  for (int i = blockIdx.y; i < rnx; i += (int)gridDim.y) {
    const int ix = ix0 + i;
    int p, slot;
    if (copy == 0) {
      p = ix < NX - 1 ? ix : NX - 2;
      slot = ix < NX - 1 ? 0 : 1;
    } else {
      p = ix > 0 ? ix - 1 : 0;
      slot = ix > 0 ? 1 : 0;
    }
    out[(int64_t)i * rny + j] = (double)zp[2 * ((int64_t)p * NY + iy) + slot];
  }
}

// ---- a window moved by whole cells (gbp_terrain_move_host) ---------------------
struct ShiftArgs {
  const void *zo;         // the old x-pairs
  void *zn;               // the new ones: another buffer
  const double *lo[3];    // the old slope layers [NX][NY] (null: the handle has none)
  double *ln[3];          // the new ones
  int NX, NY;
  int sx, sy;             // new cell (ix, iy) = old cell (ix + sx, iy + sy); |sx| < NX, |sy| < NY
};

constexpr int SHIFT_ROWS = 4;  // rows per thread and trip: their loads issue before the first store

// Output-centric over the new arrays, lanes along iy, rows by blockIdx.y.
// blockIdx.z = 0, the heights: new pair (p, iy) = old pair (p + sx, iy + sy),
// one 2-element load and one 2-element store (8 B a lane for fp32: sy makes
// the source no better aligned than that; 16 B for fp64).  At the seam rows the
// old pair row does not exist but one of its cells does: p + sx = -1 takes its
// slot 1 (old row 0) from slot 0 of old pair 0, p + sx = NX - 1 its slot 0 (old
// row NX - 1) from slot 1 of old pair NX - 2; the other slot is a strip cell and
// is the patch launch's, like every pair outside the overlap.
// blockIdx.z = 1..3, a slope layer: the overlap's cells shifted, every other
// cell (0, 0, 1), which a patch launch with layers then overwrites.
template <class ZT>
__global__ __launch_bounds__(PATCH_BLOCK) void k_terrain_shift(const ShiftArgs A) {
  using P = typename Pair<ZT>::type;
  const int iy = (int)(blockIdx.x * PATCH_BLOCK + threadIdx.x);
  if (iy >= A.NY) return;
  const int jy = iy + A.sy;
  const bool col = jy >= 0 && jy < A.NY;
  const int which = blockIdx.z;
  if (which == 0) {
    if (!col) return;
    const ZT *zo = (const ZT *)A.zo;
    ZT *zn = (ZT *)A.zn;
    const int np = A.NX - 1;
    for (int p0 = (int)blockIdx.y * SHIFT_ROWS; p0 < np; p0 += (int)gridDim.y * SHIFT_ROWS) {
      P v[SHIFT_ROWS];
#pragma unroll
      for (int k = 0; k < SHIFT_ROWS; k++) {
        const int q = p0 + k + A.sx;
        if (p0 + k < np && q >= 0 && q < np) v[k] = *(const P *)(zo + 2 * ((int64_t)q * A.NY + jy));
      }
#pragma unroll
      for (int k = 0; k < SHIFT_ROWS; k++) {
        const int p = p0 + k, q = p + A.sx;
        if (p >= np) break;
        ZT *d = zn + 2 * ((int64_t)p * A.NY + iy);
        if (q >= 0 && q < np)
          *(P *)d = v[k];
        else if (q == -1)
          d[1] = zo[2 * (int64_t)jy];  // old row 0: slot 0 of old pair 0
        else if (q == np)
          d[0] = zo[2 * ((int64_t)(np - 1) * A.NY + jy) + 1];  // old row NX - 1: slot 1 of pair NX - 2
      }
    }
  } else {
    const double *lo = A.lo[which - 1];
    double *ln = A.ln[which - 1];
    const double fill = which == 3 ? 1.0 : 0.0;
    for (int ix = blockIdx.y; ix < A.NX; ix += (int)gridDim.y) {
      const int jx = ix + A.sx;
      ln[(int64_t)ix * A.NY + iy] =
          col && jx >= 0 && jx < A.NX ? lo[(int64_t)jx * A.NY + jy] : fill;
    }
  }
}

bool valid_handle(const gbp_terrain *t) { return t != nullptr && t->d_z != nullptr; }

unsigned rows_grid(int rows) { return (unsigned)std::min(std::max(rows, 1), 65535); }

// the heights and slope layers a launch writes: the handle's own, or the
// second set a move fills
struct Dest {
  void *zp = nullptr;
  double *lay[3] = {nullptr, nullptr, nullptr};
};
Dest dest_of(const gbp_terrain *t) {
  Dest d;
  d.zp = t->d_z;
  d.lay[0] = t->d_dx;
  d.lay[1] = t->d_dy;
  d.lay[2] = t->d_dz;
  return d;
}

// the apply launch for a checked rectangle and source
int launch_patch(gbp_terrain *t, const Dest &D, const gbp_patch::Rect &q, int layout, int64_t ld,
                 int64_t off, const void *z, const void *dx, const void *dy, const void *dz,
                 const int32_t *status, hipStream_t st) {
  PatchArgs A;
  A.zp = D.zp;
  A.lay[0] = D.lay[0];
  A.lay[1] = D.lay[1];
  A.lay[2] = D.lay[2];
  A.src[0] = z;
  A.src[1] = dx;
  A.src[2] = dy;
  A.src[3] = dz;
  A.ld = ld;
  A.off = off;
  A.NX = t->nx;
  A.NY = t->ny;
  A.ix0 = q.ix0;
  A.iy0 = q.iy0;
  A.pnx = q.nx;
  A.pny = q.ny;
  A.r0 = std::max(q.ix0 - 1, 0);
  A.r1 = q.ix0 + q.nx;
  A.status = status;
  const int rows = A.r1 - A.r0;
  const unsigned nz = dx ? 4 : 1;
  const bool f32 = t->storage == GBP_STORAGE_F32;
  if (layout == GBP_SRC_F32_GRIDMAP) {
    const dim3 grid((unsigned)((q.ny + PATCH_TILE - 1) / PATCH_TILE),
                    (unsigned)((rows + PATCH_TILE - 1) / PATCH_TILE), nz);
    if (grid.y > 65535u) return GBP_E_SHAPE;
    if (f32)
      k_terrain_patch<float, GBP_SRC_F32_GRIDMAP><<<grid, PATCH_BLOCK, 0, st>>>(A);
    else
      k_terrain_patch<double, GBP_SRC_F32_GRIDMAP><<<grid, PATCH_BLOCK, 0, st>>>(A);
  } else {
    const dim3 grid((unsigned)((q.ny + PATCH_BLOCK - 1) / PATCH_BLOCK), rows_grid(rows), nz);
    if (f32)
      k_terrain_patch<float, GBP_SRC_F64_XMAJOR><<<grid, PATCH_BLOCK, 0, st>>>(A);
    else
      k_terrain_patch<double, GBP_SRC_F64_XMAJOR><<<grid, PATCH_BLOCK, 0, st>>>(A);
  }
  HIPCHK(hipGetLastError());
  return GBP_OK;
}

// the argument checks both entries share
int check_args(const gbp_terrain *t, const gbp_rect *r, int layout, int64_t ld, const void *z,
               const void *dx, const void *dy, const void *dz, gbp_patch::Rect *q) {
  int rc = gbp_patch::resolve_rect(t->nx, t->ny, r, q);
  if (rc) return rc;
  if ((rc = gbp_patch::check_source(layout, t->nx, *q, ld, z))) return rc;
  if ((dx == nullptr) != (dy == nullptr) || (dx == nullptr) != (dz == nullptr))
    return GBP_E_INVALID_ARG;
  if (dx && !t->d_dx) return GBP_E_INVALID_ARG;
  return GBP_OK;
}

// later work on the handle's host stream runs after every pending device update
int wait_pending(gbp_terrain *t) {
  for (auto &u : t->pending) HIPCHK(hipStreamWaitEvent(t->host_stream, u.done, 0));
  return GBP_OK;
}

// the rectangle's heights from the chosen copy into host out[q.nx][q.ny], on
// the host stream, synchronous
int read_rect(gbp_terrain *t, const gbp_patch::Rect &q, int copy, double *out) {
  hipStream_t st = t->host_stream;
  const size_t n = (size_t)q.nx * q.ny;
  DevBuf buf;
  double *d;
  int rc = stage_buf(buf, [&](Stage &S) { S.take(d, n); });
  if (rc) return rc;
  const dim3 grid((unsigned)((q.ny + PATCH_BLOCK - 1) / PATCH_BLOCK), rows_grid(q.nx));
  if (t->storage == GBP_STORAGE_F32)
    k_terrain_read<float><<<grid, PATCH_BLOCK, 0, st>>>((const float *)t->d_z, d, t->nx, t->ny,
                                                        q.ix0, q.iy0, q.nx, q.ny, copy);
  else
    k_terrain_read<double><<<grid, PATCH_BLOCK, 0, st>>>((const double *)t->d_z, d, t->nx, t->ny,
                                                         q.ix0, q.iy0, q.nx, q.ny, copy);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d, n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return GBP_OK;
}

// `rows` runs of `width` bytes, `spitch` apart in the host source, packed on the device
int stage_rows(void *dst, const void *src, size_t width, size_t spitch, size_t rows,
               hipStream_t st) {
  if (spitch == width || rows == 1)
    HIPCHK(hipMemcpyAsync(dst, src, width * rows, hipMemcpyHostToDevice, st));
  else
    HIPCHK(hipMemcpy2DAsync(dst, width, src, spitch, width, rows, hipMemcpyHostToDevice, st));
  return GBP_OK;
}

// Host sources of a checked rectangle staged and applied to D on st (not
// synchronised: buf holds the staged copies until the stream is through).  The
// rectangle's sub-block of each source array, packed: ld = its own width.
// GBP_SRC_F64_XMAJOR pointers address the rectangle's first cell.
int stage_patch(gbp_terrain *t, const Dest &D, const gbp_patch::Rect &q, int src_layout, int64_t ld,
                const void *z, const void *dx, const void *dy, const void *dz, DevBuf &buf,
                hipStream_t st) {
  const bool grid_map = src_layout == GBP_SRC_F32_GRIDMAP;
  const size_t esz = grid_map ? sizeof(float) : sizeof(double);
  const size_t cells = (size_t)q.nx * q.ny;
  const void *hsrc[4] = {z, dx, dy, dz};
  char *dsrc[4] = {nullptr, nullptr, nullptr, nullptr};
  const int nsrc = dx ? 4 : 1;
  int rc = stage_buf(buf, [&](Stage &S) {
    for (int k = 0; k < nsrc; k++) S.take(dsrc[k], cells * esz);
  });
  if (rc) return rc;
  // GBP_SRC_F32_GRIDMAP: source columns [a0, a0 + q.nx) of rows [b0, b0 + q.ny)
  const int64_t a0 = t->nx - q.ix0 - q.nx, b0 = t->ny - q.iy0 - q.ny;
  const int64_t sld = grid_map ? q.nx : q.ny, off = grid_map ? a0 + b0 * sld : 0;
  for (int k = 0; k < nsrc; k++) {
    const char *s = (const char *)hsrc[k] + (grid_map ? (size_t)(a0 + b0 * ld) * esz : 0);
    rc = stage_rows(dsrc[k], s, (size_t)sld * esz, (size_t)ld * esz,
                    grid_map ? (size_t)q.ny : (size_t)q.nx, st);
    if (rc) return rc;
  }
  return launch_patch(t, D, q, src_layout, sld, off, dsrc[0], dsrc[1], dsrc[2], dsrc[3], nullptr, st);
}

constexpr size_t MAX_PENDING = 64;  // caller streams with updates the mirror has not taken in

// GBP_OPT_DERIVE_SLOPES after an update of q that was given no layers: a node's
// slope cells depend on its four neighbours' heights, so q and the nodes next
// to it are derived again (gbp_slopes.hip), on st behind the apply launch
int derive_around(gbp_terrain *t, const gbp_patch::Rect &q, const int32_t *status, hipStream_t st) {
  gbp_patch::Rect d;
  d.ix0 = std::max(q.ix0 - 1, 0);
  d.iy0 = std::max(q.iy0 - 1, 0);
  d.nx = std::min(q.ix0 + q.nx + 1, t->nx) - d.ix0;
  d.ny = std::min(q.iy0 + q.ny + 1, t->ny) - d.iy0;
  double *const lay[3] = {t->d_dx, t->d_dy, t->d_dz};
  return gbp_internal_derive_slopes(t, t->d_z, t->d_x, t->d_y, lay, d, d,
                                    (int)(t->opt_derive & GBP_SLOPES_F32), status, st);
}

// what gbp_terrain_update_dev leaves for the mirror
int note_pending(gbp_terrain *t, const gbp_patch::Rect &q, hipStream_t st) {
  int rc;
  // the mirror takes the rectangle in lazily (host_mirror), a rejected one too:
  // its heights are as they were, reading them again changes nothing
  for (auto &u : t->pending)
    if (u.stream == st) {
      HIPCHK(hipEventRecord(u.done, st));  // behind the stream's earlier updates as well
      u.rect = gbp_patch::rect_union(u.rect, q);
      return GBP_OK;
    }
  if (t->pending.size() >= MAX_PENDING && (rc = gbp_internal_mirror_sync(t))) return rc;
  hipEvent_t ev;
  HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  if (hipEventRecord(ev, st) != hipSuccess) {
    (void)hipEventDestroy(ev);
    return GBP_E_HIP;
  }
  t->pending.push_back({st, q, ev});
  return GBP_OK;
}

}  // namespace

__attribute__((visibility("hidden"))) int gbp_internal_mirror_sync(gbp_terrain *t) {
  if (t->pending.empty()) return GBP_OK;
  DeviceGuard g(t->device);
  gbp_patch::Rect u = t->pending[0].rect;
  for (auto &p : t->pending) u = gbp_patch::rect_union(u, p.rect);
  int rc = wait_pending(t);
  if (rc) return rc;
  std::vector<double> h((size_t)u.nx * u.ny);
  if ((rc = read_rect(t, u, 0, h.data()))) return rc;
  // the read-back is x-major with ld = u.ny
  gbp_patch::scatter(t->host.z.data(), t->nx, t->ny, u, GBP_SRC_F64_XMAJOR, u.ny, h.data(), false);
  t->nan_free = gbp_patch::nan_free_after(t->host.z.data(), t->nx, t->ny, u, t->nan_free != 0);
  for (auto &p : t->pending) (void)hipEventDestroy(p.done);
  t->pending.clear();
  return GBP_OK;
}

extern "C" {

int gbp_terrain_update_dev(gbp_terrain *t, const gbp_rect *r, int src_layout, int64_t ld,
                           const void *z, const void *dx, const void *dy, const void *dz,
                           int32_t *status, gbp_stream stream) {
  if (!valid_handle(t)) return GBP_E_BAD_HANDLE;
  gbp_patch::Rect q;
  int rc = check_args(t, r, src_layout, ld, z, dx, dy, dz, &q);
  if (rc) return rc;
  const bool need_check = src_layout == GBP_SRC_F64_XMAJOR && t->storage == GBP_STORAGE_F32;
  if (need_check && !status) return GBP_E_INVALID_ARG;
  DeviceGuard g(t->device);
  hipStream_t st = (hipStream_t)stream;
  if (status) HIPCHK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  if (need_check) {
    const int64_t n = (int64_t)q.nx * q.ny;
    k_terrain_check<<<grid_for(n, PATCH_BLOCK, 4096), PATCH_BLOCK, 0, st>>>(
        (const double *)z, ld, q.nx, q.ny, status);
    HIPCHK(hipGetLastError());
  }
  if ((rc = launch_patch(t, dest_of(t), q, src_layout, ld, 0, z, dx, dy, dz,
                         need_check ? status : nullptr, st)))
    return rc;
  // GBP_OPT_DERIVE_SLOPES: behind the apply launch on the same stream (a launch
  // error is reported once the mirror knows of the rectangle)
  int drc = GBP_OK;
  if (t->opt_derive && !dx) drc = derive_around(t, q, need_check ? status : nullptr, st);
  rc = note_pending(t, q, st);
  return rc ? rc : drc;
}

int gbp_terrain_update_host(gbp_terrain *t, const gbp_rect *r, int src_layout, int64_t ld,
                            const void *z, const void *dx, const void *dy, const void *dz) {
  if (!valid_handle(t)) return GBP_E_BAD_HANDLE;
  gbp_patch::Rect q;
  int rc = check_args(t, r, src_layout, ld, z, dx, dy, dz, &q);
  if (rc) return rc;
  // all or nothing: the patch is checked before anything is staged
  if ((rc = gbp_patch::check_patch(t->nx, t->ny, t->storage, r, src_layout, ld, z, &q))) return rc;
  DeviceGuard g(t->device);
  hipStream_t st = t->host_stream;
  if ((rc = wait_pending(t))) return rc;
  DevBuf buf;
  if ((rc = stage_patch(t, dest_of(t), q, src_layout, ld, z, dx, dy, dz, buf, st))) return rc;
  // GBP_OPT_DERIVE_SLOPES.  The heights are on their way by now: should this
  // launch fail, the host copy still takes them in, and the error is returned
  // with the layers as they were
  const int drc = t->opt_derive && !dx ? derive_around(t, q, nullptr, st) : GBP_OK;
  HIPCHK(hipStreamSynchronize(st));
  gbp_patch::scatter(t->host.z.data(), t->nx, t->ny, q, src_layout, ld, z,
                     t->storage == GBP_STORAGE_F32);
  t->nan_free = gbp_patch::nan_free_after(t->host.z.data(), t->nx, t->ny, q, t->nan_free != 0);
  return drc;
}

int gbp_terrain_move_host(gbp_terrain *t, int64_t sx, int64_t sy, const double *x, const double *y,
                          int src_layout, int64_t ld, const void *z, const void *dx,
                          const void *dy, const void *dz) {
  if (!valid_handle(t)) return GBP_E_BAD_HANDLE;
  if (!x || !y) return GBP_E_INVALID_ARG;
  const int NX = t->nx, NY = t->ny;
  gbp_patch::Rect whole;
  whole.nx = NX;
  whole.ny = NY;
  const gbp_patch::MoveRects m = gbp_patch::move_rects(NX, NY, sx, sy);
  int rc;
  // the source is read only where there is a strip, and checked only then
  if (m.nstrips && (rc = gbp_patch::check_source(src_layout, NX, whole, ld, z))) return rc;
  if ((dx == nullptr) != (dy == nullptr) || (dx == nullptr) != (dz == nullptr))
    return GBP_E_INVALID_ARG;
  if (dx && !t->d_dx) return GBP_E_INVALID_ARG;
  if (!coords_ascending(x, NX) || !coords_ascending(y, NY)) return GBP_E_INVALID_ARG;
  // all or nothing: the strips are checked before anything is staged
  const bool f32 = t->storage == GBP_STORAGE_F32;
  for (int k = 0; f32 && k < m.nstrips; k++)
    if (!gbp_patch::round_trips(src_layout, NX, NY, m.strip[k], ld,
                                gbp_patch::move_src(src_layout, ld, z, m.strip[k])))
      return GBP_E_UNSUPPORTED;
  DeviceGuard g(t->device);
  hipStream_t st = t->host_stream;
  // behind every earlier gbp_terrain_update_dev, whose rectangles the mirror takes in first
  if ((rc = gbp_internal_mirror_sync(t))) return rc;
  const bool moved = sx != 0 || sy != 0;
  // GBP_OPT_DERIVE_SLOPES and no layers given: the second set's layers are
  // derived whole from the moved heights and the new coordinates, not shifted
  // and patched (one launch, no seam cases; tools/slopes_ab.py (d) has its cost)
  const bool derive = t->opt_derive && !dx && t->d_dx;
  // the second set of buffers, freed at scope exit unless the swap took them
  struct Spare {
    Dest d;
    ~Spare() {
      if (d.zp) (void)hipFree(d.zp);
      for (double *p : d.lay)
        if (p) (void)hipFree(p);
    }
  } spare;
  DevBuf staged[2], coords;
  // device events around the shift launch alone (gbp_terrain_move_shift_ms)
  struct Timer {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Timer() {
      for (hipEvent_t ev : e)
        if (ev) (void)hipEventDestroy(ev);
    }
  } timer;
  bool timed = false;
  if (moved || derive) {
    const size_t cells = (size_t)NX * NY, esz = f32 ? sizeof(float) : sizeof(double);
    if (moved && hipMalloc(&spare.d.zp, 2 * ((size_t)NX - 1) * NY * esz) != hipSuccess) {
      spare.d.zp = nullptr;
      return GBP_E_ALLOC;
    }
    for (int k = 0; t->d_dx && k < 3; k++)
      if (hipMalloc((void **)&spare.d.lay[k], cells * sizeof(double)) != hipSuccess) {
        spare.d.lay[k] = nullptr;
        return GBP_E_ALLOC;
      }
    const bool shift_layers = t->d_dx && !derive;
    // no overlap and no layers to shift: the strip is the whole map
    if (moved && (m.overlap.nx > 0 || shift_layers)) {
      ShiftArgs A;
      A.zo = t->d_z;
      A.zn = spare.d.zp;
      const double *lo[3] = {t->d_dx, t->d_dy, t->d_dz};
      for (int k = 0; k < 3; k++) {
        A.lo[k] = lo[k];
        A.ln[k] = spare.d.lay[k];
      }
      A.NX = NX;
      A.NY = NY;
      // no overlap: every |shift| that large is the same launch (nothing copied, layers filled)
      A.sx = m.overlap.nx > 0 ? (int)sx : NX;
      A.sy = m.overlap.nx > 0 ? (int)sy : NY;
      const dim3 grid((unsigned)((NY + PATCH_BLOCK - 1) / PATCH_BLOCK),
                      (unsigned)std::min(std::max((NX + SHIFT_ROWS - 1) / SHIFT_ROWS, 1), 4096),
                      shift_layers ? 4u : 1u);
      timed = hipEventCreate(&timer.e[0]) == hipSuccess && hipEventCreate(&timer.e[1]) == hipSuccess &&
              hipEventRecord(timer.e[0], st) == hipSuccess;
      if (f32)
        k_terrain_shift<float><<<grid, PATCH_BLOCK, 0, st>>>(A);
      else
        k_terrain_shift<double><<<grid, PATCH_BLOCK, 0, st>>>(A);
      HIPCHK(hipGetLastError());
      timed = timed && hipEventRecord(timer.e[1], st) == hipSuccess;
    }
    for (int k = 0; k < m.nstrips; k++) {
      const gbp_patch::Rect &q = m.strip[k];
      if ((rc = stage_patch(t, spare.d, q, src_layout, ld, gbp_patch::move_src(src_layout, ld, z, q),
                            gbp_patch::move_src(src_layout, ld, dx, q),
                            gbp_patch::move_src(src_layout, ld, dy, q),
                            gbp_patch::move_src(src_layout, ld, dz, q), staged[k], st))) {
        (void)hipStreamSynchronize(st);  // nothing in flight when the buffers go
        return rc;
      }
    }
    if (derive) {  // behind the shift and the strips, with the new coordinates
      double *cx = nullptr, *cy = nullptr;
      rc = stage_buf(coords, [&](Stage &S) {
        S.take(cx, (size_t)NX);
        S.take(cy, (size_t)NY);
      });
      if (!rc) rc = h2d(cx, x, (size_t)NX, st);
      if (!rc) rc = h2d(cy, y, (size_t)NY, st);
      if (!rc)
        rc = gbp_internal_derive_slopes(t, moved ? spare.d.zp : t->d_z, cx, cy, spare.d.lay, whole,
                                        whole, (int)(t->opt_derive & GBP_SLOPES_F32), nullptr, st);
      if (rc) {
        (void)hipStreamSynchronize(st);  // nothing in flight when the buffers go
        return rc;
      }
    }
    HIPCHK(hipStreamSynchronize(st));
  }
  float shift_ms = -1.0f;
  if (timed && hipEventElapsedTime(&shift_ms, timer.e[0], timer.e[1]) != hipSuccess) shift_ms = -1.0f;
  // the last step that can fail; the rest is the swap and host fields
  if ((rc = gbp_internal_set_geometry(t, x, y))) return rc;
  if ((moved || derive) && t->d_dx) {
    std::swap(t->d_dx, spare.d.lay[0]);
    std::swap(t->d_dy, spare.d.lay[1]);
    std::swap(t->d_dz, spare.d.lay[2]);
  }
  if (moved) {
    std::swap(t->d_z, spare.d.zp);  // the old buffers leave with `spare`
    double *mz = t->host.z.data();
    gbp_patch::shift_mirror(mz, NX, NY, sx, sy, m);
    for (int k = 0; k < m.nstrips; k++)
      gbp_patch::scatter(mz, NX, NY, m.strip[k], src_layout, ld,
                         gbp_patch::move_src(src_layout, ld, z, m.strip[k]), f32);
    t->nan_free = gbp_patch::nan_free_after_move(mz, NX, NY, m, t->nan_free != 0);
  }
  t->last_shift_ms = shift_ms;
  return GBP_OK;
}

int gbp_terrain_move_shift_ms(const gbp_terrain *t, float *ms) {
  if (!valid_handle(t)) return GBP_E_BAD_HANDLE;
  if (!ms) return GBP_E_INVALID_ARG;
  *ms = t->last_shift_ms;
  return GBP_OK;
}

int gbp_coord_shift(const double *old_c, const double *new_c, int n, double rel_tol, int *shift) {
  if (!old_c || !new_c || !shift) return 0;
  return gbp_patch::detect_shift(old_c, new_c, n, rel_tol, shift) ? 1 : 0;
}

int gbp_terrain_read_host(gbp_terrain *t, const gbp_rect *r, int copy, double *z) {
  if (!valid_handle(t)) return GBP_E_BAD_HANDLE;
  gbp_patch::Rect q;
  int rc = gbp_patch::resolve_rect(t->nx, t->ny, r, &q);
  if (rc) return rc;
  if ((copy != 0 && copy != 1) || !z) return GBP_E_INVALID_ARG;
  DeviceGuard g(t->device);
  // a synchronous read: the mirror takes the pending updates in on the way
  // (one more copy of their rectangles), which re-establishes nan_free
  if ((rc = gbp_internal_mirror_sync(t))) return rc;
  return read_rect(t, q, copy, z);
}

}  // extern "C"
