// gbp_terrain_patch.cpp — see gbp_terrain_patch.h
#include "gbp_terrain_patch.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace gbp_patch {

int resolve_rect(int NX, int NY, const gbp_rect *r, Rect *out) {
  Rect q;
  if (r) {
    q.ix0 = r->ix0;
    q.iy0 = r->iy0;
    q.nx = r->nx;
    q.ny = r->ny;
  } else {
    q.nx = NX;
    q.ny = NY;
  }
  if (q.nx <= 0 || q.ny <= 0 || q.ix0 < 0 || q.iy0 < 0) return GBP_E_SHAPE;
  if ((int64_t)q.ix0 + q.nx > NX || (int64_t)q.iy0 + q.ny > NY) return GBP_E_SHAPE;
  *out = q;
  return GBP_OK;
}

void pair_rows(int NX, const Rect &r, int *p0, int *p1) {
  *p0 = std::max(r.ix0 - 1, 0);
  *p1 = std::min(r.ix0 + r.nx, NX - 1);
}

Rect rect_union(const Rect &a, const Rect &b) {
  Rect u;
  u.ix0 = std::min(a.ix0, b.ix0);
  u.iy0 = std::min(a.iy0, b.iy0);
  u.nx = std::max(a.ix0 + a.nx, b.ix0 + b.nx) - u.ix0;
  u.ny = std::max(a.iy0 + a.ny, b.iy0 + b.ny) - u.iy0;
  return u;
}

int check_source(int layout, int NX, const Rect &r, int64_t ld, const void *src) {
  if (layout != GBP_SRC_F64_XMAJOR && layout != GBP_SRC_F32_GRIDMAP) return GBP_E_INVALID_ARG;
  if (!src) return GBP_E_INVALID_ARG;
  if (ld < (layout == GBP_SRC_F32_GRIDMAP ? (int64_t)NX : (int64_t)r.ny)) return GBP_E_SHAPE;
  return GBP_OK;
}

bool round_trips(int layout, int NX, int NY, const Rect &r, int64_t ld, const void *src) {
  if (layout == GBP_SRC_F32_GRIDMAP) return true;
  for (int ix = r.ix0; ix < r.ix0 + r.nx; ix++)
    for (int iy = r.iy0; iy < r.iy0 + r.ny; iy++) {
      const double v = src_value(layout, NX, NY, r, ld, src, ix, iy);
      if (!std::isnan(v) && (double)(float)v != v) return false;
    }
  return true;
}

int check_patch(int NX, int NY, int storage, const gbp_rect *r, int layout, int64_t ld,
                const void *src, Rect *out) {
  Rect q;
  int rc = resolve_rect(NX, NY, r, &q);
  if (rc) return rc;
  rc = check_source(layout, NX, q, ld, src);
  if (rc) return rc;
  if (storage == GBP_STORAGE_F32 && !round_trips(layout, NX, NY, q, ld, src))
    return GBP_E_UNSUPPORTED;
  *out = q;
  return GBP_OK;
}

void scatter(double *mirror, int NX, int NY, const Rect &r, int layout, int64_t ld,
             const void *src, bool f32) {
  for (int ix = r.ix0; ix < r.ix0 + r.nx; ix++)
    for (int iy = r.iy0; iy < r.iy0 + r.ny; iy++) {
      const double v = src_value(layout, NX, NY, r, ld, src, ix, iy);
      mirror[(int64_t)ix * NY + iy] = f32 ? (double)(float)v : v;
    }
}

bool nan_free(const double *z, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (std::isnan(z[i])) return false;
  return true;
}

bool nan_free_after(const double *mirror, int NX, int NY, const Rect &r, bool was) {
  if (!was) return nan_free(mirror, (size_t)NX * (size_t)NY);
  for (int ix = r.ix0; ix < r.ix0 + r.nx; ix++)
    if (!nan_free(mirror + (int64_t)ix * NY + r.iy0, (size_t)r.ny)) return false;
  return true;
}

MoveRects move_rects(int NX, int NY, int64_t sx, int64_t sy) {
  MoveRects m;
  const auto whole = [&] {
    Rect r;
    r.nx = NX;
    r.ny = NY;
    return r;
  };
  if (sx <= -(int64_t)NX || sx >= NX || sy <= -(int64_t)NY || sy >= NY) {
    m.nstrips = 1;
    m.strip[0] = whole();
    return m;
  }
  const int ax = (int)(sx < 0 ? -sx : sx), ay = (int)(sy < 0 ? -sy : sy);
  Rect &o = m.overlap;
  o.ix0 = sx < 0 ? ax : 0;
  o.iy0 = sy < 0 ? ay : 0;
  o.nx = NX - ax;
  o.ny = NY - ay;
  if (ax) {  // |sx| full rows: below the overlap for sx < 0, above it otherwise
    Rect &r = m.strip[m.nstrips++];
    r.ix0 = sx < 0 ? 0 : o.nx;
    r.iy0 = 0;
    r.nx = ax;
    r.ny = NY;
  }
  if (ay) {  // |sy| columns of the overlap's rows
    Rect &r = m.strip[m.nstrips++];
    r.ix0 = o.ix0;
    r.iy0 = sy < 0 ? 0 : o.ny;
    r.nx = o.nx;
    r.ny = ay;
  }
  return m;
}

void shift_mirror(double *mirror, int NX, int NY, int64_t sx, int64_t sy, const MoveRects &m) {
  const Rect &o = m.overlap;
  if (o.nx <= 0 || o.ny <= 0 || (sx == 0 && sy == 0)) return;
  // sx > 0 reads rows above the ones it writes: ascending; sx < 0 descending;
  // within a row (sx = 0) memmove takes the overlap of source and destination
  for (int k = 0; k < o.nx; k++) {
    const int ix = sx >= 0 ? o.ix0 + k : o.ix0 + o.nx - 1 - k;
    std::memmove(mirror + (int64_t)ix * NY + o.iy0, mirror + (int64_t)(ix + sx) * NY + (o.iy0 + sy),
                 sizeof(double) * (size_t)o.ny);
  }
}

bool nan_free_after_move(const double *mirror, int NX, int NY, const MoveRects &m, bool was) {
  if (!was) return nan_free(mirror, (size_t)NX * (size_t)NY);
  for (int k = 0; k < m.nstrips; k++)
    if (!nan_free_after(mirror, NX, NY, m.strip[k], true)) return false;
  return true;
}

bool detect_shift(const double *o, const double *n, int N, double rel_tol, int *shift) {
  if (N < 2) return false;
  const double h = (o[N - 1] - o[0]) / (double)(N - 1);
  if (!(h > 0) || !std::isfinite(h)) return false;
  const double s = std::round((n[0] - o[0]) / h);
  if (!(std::fabs(s) < 2147483647.0)) return false;  // NaN as well
  const int64_t sh = (int64_t)s;
  const double tol = h * rel_tol;
  for (int64_t i = std::max<int64_t>(0, -sh); i < std::min<int64_t>(N, (int64_t)N - sh); i++)
    if (!(std::fabs(n[i] - o[i + sh]) <= tol)) return false;
  for (int i = 0; i < N; i++)
    if (std::isnan(n[i])) return false;
  *shift = (int)sh;
  return true;
}

}  // namespace gbp_patch
