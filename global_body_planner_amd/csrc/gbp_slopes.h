// gbp_slopes.h — a node's slope layers (dx, dy, dz) from the heights around it,
// stated once for the device (gbp_slopes.hip's k_derive_slopes) and the host
// (tests/native/slopes_probe.cpp).  It is the recipe terrain_data.synth_fractal
// applies with numpy: central differences, (-gx, -gy, 1) / |.|, optionally
// rounded through float.
//
// Plain C++17 on doubles, FP64 in the stated operation order, built without FMA
// contraction: the pragma below does that for clang, -ffp-contract=off for g++
// (as gbp_closed_forms.h).
#pragma once
#ifdef __clang__
#pragma clang fp contract(off)
#endif

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define GBP_SLOPES_HD __host__ __device__ __forceinline__
#else
#define GBP_SLOPES_HD inline
#endif
#include <cmath>

#include "gbp.h"

namespace gbp {

// One axis of node c with neighbours m (index - 1) and p (index + 1).  A
// neighbour is usable when it lies in the map and its height is not NaN:
// central difference with both, one-sided with one, 0.0 with none.  The
// one-sided rule beside a NaN cell is deliberate: that cell already invalidates
// the states inside it, its neighbours are valid ground and keep a finite normal.
// Infinite heights and repeated coordinates get whatever IEEE gives.
GBP_SLOPES_HD double slope_gradient(bool in_m, bool in_p, double zm, double zc, double zp, double xm,
                                    double xc, double xp) {
  const bool um = in_m && !(zm != zm), up = in_p && !(zp != zp);
  if (um && up) return (zp - zm) / (xp - xm);
  if (up) return (zp - zc) / (xp - xc);
  if (um) return (zc - zm) / (xc - xm);
  return 0.0;
}

// n = (-gx, -gy, 1) / sqrt((gx gx + gy gy) + 1); the signs are part of the
// rule (a flat node gives -0.0, as numpy's -gx does).  A node whose own height
// is NaN reads (0, 0, 1), what a handle without layers reads.  GBP_SLOPES_F32:
// each component rounded through float last, what a grid_map layer would hold.
GBP_SLOPES_HD void slope_normal(double zc, double gx, double gy, int flags, double n[3]) {
  if (zc != zc) {
    n[0] = 0.0;
    n[1] = 0.0;
    n[2] = 1.0;
    return;
  }
  const double l = sqrt((gx * gx + gy * gy) + 1.0);
  n[0] = (-gx) / l;
  n[1] = (-gy) / l;
  n[2] = 1.0 / l;
  if (flags & GBP_SLOPES_F32) {
    n[0] = (double)(float)n[0];
    n[1] = (double)(float)n[1];
    n[2] = (double)(float)n[2];
  }
}

// Node (ix, iy) of an x-major map z[nx][ny] with coordinates x[nx], y[ny]: the
// rule on a plain array (the host statement; the kernel gathers the same five
// heights from the x-pairs).
inline void slope_node_xmajor(const double *z, const double *x, const double *y, int nx, int ny,
                              int ix, int iy, int flags, double n[3]) {
  const bool xm = ix > 0, xp = ix + 1 < nx, ym = iy > 0, yp = iy + 1 < ny;
  const double zc = z[(size_t)ix * ny + iy];
  const double gx = slope_gradient(xm, xp, xm ? z[(size_t)(ix - 1) * ny + iy] : 0.0, zc,
                                   xp ? z[(size_t)(ix + 1) * ny + iy] : 0.0, xm ? x[ix - 1] : 0.0,
                                   x[ix], xp ? x[ix + 1] : 0.0);
  const double gy = slope_gradient(ym, yp, ym ? z[(size_t)ix * ny + iy - 1] : 0.0, zc,
                                   yp ? z[(size_t)ix * ny + iy + 1] : 0.0, ym ? y[iy - 1] : 0.0,
                                   y[iy], yp ? y[iy + 1] : 0.0);
  slope_normal(zc, gx, gy, flags, n);
}

}  // namespace gbp
