// gbp_hrow.h — a vertex's row of the fp16 split rows the matrix-core
// nearest-neighbour search reads (gbp_nn.hip, "nearest neighbour in a device
// tree on the matrix cores": the layout's use and its error bounds), shared
// with the kernels that write rows outside the planner loop
// (gbp_tree_maint.hip's move).  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

constexpr int NH_ROW = 32;             // fp16 per row: F_hi[8] F_lo[8] F_hi[8] N_1 N_2 N_3 0[5]
constexpr double NH_SCALE = 64.0;      // F = 64 v (exact)
constexpr double NH_LIM = 8192.0;      // |F_k| < 2^13: |F|^2 * 2^-14 < 2^15 fits fp16
constexpr double NH_NSCALE = 0x1p-14;  // the norm parts are |F|^2 * 2^-14 ...

typedef _Float16 nh8 __attribute__((ext_vector_type(8)));

// fp16 hi + lo of a scaled coordinate (|x| < 2^13)
__device__ __forceinline__ void nh_split(double x, _Float16 &hi, _Float16 &lo) {
  hi = (_Float16)(float)x;
  lo = (_Float16)(float)(x - (double)hi);
}

// row j of the fp16 rows; hm = {hmax[8], hbad}
__device__ __forceinline__ void nn_put_hrow(_Float16 *__restrict__ vh, float *__restrict__ hm,
                                            int64_t j, const double *s, bool init) {
  nh8 fh, fl, nr;
  double n = 0.0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const double x = s[k] * NH_SCALE;
    const bool ok = fabs(x) < NH_LIM;
    bad = bad || !ok;
    _Float16 hi, lo;
    nh_split(ok ? x : 0.0, hi, lo);
    fh[k] = hi;
    fl[k] = lo;
    n = n + x * x;
    const float ax = ok ? (float)fabs(x) : 0.f;
    if (!hm) continue;  // a query row
    if (init)
      hm[k] = ax;
    else
      atomicMax((unsigned int *)(hm + k), __float_as_uint(ax));
  }
  const double ns = bad ? 0.0 : n * NH_NSCALE;
  const _Float16 n1 = (_Float16)(float)ns;
  const double r1 = ns - (double)n1;
  const _Float16 n2 = (_Float16)(float)r1;
  const _Float16 n3 = (_Float16)(float)(r1 - (double)n2);
  nr = nh8{n1, n2, n3, 0, 0, 0, 0, 0};
  nh8 *r = (nh8 *)(vh + (int64_t)NH_ROW * j);
  r[0] = fh;
  r[1] = fl;
  r[2] = fh;
  r[3] = nr;
  if (!hm) return;
  if (init)
    ((uint32_t *)hm)[8] = bad ? 1u : 0u;
  else if (bad)
    atomicOr((uint32_t *)hm + 8, 1u);
}
