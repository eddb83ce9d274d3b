// gbp_tree_trim.hip — a device tree trimmed by cost: which
// vertices an anytime RRT*-Connect may drop once a solution is held (the
// branch-and-bound test f = g + h > best cost) or once a tree outgrows a vertex
// budget (the max_keep - 1 non-root vertices of least f stay).  This unit is
// the decision alone, gbp_tree_trim_flags_dev: f, the budget's cut by a radix
// select, the protected chain and the flag array.  The flags are what
// gbp_tree_prune_dev (gbp_tree_maint.hip) takes as edge_valid, so the keep
// rule, the compaction, the search rows and the successor lists are the
// prune's; gbp_tree_trim_host / _keep_host run the two stages.
//
// k_trim_f writes f and resets the call's record, k_trim_chain marks the
// protected chain, eight rounds of k_trim_hist / k_trim_pick fix the cut's
// 64-bit image one byte at a time, k_trim_flags decides.  Nothing comes to the
// host in between: the cut, the select's prefix and remaining rank and the
// chain's verdict live in the record (TrimCtl) the next kernel reads.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "gbp.h"
#include "gbp_device.h"
#include "gbp_internal.h"

using namespace gbp;

namespace {

constexpr int TRIM_BINS = 256;      // one byte of the key per round
constexpr int TRIM_ROUNDS = 8;
constexpr int TRIM_HIST_GRID = 128;  // workgroups of a histogram round at most (rows of partial counts)

// the call's device record
struct TrimCtl {
  unsigned long long prefix;  // the cut's key, the bytes fixed so far (the rest zero)
  uint32_t rank;              // rank of the cut among the keys that share the prefix
  uint32_t ok;                // n is the tree's count
  uint32_t active;            // the budget applies (max_keep >= 1 and n > max_keep)
  uint32_t bad_chain;         // the protected chain left the tree or did not reach the root
  double cut;                 // +inf until the last round of an active select
};

// The order-preserving image of a double: a < b exactly when key(a) < key(b),
// for every non-NaN pair with -0 taken as +0; every NaN maps to the largest
// key, above +inf's.
__device__ __forceinline__ unsigned long long trim_key(double f) {
  if (f != f) return ~0ull;
  if (f == 0.0) f = 0.0;
  const unsigned long long b = (unsigned long long)__double_as_longlong(f);
  return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double trim_unkey(unsigned long long k) {
  if (k == ~0ull) return __longlong_as_double(0x7FF8000000000000ll);
  const unsigned long long b = (k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k;
  return __longlong_as_double((long long)b);
}

// f[i] = g[i] + pose_distance(v[i], r), r the other tree's root row, read here.
// When n is not the tree's count nothing of the tree is read and f is zero.
// Thread 0 of the grid resets the record and the stats.
__global__ __launch_bounds__(TB) void k_trim_f(gbp_tree t, gbp_tree o, int32_t n, int64_t max_keep,
                                               double *__restrict__ f, uint8_t *__restrict__ prot,
                                               TrimCtl *__restrict__ ctl,
                                               gbp_trim_stats *__restrict__ stats) {
  const bool ok = *t.count == n;
  double r[8];
  if (ok) copy8(r, o.v);
  const int64_t first = (int64_t)blockIdx.x * TB + threadIdx.x;
  for (int64_t i = first; i < n; i += (int64_t)gridDim.x * TB) {
    f[i] = ok ? t.g[i] + pose_distance(t.v + 8 * i, r) : 0.0;
    prot[i] = 0;
  }
  if (first == 0) {
    const bool active = ok && max_keep >= 1 && (int64_t)n > max_keep;
    ctl->prefix = 0ull;
    ctl->rank = active ? (uint32_t)(max_keep - 1) : 0u;
    ctl->ok = ok ? 1u : 0u;
    ctl->active = active ? 1u : 0u;
    ctl->bad_chain = 0u;
    ctl->cut = INFINITY;
    stats->n_before = n;
    stats->n_kept = 0;
    stats->n_over_bound = 0;
    stats->n_over_budget = 0;
    stats->n_protected = 0;
    stats->n_inherited = 0;
    stats->error = 0;
    stats->cut = INFINITY;
  }
}

// One lane walks protect -> root and marks it: at most n steps, every parent
// checked against [0, n).
__global__ void k_trim_chain(gbp_tree t, int32_t n, int32_t protect, uint8_t *__restrict__ prot,
                             TrimCtl *__restrict__ ctl) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || !ctl->ok) return;
  int32_t idx = protect;
  bool reached = false;
  for (int32_t steps = 0; steps < n && !reached; steps++) {
    if (idx < 0 || idx >= n) break;
    prot[idx] = 1;
    reached = idx == 0;
    if (!reached) idx = t.parent[idx];
  }
  if (!reached) ctl->bad_chain = 1u;
}

// One round of the select over f[1 .. n): the histogram of the key's byte at
// `shift` among the keys that agree with the prefix above it, counted in LDS
// and written as this workgroup's own row part[blockIdx.x][TRIM_BINS].  A
// tree's f lie close together, so in the first rounds most lanes of a wave hold
// one byte value: the lanes that share the first active lane's byte are
// counted with a ballot and added once, the others add for themselves.
__global__ __launch_bounds__(TB) void k_trim_hist(const double *__restrict__ f, int32_t n,
                                                  const TrimCtl *__restrict__ ctl, int shift,
                                                  uint32_t *__restrict__ part) {
  __shared__ uint32_t hist[TRIM_BINS];
  if (!ctl->active) return;
  const unsigned long long prefix = ctl->prefix;
  for (int b = threadIdx.x; b < TRIM_BINS; b += TB) hist[b] = 0u;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * TB;
  // every lane of a wave takes the same number of turns (the ballot is wave wide)
  for (int64_t base = (int64_t)blockIdx.x * TB; base < n - 1; base += stride) {
    const int64_t i = 1 + base + threadIdx.x;
    bool in = i < n;
    uint32_t digit = 0;
    if (in) {
      const unsigned long long k = trim_key(f[i]);
      in = shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8));
      digit = (uint32_t)(k >> shift) & (TRIM_BINS - 1);
    }
    const unsigned long long act = __ballot(in);
    if (act) {
      const int lead = __ffsll((long long)act) - 1;
      const uint32_t dl = (uint32_t)__shfl((int)digit, lead, WAVE);
      const unsigned long long same = __ballot(in && digit == dl);
      if ((int)(threadIdx.x & (WAVE - 1)) == lead)
        atomicAdd(&hist[dl], (uint32_t)__popcll(same));
      else if (in && digit != dl)
        atomicAdd(&hist[digit], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < TRIM_BINS; b += TB) part[(int64_t)blockIdx.x * TRIM_BINS + b] = hist[b];
}

// One workgroup of TRIM_BINS threads: the rows summed per byte value, the
// value whose run of keys holds the remaining rank chosen, prefix and rank
// updated; after the last round the cut is the prefix's double.
__global__ __launch_bounds__(TRIM_BINS) void k_trim_pick(const uint32_t *__restrict__ part, int rows,
                                                         int shift, TrimCtl *__restrict__ ctl) {
  __shared__ uint32_t cnt[TRIM_BINS];
  if (!ctl->active) return;
  uint32_t c = 0;
  for (int r = 0; r < rows; r++) c += part[(int64_t)r * TRIM_BINS + threadIdx.x];
  cnt[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint32_t rank = ctl->rank, before = 0;
  int d = 0;
  for (; d < TRIM_BINS - 1 && rank >= before + cnt[d]; d++) before += cnt[d];
  const unsigned long long prefix = ctl->prefix | ((unsigned long long)d << shift);
  ctl->prefix = prefix;
  ctl->rank = rank - before;
  if (shift == 0) ctl->cut = trim_unkey(prefix);
}

// keep[i]: the vertex passes both tests or lies on the protected chain; the
// counts summed per workgroup, one integer atomic each.
__global__ __launch_bounds__(TB) void k_trim_flags(int32_t n, double bound, const double *__restrict__ f,
                                                   const uint8_t *__restrict__ prot,
                                                   const TrimCtl *__restrict__ ctl,
                                                   uint8_t *__restrict__ keep, double *__restrict__ f_out,
                                                   gbp_trim_stats *__restrict__ stats) {
  __shared__ uint32_t sum[3];
  const bool good = ctl->ok && !ctl->bad_chain;
  const bool active = ctl->active != 0;
  const double cut = ctl->cut;
  if (threadIdx.x < 3) sum[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t mine[3] = {0u, 0u, 0u};
  const int64_t first = (int64_t)blockIdx.x * TB + threadIdx.x;
  for (int64_t i = first; i < n; i += (int64_t)gridDim.x * TB) {
    const double x = f[i];
    if (f_out) f_out[i] = x;
    if (!good) {
      keep[i] = 0;
      continue;
    }
    if (i == 0) {
      keep[0] = 1;
      continue;
    }
    const bool over_bound = x > bound;
    const bool over_budget = !over_bound && active && !(x < cut);
    const bool fail = over_bound || over_budget, p = prot[i] != 0;
    keep[i] = (!fail || p) ? 1 : 0;
    mine[0] += over_bound;
    mine[1] += over_budget;
    mine[2] += fail && p;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    uint32_t v = mine[c];
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) v += (uint32_t)__shfl_xor((int)v, s, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0 && v) atomicAdd(&sum[c], v);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (sum[0]) atomicAdd((unsigned long long *)&stats->n_over_bound, (unsigned long long)sum[0]);
    if (sum[1]) atomicAdd((unsigned long long *)&stats->n_over_budget, (unsigned long long)sum[1]);
    if (sum[2]) atomicAdd((unsigned long long *)&stats->n_protected, (unsigned long long)sum[2]);
    if (first == 0) {
      stats->cut = cut;
      stats->error = !ctl->ok ? 1 : ctl->bad_chain ? 2 : 0;
    }
  }
}

// the call's scratch in the tree's own grow-only buffer (the prune's attempt
// rows live there between calls)
struct TrimBuf {
  double *f = nullptr;
  uint8_t *prot = nullptr;
  uint32_t *part = nullptr;
  TrimCtl *ctl = nullptr;
};
int trim_buf(gbp_tree *tree, int64_t n, TrimBuf &B) {
  auto carve = [&](Stage &S) {
    S.take(B.f, n);
    S.take(B.prot, n);
    S.take(B.part, (size_t)TRIM_HIST_GRID * TRIM_BINS);
    S.take(B.ctl, 1);
  };
  const int rc = ensure_ws(&tree->rv, &tree->rv_bytes, stage_bytes_of(carve));
  return rc ? rc : stage_carve(tree->rv, tree->rv_bytes, carve);
}

int trim_host(gbp_tree *tree, gbp_tree *other, double bound, int64_t max_keep, int32_t protect,
              int32_t *remap, int32_t *remap_dev, int64_t remap_cap, gbp_trim_stats *stats,
              hipStream_t s) {
  if (!tree_ok(tree) || !tree_ok(other)) return GBP_E_BAD_HANDLE;
  if (!stats) return GBP_E_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GBP_E_NO_DEVICE;
  DeviceGuard g(tree->device);
  int64_t n = 0;
  int rc = gbp_tree_size(tree, &n, s);
  if (rc) return rc;
  if (remap_dev && n > remap_cap) return GBP_E_SHAPE;
  if (remap_dev) {  // the caller keeps the device remap: it must lie on the tree's device
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, remap_dev) != hipSuccess || at.device != tree->device) {
      (void)hipGetLastError();
      return GBP_E_INVALID_ARG;
    }
  }
  DevBuf buf;
  uint8_t *keep;
  int32_t *dmap;
  gbp_trim_stats *dts;
  gbp_prune_stats *dps;
  rc = stage_buf(buf, [&](Stage &S) {
    S.take(keep, n);
    S.take(dmap, remap_dev ? 0 : n);
    S.take(dts, 1);
    S.take(dps, 1);
  });
  if (rc) return rc;
  if (remap_dev) dmap = remap_dev;
  if ((rc = gbp_tree_trim_flags_dev(tree, other, n, bound, max_keep, protect, keep, nullptr, dts, s)))
    return rc;
  gbp_trim_stats ts;
  if ((rc = d2h(&ts, dts, 1, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  if (ts.error) return ts.error == 1 ? GBP_E_SHAPE : GBP_E_INVALID_ARG;
  gbp_prune_stats ps;
  if ((rc = gbp_tree_prune_dev(tree, n, keep, dmap, dps, s))) return rc;
  if (remap && (rc = d2h(remap, dmap, n, s))) return rc;
  if ((rc = d2h(&ps, dps, 1, s))) return rc;
  HIPCHK(hipStreamSynchronize(s));
  ts.n_kept = ps.n_kept;
  ts.n_inherited = ps.n_inherited;
  *stats = ts;
  return GBP_OK;
}

}  // namespace

extern "C" {

int gbp_tree_trim_flags_dev(gbp_tree *tree, gbp_tree *other, int64_t n, double bound, int64_t max_keep,
                            int32_t protect, uint8_t *keep, double *f, gbp_trim_stats *stats,
                            gbp_stream stream) {
  if (!tree_ok(tree) || !tree_ok(other)) return GBP_E_BAD_HANDLE;
  if (n < 1 || !keep || !stats || protect < -1 || protect >= n) return GBP_E_INVALID_ARG;
  if (n > tree->cap || n > 0x7FFFFFFF) return GBP_E_SHAPE;
  if (tree->device != other->device) return GBP_E_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GBP_E_NO_DEVICE;
  DeviceGuard g(tree->device);
  hipStream_t s = (hipStream_t)stream;
  TrimBuf B;
  int rc = trim_buf(tree, n, B);
  if (rc) return rc;
  const unsigned gv = grid_for(n, TB, 2048);
  const unsigned gh = grid_for(n - 1, TB, TRIM_HIST_GRID);
  hipLaunchKernelGGL(k_trim_f, dim3(gv), dim3(TB), 0, s, *tree, *other, (int32_t)n, max_keep, B.f, B.prot,
                     B.ctl, stats);
  if (protect >= 0)
    hipLaunchKernelGGL(k_trim_chain, dim3(1), dim3(WAVE), 0, s, *tree, (int32_t)n, protect, B.prot, B.ctl);
  if (max_keep >= 1 && n > max_keep) {
    for (int round = 0; round < TRIM_ROUNDS; round++) {
      const int shift = 56 - 8 * round;
      hipLaunchKernelGGL(k_trim_hist, dim3(gh), dim3(TB), 0, s, B.f, (int32_t)n, B.ctl, shift, B.part);
      hipLaunchKernelGGL(k_trim_pick, dim3(1), dim3(TRIM_BINS), 0, s, B.part, (int)gh, shift, B.ctl);
    }
  }
  hipLaunchKernelGGL(k_trim_flags, dim3(gv), dim3(TB), 0, s, (int32_t)n, bound, B.f, B.prot, B.ctl, keep,
                     f, stats);
  HIPCHK(hipGetLastError());
  return GBP_OK;
}

int gbp_tree_trim_host(gbp_tree *tree, gbp_tree *other, double bound, int64_t max_keep, int32_t protect,
                       int32_t *remap, gbp_trim_stats *stats, gbp_stream stream) {
  return trim_host(tree, other, bound, max_keep, protect, remap, nullptr, 0, stats, (hipStream_t)stream);
}

int gbp_tree_trim_keep_host(gbp_tree *tree, gbp_tree *other, double bound, int64_t max_keep,
                            int32_t protect, int32_t *remap, int32_t *remap_dev, int64_t remap_cap,
                            gbp_trim_stats *stats, gbp_stream stream) {
  return trim_host(tree, other, bound, max_keep, protect, remap, remap_dev, remap_cap, stats,
                   (hipStream_t)stream);
}

}  // extern "C"
