// gbp_tree.hip — the device tree handle of include/gbp.h ("device trees and
// the device planner loop"): create, destroy, reserve, init, size, capacity,
// read, read_links, append_host, load_host, device_ptrs, and the planner
// streams.  The handle and its allocations' list: gbp_internal.h; the fp16
// rows' writer: gbp_hrow.h; the planner's appends: gbp_plan.hip (k_append);
// a tree pruned, re-rooted or grafted: gbp_tree_maint.hip.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <new>
#include <vector>

#include "gbp.h"
#include "gbp_device.h"
#include "gbp_internal.h"

using namespace gbp;

namespace {

__global__ void k_tree_init(gbp_tree t, double r0, double r1, double r2, double r3, double r4,
                            double r5, double r6, double r7) {
  const double r[8] = {r0, r1, r2, r3, r4, r5, r6, r7};
  copy8(t.v, r);
  nn_put_hrow(t.vh, t.hm, 0, r, true);
  for (int k = 0; k < 10; k++) t.a[k] = 0.0;
  t.g[0] = 0.0;
  t.parent[0] = -1;
  t.child[0] = -1;
  t.sibling[0] = -1;
  t.prev[0] = -1;
  *t.count = 1;
}

__global__ void k_tree_append(gbp_tree t, int64_t n, const double *__restrict__ s,
                              const double *__restrict__ a, const int32_t *__restrict__ p) {
  // sequential in index order: a parent may be appended in the same call
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int32_t c = *t.count;
  for (int64_t i = 0; i < n; i++, c++) {
    copy8(t.v + 8 * (int64_t)c, s + 8 * i);
    nn_put_hrow(t.vh, t.hm, c, s + 8 * i, false);
    copy10(t.a + 10 * (int64_t)c, a + 10 * i);
    t.parent[c] = p[i];
    t.g[c] = p[i] >= 0 ? t.g[p[i]] + pose_distance(t.v + 8 * (int64_t)p[i], s + 8 * i) : 0.0;
    t.child[c] = -1;
    t.sibling[c] = -1;
    t.prev[c] = -1;
    if (p[i] >= 0) {
      const int32_t h = t.child[p[i]];
      t.sibling[c] = h;
      if (h >= 0) t.prev[h] = c;
      t.child[p[i]] = c;
    }
  }
  *t.count = c;
}

// gbp_tree_load_host: the given vertices, successor lists, then g from the
// root down through the two level queues (one lane: a test's warm start)
__global__ void k_tree_load(gbp_tree t, int64_t n, const double *__restrict__ s,
                            const double *__restrict__ a, const int32_t *__restrict__ p) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (int64_t i = 0; i < n; i++) {
    copy8(t.v + 8 * i, s + 8 * i);
    nn_put_hrow(t.vh, t.hm, i, s + 8 * i, i == 0);
    copy10(t.a + 10 * i, a + 10 * i);
    t.parent[i] = p[i];
    t.child[i] = -1;
    t.sibling[i] = -1;
    t.prev[i] = -1;
  }
  for (int64_t i = 1; i < n; i++) {
    const int32_t h = t.child[p[i]];
    t.sibling[i] = h;
    if (h >= 0) t.prev[h] = (int32_t)i;
    t.child[p[i]] = (int32_t)i;
  }
  int32_t *q = t.bfs;
  int64_t qh = 0, qt = 0;
  t.g[0] = 0.0;
  q[qt++] = 0;
  while (qh < qt) {
    const int32_t u = q[qh++];
    for (int32_t c = t.child[u]; c >= 0 && qt < n; c = t.sibling[c]) {
      t.g[c] = t.g[u] + pose_distance(t.v + 8 * (int64_t)u, t.v + 8 * (int64_t)c);
      q[qt++] = c;
    }
  }
  *t.count = (int32_t)n;
}

// gbp_tree_append_host / gbp_tree_load_host after their validation: the tree
// raised to `capacity` rows, the n host rows staged through a buffer of their
// own and written by `kernel` (k_tree_append / k_tree_load); synchronous
using TreeRowsKernel = void (*)(gbp_tree, int64_t, const double *, const double *, const int32_t *);
int tree_put_rows(gbp_tree *t, int64_t capacity, TreeRowsKernel kernel, int64_t n,
                  const double *states, const double *actions, const int32_t *parents,
                  gbp_stream stream) {
  int rc = gbp_tree_reserve(t, capacity, stream);
  if (rc) return rc;
  DeviceGuard g(t->device);
  hipStream_t s = (hipStream_t)stream;
  DevBuf buf;
  double *ds, *da;
  int32_t *dp;
  rc = stage_buf(buf, [&](Stage &S) { S.take(ds, 8 * n); S.take(da, 10 * n); S.take(dp, n); });
  if (rc) return rc;
  rc = h2d(ds, states, 8 * n, s);
  if (!rc) rc = h2d(da, actions, 10 * n, s);
  if (!rc) rc = h2d(dp, parents, n, s);
  if (!rc) {
    hipLaunchKernelGGL(kernel, dim3(1), dim3(1), 0, s, *t, n, ds, da, dp);
    if (hipGetLastError() != hipSuccess) rc = GBP_E_HIP;
  }
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = GBP_E_HIP;
  return rc;
}

}  // namespace

extern "C" {

int gbp_stream_create(int device, gbp_stream *out) {
  if (!out) return GBP_E_INVALID_ARG;
  DeviceGuard g(device);
  hipStream_t s = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *out = (gbp_stream)s;
  return GBP_OK;
}

int gbp_stream_destroy(gbp_stream stream) {
  if (stream) HIPCHK(hipStreamDestroy((hipStream_t)stream));
  return GBP_OK;
}

int gbp_tree_create(int device, int64_t capacity, gbp_tree **out) {
  if (!out || capacity < 1 || capacity > 0x7FFFFFFF) return GBP_E_INVALID_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GBP_E_NO_DEVICE;
  if (device < 0 || device >= ndev) return GBP_E_INVALID_ARG;
  DeviceGuard g(device);
  gbp_tree *t = new (std::nothrow) gbp_tree();
  if (!t) return GBP_E_ALLOC;
  t->device = device;
  if (hipMalloc(&t->count, 4) != hipSuccess || hipMalloc(&t->hm, 64) != hipSuccess ||
      tree_alloc(t, capacity) != GBP_OK) {
    gbp_tree_destroy(t);
    return GBP_E_ALLOC;
  }
  // the zeroing runs on the null stream, and the caller's planner streams are
  // non-blocking (gbp_stream_create): it must be complete before this returns,
  // or it can land after gbp_tree_init's count = 1 on another stream (seen as
  // a root overwritten by the first append under two processes per GPU)
  if (hipMemset(t->count, 0, 4) != hipSuccess || hipMemset(t->hm, 0, 64) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    gbp_tree_destroy(t);
    return GBP_E_HIP;
  }
  *out = t;
  return GBP_OK;
}

int gbp_tree_destroy(gbp_tree *t) {
  if (!t) return GBP_E_BAD_HANDLE;
  DeviceGuard g(t->device);
  (void)hipDeviceSynchronize();
  tree_free_arrays(t);
  if (t->hm) (void)hipFree(t->hm);
  if (t->count) (void)hipFree(t->count);
  if (t->rv) (void)hipFree(t->rv);
  delete t;
  return GBP_OK;
}

int gbp_tree_reserve(gbp_tree *t, int64_t capacity, gbp_stream stream) {
  if (!tree_ok(t)) return GBP_E_BAD_HANDLE;
  if (capacity <= t->cap) return GBP_OK;
  if (capacity > 0x7FFFFFFF) return GBP_E_SHAPE;
  DeviceGuard g(t->device);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipStreamSynchronize(s));
  gbp_tree grown = *t;
  const int rc = tree_alloc(&grown, capacity);
  if (rc) return rc;
  bool ok = true;
  for_each_tree_array([&](auto m, const TreeArray &A) {
    for (int k = 0; k < A.copied; k++)
      ok = ok && hipMemcpyAsync((char *)(grown.*m) + A.part_offset(k, grown.cap),
                                (const char *)(t->*m) + A.part_offset(k, t->cap), A.row * t->cap,
                                hipMemcpyDeviceToDevice, s) == hipSuccess;
  });
  if (!ok || hipStreamSynchronize(s) != hipSuccess) {
    // the tree keeps its old arrays, valid; the new ones go once no copy is in flight
    (void)hipDeviceSynchronize();
    tree_free_arrays(&grown);
    return GBP_E_HIP;
  }
  tree_free_arrays(t);
  *t = grown;
  return GBP_OK;
}

int gbp_tree_init(gbp_tree *t, const double *root, gbp_stream stream) {
  if (!tree_ok(t)) return GBP_E_BAD_HANDLE;
  if (!root) return GBP_E_INVALID_ARG;
  DeviceGuard g(t->device);
  hipLaunchKernelGGL(k_tree_init, dim3(1), dim3(1), 0, (hipStream_t)stream, *t, root[0], root[1],
                     root[2], root[3], root[4], root[5], root[6], root[7]);
  HIPCHK(hipGetLastError());
  return GBP_OK;
}

int gbp_tree_size(gbp_tree *t, int64_t *count, gbp_stream stream) {
  if (!tree_ok(t)) return GBP_E_BAD_HANDLE;
  if (!count) return GBP_E_INVALID_ARG;
  DeviceGuard g(t->device);
  int32_t c = 0;
  HIPCHK(hipMemcpyAsync(&c, t->count, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  *count = c;
  return GBP_OK;
}

int gbp_tree_capacity(gbp_tree *t, int64_t *capacity) {
  if (!tree_ok(t)) return GBP_E_BAD_HANDLE;
  if (!capacity) return GBP_E_INVALID_ARG;
  *capacity = t->cap;
  return GBP_OK;
}

int gbp_tree_read(gbp_tree *t, int64_t first, int64_t n, double *states, double *actions,
                  int32_t *parents, double *g, gbp_stream stream) {
  if (!tree_ok(t)) return GBP_E_BAD_HANDLE;
  if (first < 0 || n < 0 || first + n > t->cap) return GBP_E_INVALID_ARG;
  if (n == 0) return GBP_OK;
  DeviceGuard gd(t->device);
  hipStream_t s = (hipStream_t)stream;
  int rc = GBP_OK;
  if (!rc && states) rc = d2h(states, t->v + 8 * first, 8 * n, s);
  if (!rc && actions) rc = d2h(actions, t->a + 10 * first, 10 * n, s);
  if (!rc && parents) rc = d2h(parents, t->parent + first, n, s);
  if (!rc && g) rc = d2h(g, t->g + first, n, s);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(s));
  return GBP_OK;
}

int gbp_tree_read_links(gbp_tree *t, int64_t first, int64_t n, int32_t *child, int32_t *sibling,
                        int32_t *prev, gbp_stream stream) {
  if (!tree_ok(t)) return GBP_E_BAD_HANDLE;
  if (first < 0 || n < 0 || first + n > t->cap) return GBP_E_INVALID_ARG;
  if (n == 0) return GBP_OK;
  DeviceGuard gd(t->device);
  hipStream_t s = (hipStream_t)stream;
  int rc = GBP_OK;
  if (!rc && child) rc = d2h(child, t->child + first, n, s);
  if (!rc && sibling) rc = d2h(sibling, t->sibling + first, n, s);
  if (!rc && prev) rc = d2h(prev, t->prev + first, n, s);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(s));
  return GBP_OK;
}

int gbp_tree_append_host(gbp_tree *t, int64_t n, const double *states, const double *actions,
                         const int32_t *parents, gbp_stream stream) {
  if (!tree_ok(t)) return GBP_E_BAD_HANDLE;
  if (n < 0 || (n > 0 && (!states || !actions || !parents))) return GBP_E_INVALID_ARG;
  if (n == 0) return GBP_OK;
  int64_t c = 0;
  int rc = gbp_tree_size(t, &c, stream);
  if (rc) return rc;
  for (int64_t i = 0; i < n; i++)
    if (parents[i] < -1 || parents[i] >= c + i) return GBP_E_INVALID_ARG;
  const int64_t capacity = c + n > t->cap ? std::max<int64_t>(2 * t->cap, c + n) : t->cap;
  return tree_put_rows(t, capacity, k_tree_append, n, states, actions, parents, stream);
}

int gbp_tree_load_host(gbp_tree *t, int64_t n, const double *states, const double *actions,
                       const int32_t *parents, gbp_stream stream) {
  if (!tree_ok(t)) return GBP_E_BAD_HANDLE;
  if (n < 1 || n > 0x7FFFFFFE || !states || !actions || !parents || parents[0] != -1)
    return GBP_E_INVALID_ARG;
  // one tree rooted at 0: every parent in range, every vertex reached from the root
  {
    std::vector<int32_t> head(n, -1), next(n, -1), queue;
    for (int64_t i = 1; i < n; i++) {
      if (parents[i] < 0 || parents[i] >= n || parents[i] == i) return GBP_E_INVALID_ARG;
      next[i] = head[parents[i]];
      head[parents[i]] = (int32_t)i;
    }
    queue.reserve(n);
    queue.push_back(0);
    for (size_t h = 0; h < queue.size() && (int64_t)queue.size() <= n; h++)
      for (int32_t c = head[queue[h]]; c >= 0; c = next[c]) queue.push_back(c);
    if ((int64_t)queue.size() != n) return GBP_E_INVALID_ARG;
  }
  return tree_put_rows(t, n, k_tree_load, n, states, actions, parents, stream);
}

int gbp_tree_device_ptrs(gbp_tree *t, double **states, int32_t **count) {
  if (!tree_ok(t)) return GBP_E_BAD_HANDLE;
  if (states) *states = t->v;
  if (count) *count = t->count;
  return GBP_OK;
}

}  // extern "C"
