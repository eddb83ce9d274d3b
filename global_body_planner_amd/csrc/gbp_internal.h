// gbp_internal.h — definitions shared by the engine's translation units
// (gbp_engine.hip: terrain, lookups, pair checks, samplers, extend, NN;
// gbp_plan.hip: the device-resident planner loop's half-iteration and its
// workspace; gbp_nn.hip: the nearest-neighbour search in a device tree;
// gbp_star.hip: RRT*'s insertion; gbp_shortcut.hip: the connect table of
// found paths; gbp_tree.hip: the device tree handle;
// gbp_tree_maint.hip: a device tree pruned against a changed terrain,
// re-rooted at one of its vertices or grafted onto a root state that is none
// of them; gbp_tree_graft.hip: the graft's connect checks;
// gbp_tree_trim.hip: a device tree's trim flags by best cost or vertex budget;
// gbp_terrain.hip: a handle's heights updated in place, its window moved by
// whole cells and its host mirror;
// gbp_replan.hip: RRT*'s kept connections carried between searches and the
// joined path of two device trees;
// gbp_informed.hip: the handle's informed-sampling ellipse and its sampler;
// gbp_slopes.hip: a handle's slope layers derived from its heights): the handles, the block sizes, the device
// buffers' carve lists, and a tree's allocations and copies.
// Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "gbp.h"
#include "gbp_device.h"
#include "gbp_hrow.h"
#include "host/gbp_host_check.h"
#include "host/gbp_terrain_patch.h"

constexpr uint64_t GBP_EXTEND_STREAM = 0x45585444ull;  // "EXTD": newConfig's candidate stream
constexpr int WAVE = 64;
constexpr int TB = 256;   // threads of the grid-stride kernels
constexpr int CB = 1024;  // threads (items) per compaction tile

struct gbp_terrain {
  gbp_host::Terrain host;           // host copy (the values the device holds) for the
                                    // glibc re-decision of FRAGILE attempts
  int device = 0;
  int nx = 0, ny = 0;
  int storage = GBP_STORAGE_F64;
  double bounds[4] = {0, 0, 0, 0};
  double xNm = 0, yNm = 0;          // x[nx-2], y[ny-2]
  double inv_hx = 0, inv_hy = 0;
  int one_x = 0, one_y = 0;         // one-step bracket correction is exact (verified)
  double *d_x = nullptr, *d_y = nullptr;
  void *d_z = nullptr;
  double *d_dx = nullptr, *d_dy = nullptr, *d_dz = nullptr;
  int num_cus = 256;
  int64_t opt_kernel = GBP_KERNEL_PERSISTENT;
  int64_t opt_block = 0;            // GBP_OPT_BLOCK; 0: not set, the launch chooses (validate_block)
  int64_t opt_waves = 2;            // register budget of the validate kernels (waves/SIMD)
  int64_t opt_lds_coords = 1;       // stage the coordinate vectors in LDS when they fit
  int64_t opt_helpers = 1;          // idle lanes of a drained wave evaluate owners' next samples
  int64_t opt_affine = 1;           // compute coordinates when the affine form is exact
  int64_t opt_fast_rcp = 1;         // cell-area reciprocal by verified Newton steps
  double rcp_seed = 0;              // verified_rcp_seed (0: every spacing pair not exact)
  int nan_free = 0;                 // no height of `host` is NaN: scanned at create, kept by
                                    // every write of the mirror (gbp_patch::nan_free_after);
                                    // launches read it through nan_free_now
  int64_t opt_nan_tests = 0;        // GBP_OPT_NAN_TESTS: 1 = the general state check always
  double fragile_eps = gbp::FRAGILE_EPS;  // GBP_OPT_FRAGILE_EPS (>= the default)
  int64_t opt_xcd_map = 0;          // persistent kernel: slices numbered XCD-major
  int opt_nn_stats = 0;             // 1: the matrix-core NN search counts its fp64 re-checks
  gbp_sampling sampling{};          // direction-biased sampling (gbp_terrain_set_sampling), off
  gbp_informed informed{};          // informed sampling's ellipse (gbp_terrain_set_informed), off
  int affine = 0;                   // host-verified affine coordinates (both axes)
  int bx = 0, by = 0;
  double ax = 0, hx = 0, ay = 0, hy = 0;
  size_t lds_max = 65536;           // LDS bytes a workgroup may use
  hipStream_t host_stream = nullptr;
  void *ws = nullptr;               // grow-only device workspace
  size_t ws_bytes = 0;
  // extend-candidate workspaces, one per stream: _dev calls on one handle may
  // run concurrently on different streams without sharing scratch
  struct StreamWs {
    hipStream_t stream;
    void *ptr;
    size_t bytes;
  };
  std::vector<StreamWs> cand_ws;
  // what gbp_terrain_update_dev wrote that `host` has not taken in yet
  // (host_mirror), one entry per caller stream: the union of that stream's
  // rectangles and the event recorded behind its last apply launch
  struct PendingPatch {
    hipStream_t stream;
    gbp_patch::Rect rect;
    hipEvent_t done;
  };
  std::vector<PendingPatch> pending;
  float last_shift_ms = -1.0f;      // device time of the last move's shift launch (-1: none)
  int64_t opt_derive = 0;           // GBP_OPT_DERIVE_SLOPES: 0 off, else 1 | flags
};

// brings t->host up to date with the device (gbp_terrain.hip): waits for the
// pending updates' events, reads the union of their rectangles in one copy
// and scatters it
int gbp_internal_mirror_sync(gbp_terrain *t);

// The host copy of the heights, for the glibc re-decisions: every read of
// t->host goes through here.  With no device update pending it is a flag
// test; null when bringing the copy up to date failed (a HIP error).
inline const gbp_host::Terrain *host_mirror(gbp_terrain *t) {
  if (!t->pending.empty() && gbp_internal_mirror_sync(t) != GBP_OK) return nullptr;
  return &t->host;
}

// The map the device holds has no NaN height (GBP_OPT_NAN_FREE): true of the
// mirror, and the mirror is up to date.  gbp_terrain_update_dev writes values
// the host has not seen, so from that call until the mirror takes them in
// (host_mirror, gbp_terrain_read_host) this reads 0; no read-back is added to
// the update for it.
inline bool nan_free_now(const gbp_terrain *t) { return t->nan_free && t->pending.empty(); }

#define HIPCHK(expr)                      \
  do {                                    \
    hipError_t e_ = (expr);               \
    if (e_ != hipSuccess) return GBP_E_HIP; \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

template <class ZT>
inline gbp::TerrainView<ZT> view(const gbp_terrain *t) {
  gbp::TerrainView<ZT> v;
  v.x = t->d_x;
  v.y = t->d_y;
  v.z = (const ZT *)t->d_z;
  v.dx = t->d_dx;
  v.dy = t->d_dy;
  v.dz = t->d_dz;
  v.nx = t->nx;
  v.ny = t->ny;
  v.x0 = t->bounds[0];
  v.xN = t->bounds[1];
  v.y0 = t->bounds[2];
  v.yN = t->bounds[3];
  v.xNm = t->xNm;
  v.yNm = t->yNm;
  v.inv_hx = t->inv_hx;
  v.inv_hy = t->inv_hy;
  v.one_x = t->one_x;
  v.one_y = t->one_y;
  v.affine = t->affine;
  v.bx = t->bx;
  v.by = t->by;
  v.ax = t->ax;
  v.hx = t->hx;
  v.ay = t->ay;
  v.hy = t->hy;
  v.rcp_seed = t->opt_fast_rcp ? t->rcp_seed : 0.0;
  v.feps = t->fragile_eps;
  return v;
}

inline unsigned grid_for(int64_t n, int block, int cap = 65535 * 8) {
  int64_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

inline int ensure_ws(void **ws, size_t *have, size_t need) {
  if (*have >= need) return GBP_OK;
  if (*ws) (void)hipFree(*ws);
  *ws = nullptr;
  *have = 0;
  size_t sz = std::max(need, (size_t)1 << 20);
  if (hipMalloc(ws, sz) != hipSuccess) {
    *ws = nullptr;
    return GBP_E_ALLOC;
  }
  *have = sz;
  return GBP_OK;
}

// Device arrays stated once, as a list of take calls (a callable over a
// Stage &), 256-byte aligned in the order written.  The list runs twice:
// against a null base (the sizing pass: only `off` advances) for the byte
// count the buffer is allocated with, then against that buffer, which it may
// not outgrow (a take past `cap` yields null and stage_carve reports it).
struct Stage {
  char *base = nullptr;  // null: the sizing pass
  size_t cap = 0, off = 0;
  template <class T>
  void take(T *&p, size_t count) {
    off = (off + 255) & ~(size_t)255;
    p = base && off + count * sizeof(T) <= cap ? (T *)(base + off) : nullptr;
    off += count * sizeof(T);
  }
};
template <class F>
size_t stage_bytes_of(F &carve) {
  Stage S;
  carve(S);
  return S.off;
}
template <class F>
int stage_carve(void *buf, size_t cap, F &carve) {
  Stage S{(char *)buf, cap};
  carve(S);
  return S.off <= cap ? GBP_OK : GBP_E_ALLOC;
}
// the list carved from a device buffer of its own, freed at scope exit
struct DevBuf {
  void *p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};
template <class F>
int stage_buf(DevBuf &b, F carve) {
  const size_t need = stage_bytes_of(carve);
  if (hipMalloc(&b.p, need) != hipSuccess) {
    b.p = nullptr;
    return GBP_E_ALLOC;
  }
  return stage_carve(b.p, need, carve);
}

// ============================================================================
// the planner's handles (gbp_tree.hip creates, fills and frees the trees,
// gbp_plan.hip the workspace, whose RRT* block is gbp_star.hip's;
// gbp_tree_maint.hip replaces a tree's arrays; gbp_replan.hip reads the trees
// and the kept connections)
// ============================================================================
struct gbp_tree {
  int device = 0;
  int64_t cap = 0;
  double *v = nullptr;        // [cap][8] vertex states (GraphClass vertices)
  _Float16 *vh = nullptr;     // [cap][NH_ROW] fp16 split rows (matrix-core search, nn_put_hrow)
  float *hm = nullptr;        // [16]: [0, 8) max |64 v[j][k]|, [8] (bits) 1 = a row outside fp16
  double *a = nullptr;        // [cap][10] the action that reached each vertex
  double *g = nullptr;        // [cap] cost to come: g[parent] + poseDistance
  int32_t *parent = nullptr;  // [cap], -1 at the root
  // successor lists (graph_class.cpp:28-58 successors_), first child / next
  // sibling: the RRT*-Connect rewiring updates g over a rewired vertex's
  // subtree (graph_class.cpp:131-138); kept by every append (child order is
  // immaterial: a child's g depends on its parent's alone)
  int32_t *child = nullptr, *sibling = nullptr;  // [cap], -1 = none
  int32_t *prev = nullptr;    // [cap] previous sibling (-1: first child): O(1) removeEdge
  int32_t *bfs = nullptr;     // [2 cap] scratch: the subtree update's two level queues
  int32_t *count = nullptr;   // [1] number of vertices (device resident)
  // gbp_tree_revalidate_dev's attempt rows, gbp_tree_trim_flags_dev's f and counts
  // (grow-only; a kernel gets pointers carved from it, never these two)
  void *rv = nullptr;
  size_t rv_bytes = 0;
};

inline bool tree_ok(const gbp_tree *t) { return t && t->v && t->count; }

__device__ __forceinline__ void copy8(double *d, const double *s) {
#pragma unroll
  for (int k = 0; k < 8; k++) d[k] = s[k];
}

__device__ __forceinline__ void copy10(double *d, const double *s) {
#pragma unroll
  for (int k = 0; k < 10; k++) d[k] = s[k];
}

// The tree's capacity-sized allocations, stated once, in allocation order;
// tree_alloc, gbp_tree_reserve's copies and frees and gbp_tree_destroy all go
// through this list (count and hm are gbp_tree_create's and
// gbp_tree_destroy's own).  An allocation holds `parts` sub-arrays of
// [capacity] rows back to back, so a sub-array's offset depends on the
// capacity; a reserve carries the first `copied` of them over, the rest is
// scratch.
struct TreeArray {
  size_t row;         // bytes per vertex of one sub-array
  int parts = 1;
  int copied = 1;
  int64_t round = 1;  // rows allocated: the capacity rounded up to a multiple
  size_t bytes(int64_t cap) const { return row * parts * (size_t)((cap + round - 1) / round * round); }
  size_t part_offset(int k, int64_t cap) const { return row * k * (size_t)cap; }
};
template <class F>
inline void for_each_tree_array(F f) {
  f(&gbp_tree::v, TreeArray{64});
  f(&gbp_tree::a, TreeArray{80});
  f(&gbp_tree::g, TreeArray{8});
  f(&gbp_tree::parent, TreeArray{4});
  // child | sibling | prev | bfs[2]: the successor lists survive a reserve,
  // the subtree update's two level queues are scratch
  f(&gbp_tree::child, TreeArray{4, 5, 3});
  // the fp16 rows in whole 64-row units (nh_sweep loads a unit's rows past the
  // tree's end and masks their scores)
  f(&gbp_tree::vh, TreeArray{2 * NH_ROW, 1, 1, 64});
}

inline void tree_free_arrays(gbp_tree *t) {
  for_each_tree_array([&](auto m, const TreeArray &) {
    if (t->*m) (void)hipFree(t->*m);
    t->*m = nullptr;
  });
}

// fresh arrays of `cap` rows in *t (what it held before is the caller's to
// free); on failure nothing is allocated and *t is unchanged
inline int tree_alloc(gbp_tree *t, int64_t cap) {
  gbp_tree n = *t;
  for_each_tree_array([&](auto m, const TreeArray &) { n.*m = nullptr; });
  bool ok = true;
  for_each_tree_array([&](auto m, const TreeArray &A) {
    if (ok && hipMalloc(&(n.*m), A.bytes(cap)) != hipSuccess) {
      n.*m = nullptr;
      ok = false;
    }
  });
  if (!ok) {
    tree_free_arrays(&n);
    return GBP_E_ALLOC;
  }
  n.sibling = n.child + cap;
  n.prev = n.child + 2 * cap;
  n.bfs = n.child + 3 * cap;
  n.cap = cap;
  *t = n;
  return GBP_OK;
}

template <class T>
inline int d2h(T *dst, const T *src, size_t count, hipStream_t s) {
  HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, s));
  return GBP_OK;
}
template <class T>
inline int h2d(T *dst, const T *src, size_t count, hipStream_t s) {
  HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, s));
  return GBP_OK;
}

// the segment scans k_nn_hreduce lists (a fourth unit of a segment within
// the threshold: the segment's rows in fp64) and their merge; one set for the
// caller's stream, one for the look-ahead stream
constexpr int NSC_CAP = 16384;  // listed scans per search (more: scanned in the reduce)
constexpr int NSC_UNITS = NSC_CAP * 8;  // (scan, part) results: NSC_CAP x NSC_P
struct NsBuf {
  uint32_t cap;             // list capacity (NSC_CAP; GBP_NSC_CAP lowers it: tests)
  int2 *list;               // (query, segment)
  uint32_t *cnt;            // listed
  double *ed;               // [NSC_UNITS] a scan part's minimum
  int32_t *ei;              // ... its index (lowest at that minimum)
  double *hd;               // [bmax] the reduce's own answer
  int32_t *hi;
  int2 *qh;                 // [bmax] a query's first entry and its entries
};

// the search's share of the planner workspace (gbp_plan_ws::nnw): sized by
// nn_ws_init, carved from the workspace's block by nn_ws_carve, its counters
// zeroed by nn_ws_zero (gbp_nn.h)
struct NnWs {
  int stats = 0;               // GBP_OPT_NN_STATS: k_nn_hreduce counts its re-checks in the status
  int items = 4096;            // matrix-core search: work items (= waves) per launch
  // the partials: NN_MAX_CHUNKS * bmax slots, pd[c * nq + qi]
  // (d2 / i2: the look-ahead search's, on its own stream)
  double *d = nullptr, *d2 = nullptr;
  int32_t *i = nullptr, *i2 = nullptr;
  // the direct search for a few queries (k_nn_small): per-workgroup partials
  // and the completion count of its last-workgroup reduce
  double *ns_d = nullptr;
  int32_t *ns_i = nullptr;
  uint32_t *ns_fin = nullptr;
  int ns_grid = 1;             // its workgroups (one per CU of an XCD)
  int64_t ns_capq = 0;         // queries its partials hold (ns_grid x ns_capq slots)
  NsBuf nsb[2] = {};           // k_nn_scan's lists: the caller's stream, the look-ahead's
};

// the look-ahead search's device state (gbp_plan_ws::la), by half % 3 (the
// drawn-ahead target sets) and by parity (the searched trees' snapshots)
struct gbp_plan_la {
  int32_t nt[3];     // valid targets drawn for the half (ordered_rank's total)
  uint32_t frag[3];  // half + 1 when one of its draws was FRAGILE
  int32_t nv[2];     // the searched tree's vertex count when its search was launched
  uint32_t go[2];    // 0: the sequence had stopped when the search was launched (it idles)
};

struct gbp_plan_ws {
  int device = 0;
  int num_cus = 256;
  int64_t bmax = 0;            // largest batch of draws per half-iteration
  gbp_plan_status *st = nullptr;
  unsigned long long *tiles = nullptr;  // look-back tile states
  uint32_t epoch = 0;          // per-compaction tag of the tile states
  uint64_t seq = 0;            // launch sequence number of the planner kernels (gated())
  int64_t ntiles = 0;
  // stage 0-1: three sets, by half % 3 (with the look-ahead search, half
  // h + 2's targets are drawn while half h + 1's are searched and half h
  // still reads its own); cand..tqh point at the set of the half being
  // enqueued or resolved (select_targets)
  struct TargetSet {
    double *cand, *targets;
    uint32_t *cflag;
    _Float16 *tqh;
  } tset[3] = {};
  double *cand = nullptr;      // [bmax][8] drawn states
  uint32_t *cflag = nullptr;   // [bmax] their isValidState flags
  double *targets = nullptr;   // [bmax][8] the valid ones, in draw order
  _Float16 *tqh = nullptr;     // [bmax][NH_ROW] their fp16 rows (k_nn_mfma's queries)
  // stage 2-3; nn, cs and ca in two sets by the half's parity (the
  // look-ahead search of half h + 1 writes its own while half h reads)
  int32_t *nn = nullptr;       // [bmax] nearest vertex of T per target
  double *cs = nullptr;        // [6 bmax][8] candidate s_near
  double *ca = nullptr;        // [6 bmax][10] candidate actions
  int32_t *nnp[2] = {};
  double *csp[2] = {}, *cap[2] = {};
  double *csn = nullptr;       // [6 bmax][8] candidate s_new
  uint32_t *cf = nullptr;      // [6 bmax] candidate flags
  uint32_t *cc = nullptr;      // [6 bmax] candidate counts
  int32_t *eres = nullptr;     // [bmax] extend result
  int32_t *echo = nullptr;     // [bmax] chosen candidate
  double *esn = nullptr;       // [bmax][8]
  double *ean = nullptr;       // [bmax][10]
  uint32_t *ef = nullptr;      // [bmax] extend flags
  int32_t *evtx = nullptr;     // [bmax] new vertex index (or -1)
  // stage 4-5
  int32_t *nno = nullptr;      // [bmax] nearest vertex of O per new vertex
  int32_t *kres = nullptr;     // [bmax] connect result
  double *ksn = nullptr;       // [bmax][8]
  double *kan = nullptr;       // [bmax][10]
  uint32_t *kf = nullptr;      // [bmax] connect flags
  NnWs nnw;                    // the searches' partials, lists and knobs (gbp_nn.hip)
  // the look-ahead search (gbp_plan_halves_dev): half h + 1's targets drawn
  // and searched on la_stream while half h's extends, connects and appends
  // run on the caller's stream (la_go: main -> side, la_done: side -> main)
  gbp_plan_la *la = nullptr;   // device: counts, snapshots, flags
  unsigned long long *la_tiles = nullptr;  // look-back tiles of the drawn-ahead targets
  hipStream_t la_stream = nullptr;
  hipEvent_t la_go = nullptr, la_done = nullptr;
  void *block = nullptr;       // the one allocation all of the above live in
  // RRT*-Connect (gbp_plan_star_config; star = 0: RRT-Connect): stages 6-7
  int star = 0;
  double star_delta = 3.0;     // rrt_star_connect.h:59
  int64_t star_max_pairs = 0, star_max_shared = 0;
  int64_t star_items = 0;      // scan items per half (new vertex x position chunk)
  int star_grid = 0;           // count / fill / check workgroups cap (GBP_STAR_GRID, tests; 0: none)
  int64_t star_ch = 1024;      // map positions per scan item before growth (STAR_CH)
  int32_t star_lds[3] = {-1, -1, -1};  // the replay's LDS limits (GBP_STAR_LDS, tests; -1: RP, RK, RQ)
  // a half's insertion buffers, one set per tree (half & 1): half h's replay
  // runs on star_stream beside half h's connects and half h + 1, which fills
  // the other set; half h + 2 refills this one only after the replay (its
  // stage 5 waits for it first)
  struct StarSet {
    unsigned long long *scnt = nullptr;  // [star_items] neighbours per scan item (k_star_count: tile_word)
    int32_t *sioff = nullptr;    // [star_items] the items' offsets
    int32_t *soff = nullptr;     // [bmax + 1] each new vertex's first pair
    int32_t *snb = nullptr;      // [max_pairs] the neighbour of each pair
    int32_t *sown = nullptr;     // [max_pairs] its new vertex (k)
    int32_t *srowof = nullptr;   // [2 max_pairs] connect check -> pair-check row (-1: none)
    double *srs = nullptr;       // [2 max_pairs][8] rows: the pair checks' states
    double *sra = nullptr;       // [2 max_pairs][10] and actions
    uint32_t *srf = nullptr;     // [2 max_pairs] their flags
    int64_t *meta = nullptr;     // [4] n_added, added_base, pairs (k_star_count's scan); shared count (stage-5 append)
    uint32_t *sfin = nullptr;    // [64] k_star_count's finished-workgroup count (zeroed, self-resetting)
  } ss[2];
  int32_t *kvtx = nullptr;     // [bmax] O's vertex of each connection (-1: none)
  // the replay (and the best connection's ranking) off the caller's stream:
  // e6 (stage 6 done) and e5 (stage 5 done) main -> star, rdone[k] star -> main
  // (tree k's last replay / ranking), sdone the call's join
  hipStream_t star_stream = nullptr;
  hipEvent_t star_e6 = nullptr, star_e5 = nullptr, star_rdone[2] = {nullptr, nullptr},
             star_sdone = nullptr;
  // gbp_plan_stage_timing: a ring of per-half timing events (start, after
  // stage 3, after stage 6, replay start / end, end), read back once complete
  bool timing = false;
  struct TimedHalf {
    hipEvent_t ev[8] = {};  // + [6] after stage 6's connect actions, [7] after their pair checks
    bool pending = false, star = false;
    int32_t half = 0;
  };
  TimedHalf *tring = nullptr;  // [ntring] (a plain array: no template of a gbp type exported)
  size_t ntring = 0, tnext = 0;
  double tsum[7] = {0, 0, 0, 0, 0, 0, 0};
  int64_t tcount = 0;
  int32_t *sshared = nullptr;  // [max_shared][2] the REACHED connections (a, b)
  void *star_block = nullptr;
  // gbp_replan.hip's scratch (the list's second buffer, the compaction's tile
  // counts and offsets, its control record): grow-only, sized by
  // star_max_shared when an entry first needs it; host side only, no kernel
  // of gbp_plan.hip takes it
  void *replan = nullptr;
  size_t replan_bytes = 0;
};

// a function one translation unit defines for another: never exported
#define GBP_INTERNAL __attribute__((visibility("hidden")))

// ascending with no NaN (fast_terrain_map.cpp:101-108), n >= 2: what
// gbp_terrain_create and gbp_terrain_move_host accept as a coordinate vector
inline bool coords_ascending(const double *d, int n) {
  for (int i = 0; i + 1 < n; i++)
    if (!(d[i] <= d[i + 1])) return false;
  return true;
}

// What a handle derives from its coordinate vectors x[t->nx], y[t->ny] (both
// coords_ascending), in one place for gbp_terrain_create and
// gbp_terrain_move_host (gbp_engine.hip): bounds, xNm / yNm, inv_h*, one_x /
// one_y, the affine fit, rcp_seed, the device copies d_x / d_y and the
// mirror's x / y.  All or nothing: on failure (GBP_E_ALLOC, GBP_E_HIP) the
// handle is as it was.
GBP_INTERNAL int gbp_internal_set_geometry(gbp_terrain *t, const double *x, const double *y);

// The derive launch alone, on st (gbp_slopes.hip), for gbp_terrain.hip's
// upkeep under GBP_OPT_DERIVE_SLOPES: the nodes of `launch` (inside the map)
// that lie in `inner` get the rule of gbp_slopes.h, the others (0, 0, 1).
// Heights from the x-pairs zp, coordinates from the device vectors x / y,
// results into lay[3]: the handle's own buffers or a move's second set.
// status: null, or an update's check word (1 = write nothing).
GBP_INTERNAL int gbp_internal_derive_slopes(const gbp_terrain *t, const void *zp, const double *x,
                                            const double *y, double *const lay[3],
                                            const gbp_patch::Rect &launch,
                                            const gbp_patch::Rect &inner, int flags,
                                            const int32_t *status, hipStream_t st);

// the device's look-ahead stream of the planner loop (created once per
// process and device; null on failure); gbp_plan.hip
hipStream_t gbp_internal_la_stream(int device, int num_cus);

// RRT*'s part of a half-iteration, enqueued by gbp_plan.hip's enqueue_stages
// (gbp_star.hip; th: the half's timing slot or null).  Stage 6 on s: the
// neighbourhoods, the connect checks and their pair checks.
template <class ZT>
GBP_INTERNAL int star_enqueue_checks(gbp_terrain *t, gbp_plan_ws *w, gbp_tree *T, int32_t half,
                                     int direction, int adaptive, gbp_plan_ws::TimedHalf *th,
                                     hipStream_t s);
// stage 7 on star_stream behind what s holds: the ordered replay into T
// (tree kT: Ta 0, Tb 1)
GBP_INTERNAL int star_enqueue_replay(gbp_plan_ws *w, gbp_tree *T, int32_t half, int kT,
                                     gbp_plan_ws::TimedHalf *th, hipStream_t s);
// after Tb's half, on star_stream behind s's stage 5: the kept connections
// ranked with the trees' current g (ga: Ta's, gb: Tb's)
GBP_INTERNAL int star_enqueue_rank(gbp_plan_ws *w, int32_t half, int kT, const double *ga,
                                   const double *gb, hipStream_t s);
// the workspace's side stream and its events released (gbp_plan.hip's ws_free)
GBP_INTERNAL void star_stream_destroy(gbp_plan_ws *w);

// the persistent validate kernel with the batch size read on the device from
// n_dev (n_max bounds the grid); gbp_engine.hip
int gbp_internal_validate_dev_n(gbp_terrain *t, int64_t n_max, const int *n_dev, const double *s,
                                const double *a, const uint8_t *dir, int dir_all, int adaptive,
                                uint8_t *valid, double *s_new, double *t_new, uint32_t *flags,
                                uint32_t *counts, hipStream_t st);

