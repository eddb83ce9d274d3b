/*
 * gbp.h — C ABI of the MI355X batched RRT-Connect extend/validity engine.
 *
 * This is the drop-in boundary for the hot path of LiuShenLan/global_body_planner
 * (reference snapshot 2025-02-04).  Every entry point below replaces one reference
 * C++ interface; the reference file:line it stands in for is cited on each.
 *
 *   - plain C: opaque handles, int status codes (GBP_OK = 0, < 0 = error), no
 *     exceptions cross this boundary, no torch / HIP types in the signatures
 *     (a stream is passed as an opaque `void*` = hipStream_t, NULL = default).
 *   - State  = double[8]  {x, y, z, dx, dy, dz, p, dp}   (planning_utils.h:57-61)
 *   - Action = double[10] {a_x_td, a_y_td, a_z_td, a_x_to, a_y_to, a_z_to,
 *                          t_s, t_f, a_p_td, a_p_to}     (planning_utils.h:58-62)
 *     Batches are AoS `double[n][8]` / `double[n][10]`, i.e. exactly the
 *     std::array layout, so a std::vector<State> can be passed as-is.
 *   - All arithmetic is IEEE FP64 in the reference operation order, compiled
 *     without FMA contraction, so decisions are bit-exact with the reference
 *     algorithm (see DESIGN.md "Parity").
 *   - `_dev` entry points take DEVICE pointers and enqueue on `stream`
 *     (asynchronous); `_host` entry points take host pointers and block.
 *   - A handle is used by one host thread at a time; there is no global mutable
 *     state, so distinct handles (e.g. one per GPU) are fully reentrant.
 */
#ifndef GBP_H
#define GBP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define GBP_OK              0
#define GBP_E_INVALID_ARG  (-1)
#define GBP_E_BAD_HANDLE   (-2)
#define GBP_E_ALLOC        (-3)
#define GBP_E_HIP          (-4)
#define GBP_E_SHAPE        (-5)
#define GBP_E_NO_DEVICE    (-6)
#define GBP_E_UNSUPPORTED  (-7)

/* ---- reference enums (planning_utils.h:50-54, rrt.h:7-9) ---------------- */
#define GBP_FLIGHT          0
#define GBP_STANCE          1
#define GBP_CONNECT_STANCE  2
#define GBP_FORWARD         0
#define GBP_REVERSE         1
#define GBP_TRAPPED         0
#define GBP_ADVANCED        1
#define GBP_REACHED         2

#define GBP_STATE_DIM       8
#define GBP_ACTION_DIM     10
#define GBP_NUM_GEN_STATES  6   /* planning_utils.h:45 */
/* attemptConnect (rrt_connect.cpp:20-84) recurses without a bound; the
 * engine stops a connection after this many levels and reports it TRAPPED
 * (counted as depth_capped).  Each level's stance time shrinks by >= one
 * KINEMATICS_RES step except in degenerate reverse cases, so a cap of 1024
 * covers t_s up to 51 s (a 38 m connect at V_NOM) without truncation.      */
#define GBP_CONNECT_MAX_DEPTH 1024

/* ---- per-attempt flag word (output of the validate/extend entry points) -- */
#define GBP_F_VALID      (1u << 0)  /* the pair check returned true                      */
#define GBP_F_OOD        (1u << 1)  /* a lookup whose reference result is UB (point outside
                                       [x_0,x_{N-1}) x [y_0,y_{N-1}), fast_terrain_map.cpp:96-117)
                                       was reached; by this engine's convention the state is
                                       invalid (DESIGN.md "Out-of-domain convention")       */
#define GBP_F_NAN        (1u << 2)  /* a state failed on a NaN terrain cell                 */
#define GBP_F_SNEW_SET   (1u << 3)  /* the reference assigned s_new (else buffer untouched) */
#define GBP_F_TNEW_SET   (1u << 4)  /* the reference assigned t_new (else buffer untouched) */
#define GBP_F_FRAGILE    (1u << 5)  /* a trig-dependent comparison was within 1e-12 of its
                                       threshold (decision could differ across libm builds) */
#define GBP_F_LIMIT      (1u << 6)  /* the pair needed more than GBP_MAX_SAMPLES state checks
                                       (t_s + t_f > ~350 s, e.g. a connect longer than ~262 m at
                                       V_NOM, or t_s = inf where the reference never
                                       terminates); the check is stopped and reported invalid.
                                       The cap keeps G = 9 V below the 16-bit counter field. */
#define GBP_F_RESOLVED   (1u << 7)  /* a FRAGILE attempt whose outputs were re-decided on the
                                       host with glibc trig (gbp_resolve_fragile_host)        */
#define GBP_MAX_SAMPLES  7000u
#define GBP_F_DEPTH_CAPPED (1u << 12) /* a connect stopped at GBP_CONNECT_MAX_DEPTH (TRAPPED) */
#define GBP_F_STAGE_SHIFT 8u        /* bits 8..11: stage in which the check ended          */
#define GBP_F_STAGE_MASK  (0xFu << GBP_F_STAGE_SHIFT)
#define GBP_STAGE_FWD_STANCE 1u     /* planning_utils.cpp:718-730 */
#define GBP_STAGE_FWD_FLIGHT 2u     /* :735-741 */
#define GBP_STAGE_FWD_LAND   3u     /* :743-749 */
#define GBP_STAGE_REV_FLIGHT 4u     /* :842-847 */
#define GBP_STAGE_REV_STANCE 5u     /* :852-863 */
#define GBP_STAGE_REV_START  6u     /* :866-872 */

/* lookup counters: counts[i] = G | (V << 16), G = executed getGroundHeight calls,
   V = executed isValidState calls (reference semantics).         */
#define GBP_COUNT_G(c) ((c) & 0xFFFFu)
#define GBP_COUNT_V(c) ((c) >> 16)

/* ---- opaque handles ------------------------------------------------------ */
typedef struct gbp_terrain gbp_terrain;
typedef void *gbp_stream; /* hipStream_t; NULL = the device's null stream */

/* ---- library / device ---------------------------------------------------- */
int         gbp_version(void);                 /* 10000*major + 100*minor + patch */
const char *gbp_status_string(int status);
int         gbp_device_count(int *count);
int         gbp_device_alloc(int device, size_t bytes, void **ptr);
int         gbp_device_free(void *ptr);
int         gbp_memcpy_h2d(void *dst, const void *src, size_t bytes, gbp_stream stream);
int         gbp_memcpy_d2h(void *dst, const void *src, size_t bytes, gbp_stream stream);
int         gbp_stream_synchronize(gbp_stream stream);

/* ---- terrain (replaces FastTerrainMap storage + loadData,
 *      fast_terrain_map.h:97-118, fast_terrain_map.cpp:10-28) -------------- */
#define GBP_STORAGE_AUTO 0  /* fp32 if every z value round-trips through float, else fp64 */
#define GBP_STORAGE_F32  1  /* lossless for grid_map-sourced maps (fast_terrain_map.cpp:60) */
#define GBP_STORAGE_F64  2

/* x[nx], y[ny] ascending coordinates; z, dx, dy, dz are x-major [nx][ny]
 * (z[ix*ny + iy] == z_data_[ix][iy]).  dx/dy/dz may be NULL => (0, 0, 1),
 * as loadDataFromGridMap does for maps without slope layers (:70-74). */
int gbp_terrain_create(int device, int nx, int ny, const double *x, const double *y,
                       const double *z, const double *dx, const double *dy,
                       const double *dz, int storage, gbp_terrain **out);
int gbp_terrain_destroy(gbp_terrain *t);
/* bounds = {x_0, x_{N-1}, y_0, y_{M-1}} (the getXData().front()/back() values) */
int gbp_terrain_info(const gbp_terrain *t, int *nx, int *ny, int *storage,
                     double bounds[4], int *device);

/* ---- a terrain's heights updated in place ----------------------------------
 * The node loads every new map into the same FastTerrainMap
 * (global_body_planner.cpp:37-44).  An update replaces the heights (and, when
 * given, the slope layers) of a rectangle of cells, or of the whole map, of a
 * living handle.  Geometry, storage type, options, sampling, workspaces and
 * the gbp_plan_ws objects created for the handle are untouched: afterwards the
 * handle is bit for bit what gbp_terrain_create would have made of the patched
 * map with the same storage and options.  An update never changes the storage
 * type: a changed size or storage type stays a new gbp_terrain_create (a window
 * of the same size moved by whole cells is gbp_terrain_move_host, below). */
typedef struct gbp_rect { int32_t ix0, iy0, nx, ny; } gbp_rect; /* cells [ix0, ix0+nx) x [iy0, iy0+ny); NULL = whole map */
#define GBP_SRC_F64_XMAJOR  0  /* double src[i*ld + j] = z[ix0+i][iy0+j], ld >= rect.ny */
#define GBP_SRC_F32_GRIDMAP 1  /* a whole grid_map layer as it lies in memory: float,
                                  column-major, start index 0, ld >= terrain nx;
                                  z[ix][iy] = src[(NX-1-ix) + (NY-1-iy)*ld]
                                  (fast_terrain_map.cpp:57-61); the rect selects which
                                  cells are taken */
/* z, and dx / dy / dz (all three or none), in src_layout with leading dimension
 * ld.  Slope layers given for a handle created without them: GBP_E_INVALID_ARG;
 * omitted for a handle that has them: they stay as they are (or are derived
 * again from the heights: GBP_OPT_DERIVE_SLOPES, below).  A rectangle that
 * is empty or leaves the map, or an ld below the layout's minimum: GBP_E_SHAPE;
 * an unknown layout: GBP_E_INVALID_ARG.
 * All or nothing: an fp32-storage handle holds only heights that round-trip
 * through float, and an update keeps that true.  An fp64 source height that is
 * neither NaN nor float-representable rejects the whole update, slope layers
 * included, and nothing is written.  gbp_terrain_update_host finds that on the
 * host before it stages anything and returns GBP_E_UNSUPPORTED.
 * gbp_terrain_update_dev cannot: its first launch checks the patch and writes
 * status[0] (device, one word: 0 applied, 1 rejected), its second applies the
 * patch unless it reads 1; the call itself returns GBP_OK.  A GBP_SRC_F32_GRIDMAP
 * source and an fp64-storage handle cannot be rejected (status[0] = 0; status
 * may then be NULL).  NaN heights are stored as NaN.
 * Ordering: gbp_terrain_update_dev takes DEVICE pointers and only enqueues on
 * `stream`, like every _dev entry: work enqueued on that stream before it sees
 * the old map, work enqueued after it the new one.  Ordering against work on
 * any other stream (the handle's own host stream of the _host entries
 * included) is the caller's.  gbp_terrain_update_host takes host pointers, runs
 * on the handle's host stream after every earlier gbp_terrain_update_dev, and
 * returns when the device and the host copy hold the patch. */
int gbp_terrain_update_dev(gbp_terrain *t, const gbp_rect *r, int src_layout, int64_t ld,
                           const void *z, const void *dx, const void *dy, const void *dz,
                           int32_t *status, gbp_stream stream);
int gbp_terrain_update_host(gbp_terrain *t, const gbp_rect *r, int src_layout, int64_t ld,
                            const void *z, const void *dx, const void *dy, const void *dz);
/* The heights the device holds, x-major z[r.nx][r.ny] (host, synchronous, after
 * every earlier gbp_terrain_update_dev).  A height lies in up to two places
 * (slot 0 of x-pair ix, slot 1 of x-pair ix-1): copy 0 reads row ix from slot 0
 * of pair ix (row nx-1, which has none, from slot 1 of pair nx-2), copy 1 reads
 * row ix from slot 1 of pair ix-1 (row 0 from slot 0 of pair 0). */
int gbp_terrain_read_host(gbp_terrain *t, const gbp_rect *r, int copy, double *z);

/* ---- a terrain's window moved by whole cells --------------------------------
 * A robot-centred elevation map scrolls by whole cells as the robot moves
 * (grid_map's move): the map keeps its size, its coordinates are displaced and
 * only a strip of its heights is new.  gbp_terrain_move_host gives a living
 * handle that new geometry: x[nx], y[ny] are the new coordinate vectors (the
 * handle's sizes, ascending as at create), and new cell (ix, iy) holds what old
 * cell (ix + sx, iy + sy) held where that cell lies in the old map (the
 * overlap, shifted on the device).  Every other new cell (the strips: |sx| full
 * rows and |sy| columns of the remaining rows) takes its height, and when dx /
 * dy / dz are given its slope values, from the source, which is the WHOLE new
 * map in src_layout: GBP_SRC_F64_XMAJOR z[ix*ld + iy] with ld >= ny,
 * GBP_SRC_F32_GRIDMAP as above.  Only the strips' cells are read and staged; a
 * value in the overlap's part of the source is never looked at.
 * The shift is the caller's statement: the old and new coordinates are not
 * compared (grid_map recomputes positions from the new centre, and they may
 * differ from the displaced old ones in the last ulp).  |sx| >= nx or |sy| >=
 * ny leaves no overlap: the whole map comes from the source.  sx = sy = 0 only
 * replaces the coordinate vectors (z may then be NULL).
 * Afterwards the handle is bit for bit what gbp_terrain_create makes of x, y
 * and the moved arrays with the same storage and options: heights in both
 * copies of every x-pair, slope layers, bounds, everything derived from the
 * coordinates (the coordinate class may change, e.g. affine to not affine, and
 * GBP_OPT_COORD_MODE with it), the host copy and GBP_OPT_NAN_FREE.  Options,
 * sampling, workspaces and the gbp_plan_ws objects of the handle stay.
 * Slope layers given to a handle created without them: GBP_E_INVALID_ARG.
 * Omitted for a handle that has them: the overlap's slope values shift with the
 * heights and the strips' slope cells become (0, 0, 1), what a create without
 * layers reads everywhere (with GBP_OPT_DERIVE_SLOPES on: the layers of the
 * moved map are derived whole from its heights and the new coordinates).
 * All or nothing: descending coordinates or a NaN among them:
 * GBP_E_INVALID_ARG; an ld below the layout's minimum: GBP_E_SHAPE; an
 * fp32-storage handle and a strip height that is neither NaN nor
 * float-representable: GBP_E_UNSUPPORTED, found on the host before anything is
 * staged.  The moved map is built in a second set of device buffers, which
 * replace the handle's own as the last step together with the host-side fields,
 * so a failure at any point leaves the handle as it was.  The old buffers are
 * then freed: between moves the handle holds one copy of the map.
 * Ordering: as gbp_terrain_update_host.  The entry runs on the handle's host
 * stream behind every earlier gbp_terrain_update_dev, whose rectangles the host
 * copy takes in first, and returns when the device and the host copy hold the
 * moved map.  Work of the caller's on other streams that reads the handle must
 * have finished.  There is no _dev form: a launch's view of the terrain (the
 * buffers, the bounds and the other coordinate-derived scalars) is built from
 * host fields when the launch is enqueued, so a move ordered on a caller's
 * stream would need another design. */
int gbp_terrain_move_host(gbp_terrain *t, int64_t sx, int64_t sy, const double *x,
                          const double *y, int src_layout, int64_t ld, const void *z,
                          const void *dx, const void *dy, const void *dz);
/* Device time (ms, by events on the handle's host stream) of the shift launch of
 * the last gbp_terrain_move_host that succeeded; -1 when there was none or it
 * launched none (sx = sy = 0, or no overlap and no slope layers).  For
 * tools/terrain_move_ab.py. */
int gbp_terrain_move_shift_ms(const gbp_terrain *t, float *ms);
/* Is the coordinate vector new_c[n] the vector old_c[n] displaced by a whole
 * number of cells (no device call)?  h = (old_c[n-1] - old_c[0]) / (n - 1),
 * *shift = round((new_c[0] - old_c[0]) / h); returns 1 when every new position
 * with an old counterpart, new_c[i] against old_c[i + *shift], lies within
 * h * rel_tol of it (none has one when |*shift| >= n: 1), else 0 with *shift
 * untouched: a changed spacing, a displacement by a fraction of a cell, n < 2,
 * NaN.  FastTerrainMap::moveFromGridMap calls it with rel_tol = 1.0 / 1024. */
int gbp_coord_shift(const double *old_c, const double *new_c, int n, double rel_tol, int *shift);

/* ---- a terrain's slope layers derived from its heights ----------------------
 * The maps a node receives from a sensor pipeline carry an elevation layer and
 * no slope layers.  These entries compute dx / dy / dz on the device from the
 * heights the handle holds (csrc/gbp_slopes.h, the recipe of
 * terrain_data.synth_fractal).  For node (ix, iy) and each axis (x shown, m =
 * ix - 1, p = ix + 1; a neighbour is usable when it lies in the map and its
 * height is not NaN):
 *   both usable   g = (z_p - z_m) / (x_p - x_m)
 *   only p        g = (z_p - z_c) / (x_p - x_c)
 *   only m        g = (z_c - z_m) / (x_c - x_m)
 *   neither       g = 0.0
 * then l = sqrt((gx*gx + gy*gy) + 1.0) and (dx, dy, dz) = ((-gx)/l, (-gy)/l,
 * 1.0/l).  A node whose own height is NaN gets (0, 0, 1).  Heights are read as
 * the handle stores them (fp32 storage widened to double).  With
 * GBP_SLOPES_F32 each component is rounded through float last, what a grid_map
 * layer would hold.  Any other flag bit: GBP_E_INVALID_ARG. */
#define GBP_SLOPES_F32 2
/* Recomputes the slope cells of the nodes in r (NULL: the whole map); reads one
 * node beyond r on each side where the map has one.  Ordered on `stream` like
 * gbp_terrain_update_dev; it only enqueues and cannot allocate, so a handle
 * without slope layers is GBP_E_INVALID_ARG.  Rectangle errors as
 * gbp_terrain_update_*.  The heights do not change, so the call leaves nothing
 * for the host copy and is NOT among the device updates that the _host entries
 * wait for: before gbp_terrain_read_slopes_host, gbp_terrain_derive_slopes_host
 * or any other _host entry that reads or writes the layers, the caller
 * synchronises `stream` (ordering against other streams is the caller's, as
 * for every _dev entry). */
int gbp_terrain_derive_slopes_dev(gbp_terrain *t, const gbp_rect *r, int flags, gbp_stream stream);
/* The same on the handle's host stream behind every earlier
 * gbp_terrain_update_dev, synchronous.  A handle created without slope layers
 * gets them here: (0, 0, 1) outside r, derived inside.  If it fails at any
 * point the handle is as it was. */
int gbp_terrain_derive_slopes_host(gbp_terrain *t, const gbp_rect *r, int flags);
/* The slope layers the device holds, each x-major [r.nx][r.ny] (host,
 * synchronous, after every earlier gbp_terrain_update_dev and the derive launch
 * it enqueued under GBP_OPT_DERIVE_SLOPES; not after a
 * gbp_terrain_derive_slopes_dev, see there): the counterpart of
 * gbp_terrain_read_host.  A handle without layers: GBP_E_INVALID_ARG. */
int gbp_terrain_read_slopes_host(gbp_terrain *t, const gbp_rect *r, double *dx, double *dy,
                                 double *dz);

/* engine options (per handle) */
#define GBP_OPT_KERNEL        1  /* GBP_KERNEL_* for the validate/extend entry points */
#define GBP_OPT_BLOCK         2  /* threads per workgroup (multiple of 64, <= 512; the
                                    direct kernel uses min(block, 256)); default 256.
                                    Until it is set (or once it is set to 0 again) the
                                    persistent kernel's launch runs 128 lanes where
                                    2 * waves such workgroups fit a CU's LDS with their
                                    coordinate vectors: GBP_OPT_LAUNCH_BLOCK           */
/* keys 3, 6, 7, 11, 12 (grid size, dynamic work sources, chunking, prefix,
   oversubscription) were measured slower than static per-wave slices and removed */
#define GBP_OPT_WAVES         4  /* register budget: min waves per SIMD (2..4)        */
#define GBP_OPT_LDS_COORDS    5  /* 1: stage coordinate vectors in LDS when they fit  */
#define GBP_OPT_HELPERS       8  /* 1: a drained wave's idle lanes evaluate the remaining
                                    attempts' next samples ahead (default 1)          */
#define GBP_OPT_AFFINE_COORDS 9  /* 1 (default): compute grid coordinates when the host
                                    verified x[i] == a + h*(i - b) bit for bit         */
#define GBP_OPT_COORD_MODE   10  /* read-only: 2 computed, 1 LDS-staged, 0 global      */
#define GBP_OPT_XCD_MAP      13  /* 1 = each XCD takes one contiguous eighth of the batch
                                    (workgroup b runs on XCD b % 8): for batches the
                                    caller ordered by position                         */
#define GBP_OPT_FAST_RCP     14  /* 1 (default): the bilinear 1/((x2-x1)(y2-y1)) by two
                                    Newton steps when gbp_terrain_create verified them
                                    bit-exact for every spacing pair; get: 1 = in use   */
#define GBP_OPT_FRAGILE_EPS  15  /* the FRAGILE margin in units of 1e-15 (default 1000 =
                                    1e-12, the smallest accepted): a wider margin flags
                                    and re-decides more attempts on the host, with the
                                    same results (tests use it to force host resolutions) */
/* 16, 17, 19: retired (round 4) — a Morton-sorted nearest-neighbour index, the
   packed fp32 VALU filter and a two-stream draw overlap, each measured no
   faster than the default path; setting them is an error     */
#define GBP_OPT_NN_STATS     18  /* 1: the matrix-core search counts its fp64 re-checks
                                    in gbp_plan_status.stat_nn_* (diagnostics: costs
                                    same-address atomics; default 0)                  */
#define GBP_OPT_LAUNCH_BLOCK 20  /* read-only: threads per workgroup of the next
                                    persistent validate launch at the current options:
                                    GBP_OPT_BLOCK where the caller set it, else 128 or
                                    256 by the rule above                              */
#define GBP_OPT_REFILL_WINDOW 19 /* read-only, always 0: the persistent validate kernel's
                                    LDS prefetch window is retired; rows are
                                    prefetched into registers where they fit            */
#define GBP_OPT_NAN_FREE     21  /* read-only: 1 = the host has verified that no height
                                    of the map is NaN (at create, kept by every
                                    gbp_terrain_update_host), so the persistent validate
                                    kernel runs the state check without its NaN tests
                                    and centre lookup: same results.  0 from a
                                    gbp_terrain_update_dev until the host copy has taken
                                    its values in (the next host re-decision or
                                    gbp_terrain_read_host)                             */
#define GBP_OPT_NAN_TESTS    22  /* 1: always run the general state check, whatever
                                    GBP_OPT_NAN_FREE reads (A/B runs, tests); default 0 */
#define GBP_OPT_DERIVE_SLOPES 23 /* 0 (default): off.  1 | flags (flags: GBP_SLOPES_F32):
                                    gbp_terrain_update_dev / _update_host / _move_host
                                    calls given NO slope layers keep the layers derived
                                    from the heights.  An update re-derives its
                                    rectangle and the nodes next to it (update_dev on
                                    the same stream behind its apply launch, skipped
                                    with a rejected patch); after a move the layers are
                                    those of a whole-map derivation of the moved map
                                    with its new coordinates.  Calls given layers write
                                    them as before.  Should the derive launch of a
                                    gbp_terrain_update_host itself fail (a HIP launch
                                    error), the call returns that error with the
                                    heights updated on the device and in the host copy
                                    and the layers of the rectangle as they were.
                                    Setting it launches nothing; a
                                    handle without slope layers: GBP_E_INVALID_ARG (run
                                    gbp_terrain_derive_slopes_host first)              */
#define GBP_KERNEL_DIRECT     0  /* one lane per attempt                              */
#define GBP_KERNEL_PERSISTENT 1  /* persistent waves, lanes re-packed per sample      */
int gbp_terrain_set_option(gbp_terrain *t, int key, int64_t value);
int gbp_terrain_get_option(const gbp_terrain *t, int key, int64_t *value);
/* The LDS a persistent validate launch would request for an nx x ny terrain
 * with straight-line brackets (no device needed): `block` threads per
 * workgroup (0: GBP_OPT_BLOCK not set, the launch's own choice), `waves` per SIMD, `lds_max` bytes a workgroup may use.  Outputs
 * (each may be NULL): coord_lds 1 when the coordinate vectors are staged in
 * LDS, window 0 (the refill's LDS prefetch window is retired; the argument
 * stays for callers), bytes the dynamic LDS of the launch. */
int gbp_validate_lds_plan(int nx, int ny, int64_t block, int64_t waves, size_t lds_max,
                          int *coord_lds, int *window, size_t *bytes);

/* ---- batched terrain queries ---------------------------------------------
 * FastTerrainMap::getGroundHeight + heightIsNan (fast_terrain_map.cpp:94-157)
 * xy[n][2] in; height[n], is_nan[n], ood[n] out (any output may be NULL).
 * An ood point gets height NaN and is_nan 1 (reference: undefined). */
int gbp_height_batch_dev(gbp_terrain *t, int64_t n, const double *xy, double *height,
                         uint8_t *is_nan, uint8_t *ood, gbp_stream stream);
int gbp_height_batch_host(gbp_terrain *t, int64_t n, const double *xy, double *height,
                          uint8_t *is_nan, uint8_t *ood);
/* FastTerrainMap::getSurfaceNormal (fast_terrain_map.cpp:160-213): normal[n][3] */
int gbp_normal_batch_dev(gbp_terrain *t, int64_t n, const double *xy, double *normal,
                         uint8_t *ood, gbp_stream stream);
int gbp_normal_batch_host(gbp_terrain *t, int64_t n, const double *xy, double *normal,
                          uint8_t *ood);

/* ---- state validity (planning_utils::isValidState, planning_utils.cpp:562-635)
 * states[n][8], phase[n] (or NULL => phase_all) -> valid[n], flags[n], counts[n] */
int gbp_valid_states_dev(gbp_terrain *t, int64_t n, const double *states,
                         const uint8_t *phase, int phase_all, uint8_t *valid,
                         uint32_t *flags, uint32_t *counts, gbp_stream stream);
int gbp_valid_states_host(gbp_terrain *t, int64_t n, const double *states,
                          const uint8_t *phase, int phase_all, uint8_t *valid,
                          uint32_t *flags, uint32_t *counts);

/* ---- THE HOT PATH: batched state-action pair checks ----------------------
 * planning_utils::isValidStateActionPair / isValidStateActionPairReverse
 * (+ the AdaptiveStepSize variants when adaptive != 0),
 * planning_utils.cpp:645-881.
 *   s[n][8], a[n][10]; direction[n] (GBP_FORWARD / GBP_REVERSE) or NULL =>
 *   direction_all.  Outputs (any may be NULL except flags):
 *   valid[n]      the returned bool
 *   s_new[n][8]   written ONLY where the reference assigns s_new (GBP_F_SNEW_SET),
 *                 otherwise the caller's contents are left untouched, exactly
 *                 like the reference's in/out reference parameter
 *   t_new[n]      likewise (GBP_F_TNEW_SET)
 *   flags[n]      GBP_F_* word
 *   counts[n]     G | V << 16                                               */
int gbp_validate_pairs_dev(gbp_terrain *t, int64_t n, const double *s, const double *a,
                           const uint8_t *direction, int direction_all, int adaptive,
                           uint8_t *valid, double *s_new, double *t_new, uint32_t *flags,
                           uint32_t *counts, gbp_stream stream);
int gbp_validate_pairs_host(gbp_terrain *t, int64_t n, const double *s, const double *a,
                            const uint8_t *direction, int direction_all, int adaptive,
                            uint8_t *valid, double *s_new, double *t_new, uint32_t *flags,
                            uint32_t *counts);

/* ---- counter-based samplers (Philox4x32-10, keyed (seed, stream, index)) ---
 * Identical draws regardless of batching / device count.  The distributions
 * are the reference's; its unseeded rand() / clock-seeded engines
 * (planning_utils.cpp:435, planner_class.cpp:51) are not reproducible, so the
 * engine defines its own reproducible streams.
 *
 * PlannerClass::randomState (planner_class.cpp:38-76), index i of stream.
 * If require_phase >= 0 the draw is repeated (k = 0..max_tries-1) until
 * isValidState(state, require_phase) holds; tries[i] = k+1 (or -1 if none). */
int gbp_sample_states_dev(gbp_terrain *t, int64_t n, uint64_t seed, uint64_t stream_id,
                          int64_t index_base, int require_phase, int max_tries,
                          double *states, int32_t *tries, gbp_stream stream);
int gbp_sample_states_host(gbp_terrain *t, int64_t n, uint64_t seed, uint64_t stream_id,
                           int64_t index_base, int require_phase, int max_tries,
                           double *states, int32_t *tries);
/* getRandomAction(surf_norm) (planning_utils.cpp:392-442) with rotate_grf
 * (:198-231): actions[n][10] from normals[n][3]; draw (stream_id, index_base+i). */
int gbp_sample_actions_dev(int64_t n, const double *normals, uint64_t seed,
                           uint64_t stream_id, int64_t index_base, double *actions,
                           gbp_stream stream);
int gbp_sample_actions_host(gbp_terrain *t, int64_t n, const double *normals, uint64_t seed,
                            uint64_t stream_id, int64_t index_base, double *actions);

/* ---- direction-biased sampling (ROS params state_direction_sampling/... and
 *      action_direction_sampling/..., config/params.yaml:21-27, forwarded by
 *      global_body_planner.cpp:193-205 to RRTClass::set_state_direction_sampling /
 *      set_action_direction_sampling, rrt.cpp:268-278).  Off by default, as in
 *      the reference.  The reference's coin is `rand()/RAND_MAX <= p`; the engine's
 *      is a Philox uniform of its own purpose (index, try) so both branches keep
 *      their counter-addressed draws. */
typedef struct {
  int32_t state_flag;            /* randomState -> randomStateDirection with probability state_p */
  int32_t state_speed_direction; /* speed_direction_flag: velocity heading = atan2(to - from) */
  double state_p;                /* probability_threshold */
  int32_t action_flag;           /* getRandomAction -> getRandomActionDirection with prob. action_p */
  int32_t reserved;
  double action_p;
} gbp_sampling;
/* The handle's sampling configuration (NULL = off): applied by every entry
 * point that draws newConfig's candidate actions (gbp_extend_batch_*,
 * gbp_extend_resolve_host, gbp_extend_tree_*) and by the device planner loop's
 * targets (gbp_plan_half_dev: s_from / s_to as rrt_connect.cpp:248-252, :283-287,
 * the trees' last vertices and roots when the half starts). */
int gbp_terrain_set_sampling(gbp_terrain *t, const gbp_sampling *cfg);
int gbp_terrain_get_sampling(const gbp_terrain *t, gbp_sampling *cfg);
/* PlannerClass::randomState(terrain, flag, p, speed_direction_flag, s_from, s_to)
 * (planner_class.cpp:22-35): index i of stream draws the coin, then either
 * randomStateDirection (:82-148: x, y uniform over the s_from / s_to rectangle,
 * heading atan2(to - from) when speed_direction) or randomState (:38-76) from
 * the same draws as gbp_sample_states_dev.  s_from[8], s_to[8] are HOST arrays;
 * cfg NULL = the handle's configuration. */
int gbp_sample_states_dir_dev(gbp_terrain *t, int64_t n, uint64_t seed, uint64_t stream_id,
                              int64_t index_base, const gbp_sampling *cfg, const double *s_from,
                              const double *s_to, double *states, gbp_stream stream);
int gbp_sample_states_dir_host(gbp_terrain *t, int64_t n, uint64_t seed, uint64_t stream_id,
                               int64_t index_base, const gbp_sampling *cfg, const double *s_from,
                               const double *s_to, double *states);
/* getRandomAction(surf_norm, direction, flag, p, s, s_near) (planning_utils.cpp:379-391):
 * the coin, then getRandomActionDirection(surf_norm, s_from, s_to) (:443-515,
 * FORWARD: s_near -> s, REVERSE: s -> s_near) or getRandomAction(surf_norm).
 * normals[n][3], s[n][8] (the state extended toward), s_near[n][8], direction[n]
 * (or NULL => direction_all); cfg NULL = the handle's configuration. */
int gbp_sample_actions_dir_dev(gbp_terrain *t, int64_t n, const double *normals, const double *s,
                               const double *s_near, const uint8_t *direction, int direction_all,
                               const gbp_sampling *cfg, uint64_t seed, uint64_t stream_id,
                               int64_t index_base, double *actions, gbp_stream stream);
int gbp_sample_actions_dir_host(gbp_terrain *t, int64_t n, const double *normals, const double *s,
                                const double *s_near, const uint8_t *direction, int direction_all,
                                const gbp_sampling *cfg, uint64_t seed, uint64_t stream_id,
                                int64_t index_base, double *actions);

/* ---- informed sampling: targets inside the best cost's ellipse -------------
 * Path cost is a sum of poseDistance (3-D) and a 2-D distance never exceeds
 * the 3-D one, so a state on a path shorter than c between the two trees'
 * roots A and B satisfies |p.xy - A.xy| + |p.xy - B.xy| < c: an ellipse in xy
 * with foci A.xy, B.xy and major axis c, a superset of the 3-D informed set.
 * Off by default: the reference draws over the whole map. */
typedef struct {
  int32_t active;    /* 0: draws are the plain sampler's */
  int32_t reserved;
  double cost;       /* c */
  double cx, cy;     /* centre */
  double ux, uy;     /* unit vector focus a -> focus b in xy; (1, 0) when they coincide */
  double a, b;       /* semi-axes */
} gbp_informed;
/* The ellipse of two foci and a cost (host, no device call); focus_a, focus_b:
 * at least [2] (x, y); bounds = gbp_terrain_info's {x_0, x_N-1, y_0, y_M-1}.
 * binary64, each step its own rounding:
 *   dx = bx - ax; dy = by - ay; d = sqrt(dx*dx + dy*dy);
 *   ux = d > 0 ? dx / d : 1; uy = d > 0 ? dy / d : 0;
 *   cx = (ax + bx) * 0.5; cy = (ay + by) * 0.5;
 *   a = cost * 0.5; w = cost*cost - d*d; b = w > 0 ? sqrt(w) * 0.5 : 0;
 *   active = cost < INFINITY && (MY_PI * a) * b < (bounds[1]-bounds[0]) * (bounds[3]-bounds[2])
 * (uniform draws in the ellipse beat uniform draws in the map exactly when the
 * ellipse is the smaller; MY_PI is the planner's 3.14159).  cost = +inf:
 * active 0 with the other fields filled; cost below d: b = 0, the segment
 * between the foci.  GBP_E_INVALID_ARG for a null pointer, a NaN among the four
 * focus coordinates, a NaN cost or cost <= 0 (*out untouched). */
int gbp_informed_ellipse(const double *focus_a, const double *focus_b, double cost,
                         const double bounds[4], gbp_informed *out);
/* The handle's ellipse (NULL = off), per handle like gbp_sampling: applied to
 * the device planner loop's targets (gbp_plan_half_dev, gbp_plan_halves_dev;
 * a half with `active` set runs the inline sequence, without the look-ahead
 * search) and to the host planner's.  GBP_E_INVALID_ARG for an active ellipse
 * with a NaN field or a negative semi-axis. */
int gbp_terrain_set_informed(gbp_terrain *t, const gbp_informed *inf);
int gbp_terrain_get_informed(const gbp_terrain *t, gbp_informed *inf);
/* Index i of stream with gbp_sample_states_dir_dev's draws (one try, the same
 * eight uniforms of PURPOSE_STATE) and arguments; where the coin does not pick
 * the direction draw and inf->active is set, x and y are uniform over the
 * ellipse instead of the map:
 *   r = sqrt(u00); th = (2.0 * MY_PI) * u01; (si, co) = sincos(th);
 *   ex = (a * r) * co; ey = (b * r) * si;
 *   x = cx + (ux * ex - uy * ey); y = cy + (uy * ex + ux * ey);
 * height (NaN outside the map: such a state is GBP_F_OOD to the state check),
 * velocity, pitch and q[7] as gbp_sample_states_dev forms them.  active = 0:
 * gbp_sample_states_dir_dev's draws bit for bit.  cfg, inf NULL = the
 * handle's; s_from, s_to may be NULL when cfg's state_flag is off. */
int gbp_sample_states_informed_dev(gbp_terrain *t, int64_t n, uint64_t seed, uint64_t stream_id,
                                   int64_t index_base, const gbp_sampling *cfg,
                                   const gbp_informed *inf, const double *s_from,
                                   const double *s_to, double *states, gbp_stream stream);
int gbp_sample_states_informed_host(gbp_terrain *t, int64_t n, uint64_t seed, uint64_t stream_id,
                                    int64_t index_base, const gbp_sampling *cfg,
                                    const gbp_informed *inf, const double *s_from,
                                    const double *s_to, double *states);

/* ---- batched extend (RRTClass::newConfig + the acceptance half of
 *      RRTClass::extend, rrt.cpp:20-102) --------------------------------------
 * For extend i: s_near[i] (the nearest vertex, found by gbp_nearest_batch),
 * target[i] (the state the tree is extended towards).  Candidate action j
 * (j = 0..5) is getRandomAction(getSurfaceNormal(target)) drawn from stream
 * (seed, extend_base + i, j) — with the handle's gbp_sampling, the reference's
 * getRandomAction(surf_norm, direction, flag, p, target, s_near) (rrt.cpp:34, :49)
 * as gbp_sample_actions_dir_dev; candidates are checked (forward or reverse by
 * direction) and the LOWEST valid j is taken — the sequential newConfig.
 * result[i] = TRAPPED / ADVANCED / REACHED (isWithinBounds(s_new, target));
 * chosen[i] = j or -1; s_new[i], a_new[i] written when result != TRAPPED.   */
int gbp_extend_batch_dev(gbp_terrain *t, int64_t n, const double *s_near,
                         const double *target, const uint8_t *direction,
                         int direction_all, int adaptive, uint64_t seed,
                         int64_t extend_base, int32_t *result, int32_t *chosen,
                         double *s_new, double *a_new, uint32_t *counts,
                         uint32_t *flags, gbp_stream stream);
/* (flags[i]: OR of the executed candidates' VALID / OOD / NAN / FRAGILE / LIMIT
 *  bits; a FRAGILE extend is re-decided by gbp_extend_resolve_host.  The _host
 *  variant does that itself: its outputs are final.) */
int gbp_extend_batch_host(gbp_terrain *t, int64_t n, const double *s_near,
                          const double *target, const uint8_t *direction,
                          int direction_all, int adaptive, uint64_t seed,
                          int64_t extend_base, int32_t *result, int32_t *chosen,
                          double *s_new, double *a_new, uint32_t *counts,
                          uint32_t *flags);

/* ---- FRAGILE attempts: the host re-decision ---------------------------------
 * The kernels form isValidState's rotation without libm; where a decision's
 * margin is below 1e-12 (a height within 1e-12 of H_MIN / H_MAX, a lookup
 * point within 1e-12 of a grid line) the attempt is flagged GBP_F_FRAGILE,
 * because glibc's atan2 / cos / sin (the reference's) could decide it the
 * other way.  These entry points re-run exactly the flagged entries on the
 * host with glibc and the reference's expressions (planning_utils.cpp
 * :562-881, compiled without FMA like the reference) and overwrite their
 * outputs; flags get GBP_F_RESOLVED (FRAGILE cleared).  Host pointers; the
 * _host entry points above call them already, the _dev entry points leave it
 * to the caller.  Entries the host check does not assign keep the buffer's
 * contents.  n_resolved (may be NULL) = how many were re-decided. */
int gbp_resolve_fragile_host(gbp_terrain *t, int64_t n, const double *s, const double *a,
                             const uint8_t *direction, int direction_all, int adaptive,
                             uint8_t *valid, double *s_new, double *t_new, uint32_t *flags,
                             uint32_t *counts, int64_t *n_resolved);
int gbp_resolve_fragile_states_host(gbp_terrain *t, int64_t n, const double *states,
                                    const uint8_t *phase, int phase_all, uint8_t *valid,
                                    uint32_t *flags, uint32_t *counts, int64_t *n_resolved);
/* newConfig + acceptance (rrt.cpp:20-101) re-decided for every extend whose
 * flags carry GBP_F_FRAGILE (same arguments as gbp_extend_batch_dev, host
 * pointers): the six candidate actions are regenerated on the device from
 * the same stream, then checked in order with the glibc pair check. */
int gbp_extend_resolve_host(gbp_terrain *t, int64_t n, const double *s_near, const double *target,
                            const uint8_t *direction, int direction_all, int adaptive,
                            uint64_t seed, int64_t extend_base, int32_t *result, int32_t *chosen,
                            double *s_new, double *a_new, uint32_t *counts, uint32_t *flags,
                            int64_t *n_resolved);

/* ---- nearest neighbour (PlannerClass::getNearestNeighbor,
 *      planner_class.cpp:185-200) ----------------------------------------------
 * vertices[n_vert][8] (device-resident SoA-free flat tree), queries[n_q][8];
 * index[i] = argmin_v stateDistance(query_i, v) with ties to the LOWEST index
 * (the reference ties to unordered_map iteration order). */
int gbp_nearest_batch_dev(int64_t n_query, const double *queries, int64_t n_vert,
                          const double *vertices, int32_t *index, double *dist,
                          gbp_stream stream);
int gbp_nearest_batch_host(int64_t n_query, const double *queries, int64_t n_vert,
                           const double *vertices, int32_t *index, double *dist);

/* ---- radius neighbourhood (PlannerClass::neighborhoodDist,
 *      planner_class.cpp:173-182; used by RRT*-Connect, rrt_star_connect.cpp:28)
 * out[i][0..max_out): the vertices with 0 < stateDistance(query_i, v) <= radius
 * in the order the reference's vertex map holding keys 0..n_vert-1 iterates
 * them (gbp_vertex_map_order); count[i] = how many there are (entries beyond
 * max_out are not written). */
int gbp_neighbors_batch_dev(int64_t n_query, const double *queries, int64_t n_vert,
                            const double *vertices, double radius, int max_out, int32_t *out,
                            int32_t *count, gbp_stream stream);
int gbp_neighbors_batch_host(int64_t n_query, const double *queries, int64_t n_vert,
                             const double *vertices, double radius, int max_out, int32_t *out,
                             int32_t *count);

/* ---- the reference vertex map's iteration order ------------------------------
 * GraphClass stores a tree's vertices in std::unordered_map<int, State>
 * (graph_class.h:155) filled with keys 0, 1, ... (graph_class.cpp:28-31) and
 * neighborhoodDist / RRT*'s choose-parent and rewire loops follow its iteration
 * order (planner_class.cpp:176-179, rrt_star_connect.cpp:31-64).  The order is
 * libstdc++'s (GCC 11.4): out[n] = the keys 0..n-1 as iterated; *rank = the
 * position of `key` (0 <= key < n).  Host functions, no device needed. */
int gbp_vertex_map_order(int64_t n, int32_t *out);
int gbp_vertex_map_rank(int64_t key, int64_t n, int64_t *rank);

/* ---- k nearest (PlannerClass::neighborhoodN, planner_class.cpp:151-171) ----
 * out[i][0..k), k = min(n_nearest, n_vert): the vertices of smallest
 * stateDistance(query_i, v) in the order the reference pops its min-heap of
 * std::pair<double, int> — ascending distance, equal distances by ascending
 * index; a NaN distance orders after every number.  dist[i][...] (may be NULL)
 * their distances; entries k .. n_nearest-1 are -1 / NaN.  1 <= n_nearest <=
 * GBP_KNN_MAX.  The reference's cost_add_yaw variant: gbp_knn_yaw_batch_dev. */
#define GBP_KNN_MAX 64
int gbp_knn_batch_dev(int64_t n_query, const double *queries, int64_t n_vert,
                      const double *vertices, int n_nearest, int32_t *out, double *dist,
                      gbp_stream stream);
int gbp_knn_batch_host(int64_t n_query, const double *queries, int64_t n_vert,
                       const double *vertices, int n_nearest, int32_t *out, double *dist);

/* neighborhoodN with cost_add_yaw set (planner_class.cpp:151-171 with
 * stateDistance(q, v, true, lw, yw), planning_utils.h:146-155): the order key
 * is poseDistance(q, v) * length_weight + stateYawDistance(q, v) * yaw_weight,
 * ordered as gbp_knn_batch_dev.  The yaws atan2(s[4], s[3]) are the caller's
 * (query_yaw[n_query], vertex_yaw[n_vert], glibc's bits: no device atan2
 * reproduces them); the _host entry forms them with glibc itself. */
int gbp_knn_yaw_batch_dev(int64_t n_query, const double *queries, const double *query_yaw,
                          int64_t n_vert, const double *vertices, const double *vertex_yaw,
                          double length_weight, double yaw_weight, int n_nearest, int32_t *out,
                          double *dist, gbp_stream stream);
int gbp_knn_yaw_batch_host(int64_t n_query, const double *queries, int64_t n_vert,
                           const double *vertices, double length_weight, double yaw_weight,
                           int n_nearest, int32_t *out, double *dist);
/* atan2(s[4], s[3]) with glibc (the reference's yaw of a state, planning_utils.h:135) */
double gbp_host_yaw(const double *state);

/* ---- streams ------------------------------------------------------------ */
int gbp_stream_create(int device, gbp_stream *out);  /* a non-blocking HIP stream */
int gbp_stream_destroy(gbp_stream stream);

/* ---- device-resident trees (GraphClass / PlannerClass storage,
 *      graph_class.cpp:28-77, planner_class.cpp) ------------------------------
 * A tree lives in HBM as SoA arrays: states [cap][8], the action that reached
 * each vertex [cap][10], parent [cap] (-1 at the root), g [cap] (cost to come,
 * g[parent] + poseDistance, graph_class.cpp:36-42), and its vertex count, kept
 * on the device so that kernels append to it without a host round trip.  The
 * yaw cost y (stateYawDistance, an atan2) is left to the host, which computes
 * it along the returned path with glibc, as the reference does. */
typedef struct gbp_tree gbp_tree;
typedef struct gbp_plan_ws gbp_plan_ws;
int gbp_tree_create(int device, int64_t capacity, gbp_tree **out);
int gbp_tree_destroy(gbp_tree *tree);
/* GraphClass::init (graph_class.cpp:141-152): count = 1, vertex 0 = root */
int gbp_tree_init(gbp_tree *tree, const double *root, gbp_stream stream);
/* grows the arrays (contents kept); synchronises the stream */
int gbp_tree_reserve(gbp_tree *tree, int64_t capacity, gbp_stream stream);
int gbp_tree_capacity(gbp_tree *tree, int64_t *capacity);
int gbp_tree_size(gbp_tree *tree, int64_t *count, gbp_stream stream);  /* synchronous */
/* host copies of vertices [first, first + n); any output may be NULL (synchronous) */
int gbp_tree_read(gbp_tree *tree, int64_t first, int64_t n, double *states, double *actions,
                  int32_t *parents, double *g, gbp_stream stream);
/* the successor lists (graph_class.cpp:28-58 successors_) of vertices [first,
 * first + n) as the tree keeps them: child = a vertex's first child, sibling =
 * the next child of its parent, prev = the one before it, -1 = none (the order
 * within a list carries no meaning); any output may be NULL (synchronous) */
int gbp_tree_read_links(gbp_tree *tree, int64_t first, int64_t n, int32_t *child,
                        int32_t *sibling, int32_t *prev, gbp_stream stream);
/* appends n vertices (addVertex + addEdge + addAction) in order; g computed on
 * the device; parents may name vertices appended earlier in the same call */
int gbp_tree_append_host(gbp_tree *tree, int64_t n, const double *states, const double *actions,
                         const int32_t *parents, gbp_stream stream);
/* replaces the tree with n >= 1 given vertices: an RRT*-Connect tree, whose
 * rewiring gives vertices parents added after them (rrt_star_connect.cpp:55-62).
 * parents[0] = -1, every other parent in [0, n) and the whole a tree rooted at
 * vertex 0 (else GBP_E_INVALID_ARG, nothing changed); g is derived on the
 * device from the root down (graph_class.cpp:131-138 keeps g[c] = g[parent] +
 * poseDistance).  Synchronises the stream. */
int gbp_tree_load_host(gbp_tree *tree, int64_t n, const double *states, const double *actions,
                       const int32_t *parents, gbp_stream stream);
/* PlannerClass::getNearestNeighbor (planner_class.cpp:185-200) for n device
 * queries[n][8] against the tree (count read on the device): index[n], ties to
 * the lowest index like gbp_nearest_batch_dev.  Uses ws's status and scratch
 * (n <= its max_batch). */
int gbp_tree_nearest_dev(gbp_plan_ws *ws, gbp_tree *tree, int64_t n, const double *queries,
                         int32_t *index, gbp_stream stream);
/* the tree's device arrays (for gbp_nearest_batch_dev and the like): READ ONLY —
 * vertices are written through init / append only, which also keep the fp16
 * rows and magnitude bounds the matrix-core search relies on */
int gbp_tree_device_ptrs(gbp_tree *tree, double **states, int32_t **count);

/* ---- a tree against a changed terrain ---------------------------------------
 * The map reaches the reference node through a callback
 * (global_body_planner.cpp:37-44) and the node plans on it again; a tree grown
 * on the map before keeps the vertices that are still reachable on the new
 * one.  Edge (parent[i] -> i) of a tree grown in `direction` was inserted
 * because the pair check of (v[parent[i]], a[i], direction) was valid (extend,
 * rrt.cpp:77-102; the connect's last level, rrt_connect.cpp:20-91; the RRT*
 * rewire, rrt_star_connect.cpp:55-62): the edge is valid on terrain t when
 * that check is.  A vertex is kept when every edge between it and the root
 * is.  The root is never tested (a goal root may be FLIGHT-valid only:
 * callers test roots with gbp_valid_states_*), and v[i] is not compared with
 * the check's s_new: only the decision is used. */
typedef struct {
  int64_t n_before;        /* vertices of the tree before the prune            */
  int64_t n_kept;          /* ... and after it                                 */
  int64_t n_edge_invalid;  /* pruned vertices whose own edge failed            */
  int64_t n_inherited;     /* pruned only because an ancestor was              */
} gbp_prune_stats;
/* Stage A: the edges' decisions on terrain t.  n = the tree's size as the
 * caller knows it (gbp_tree_size); device edge_valid[n], flags[n]:
 * edge_valid[i] = the returned bool and flags[i] = the GBP_F_* word of vertex
 * i's edge, edge_valid[0] = 1, flags[0] = 0.  Enqueue-only on `stream`, with
 * one exception: the rows live in one buffer the tree owns, and a call that
 * finds it too small (the first, or one after the tree grew) frees and
 * allocates it, which synchronises the device.  Because of that buffer, two
 * calls on the same tree must not be in flight at once.  A FRAGILE edge is
 * left to the caller to re-decide.  GBP_E_SHAPE when n exceeds the tree's
 * capacity; when n is not the device's count the kernels read nothing of the
 * tree and report it as edge_valid[0] = 0 (gbp_tree_prune_dev then returns
 * GBP_E_SHAPE). */
int gbp_tree_revalidate_dev(gbp_terrain *t, gbp_tree *tree, int64_t n, int direction, int adaptive,
                            uint8_t *edge_valid, uint32_t *flags, gbp_stream stream);
/* Stage B: keeps the vertices whose edges up to the root all have
 * edge_valid = 1 (device edge_valid[n], [0] ignored), in their order: device
 * remap[n] = a vertex's new index or -1, the kept rows of v / a / g moved,
 * parent = remap[parent], the fp16 search rows and successor lists rebuilt,
 * the count set; device stats[1].  The rows go into fresh arrays that replace
 * the tree's, with a count and search bounds of their own (the capacity
 * stays; pointers from gbp_tree_device_ptrs are stale afterwards, as after a
 * reserve that grew the tree).  Synchronises the stream (before, to compare n
 * with the device's count: GBP_E_SHAPE when they differ; and after, to free
 * the old arrays).  The swap is the last step: a call that returns an error
 * leaves the tree as it was (remap and stats may have been written). */
int gbp_tree_prune_dev(gbp_tree *tree, int64_t n, const uint8_t *edge_valid, int32_t *remap,
                       gbp_prune_stats *stats, gbp_stream stream);
/* Both stages, synchronous, on the terrain's own stream: stage A, one
 * read-back of the flags, the FRAGILE edges re-decided with glibc
 * (gbp_resolve_fragile_host: GBP_F_RESOLVED, *n_resolved, may be NULL), stage
 * B.  Host remap[size of the tree before] (may be NULL) and stats[1]. */
int gbp_tree_revalidate_host(gbp_terrain *t, gbp_tree *tree, int direction, int adaptive,
                             int32_t *remap, gbp_prune_stats *stats, int64_t *n_resolved);
/* The same, with stage B's remap also left in the caller's device array
 * remap_dev[remap_cap] (its first n_before entries; GBP_E_SHAPE, nothing
 * changed, when the tree holds more than remap_cap vertices), for a caller
 * that carries indices of its own through the prune on the device
 * (gbp_plan_shared_remap_dev).  remap_dev == NULL: gbp_tree_revalidate_host. */
int gbp_tree_revalidate_keep_host(gbp_terrain *t, gbp_tree *tree, int direction, int adaptive,
                                  int32_t *remap, int32_t *remap_dev, int64_t remap_cap,
                                  gbp_prune_stats *stats, int64_t *n_resolved);

/* ---- a tree re-rooted at one of its vertices ----------------------------------
 * The robot executes its plan: at the next call it stands on a later state of
 * the path, a vertex k of the forward-grown start tree.  The dynamics are not
 * reversible, so what the next search may reuse of that tree is the subtree
 * below k.  Vertex i is kept when k lies on i's parent chain (i = k included)
 * and every edge (parent[j] -> j), j on the chain from i up to but excluding
 * k, has edge_valid[j] = 1; edge_valid[k] and everything above k are ignored.
 * k becomes vertex 0 (its action ten zeros, its parent -1, as gbp_tree_init
 * writes them) and the other kept vertices follow in ascending old index; in
 * a tree whose parents precede their children the result has them so again.
 * g is derived again from the new root down, g[c] = g[parent[c]] +
 * poseDistance(v[parent[c]], v[c]) with g[0] = 0, as gbp_tree_load_host
 * derives it (not g - g[k], which differs in the last bits). */
typedef struct {
  int64_t n_before;        /* vertices of the tree before the call                 */
  int64_t n_kept;          /* ... and after it                                     */
  int64_t n_outside;       /* dropped: not below new_root                          */
  int64_t n_edge_invalid;  /* dropped: below it, own edge failed                   */
  int64_t n_inherited;     /* dropped: below it, only because an ancestor was      */
  int64_t depth;           /* most edges between the new root and a kept vertex    */
} gbp_reroot_stats;
/* Device edge_valid[n] (NULL: every edge holds), remap[n] = a vertex's new
 * index or -1, stats[1].  The kept rows of v / a are moved, parent =
 * remap[parent], g derived, the fp16 search rows, the search bounds and the
 * successor lists rebuilt from the kept rows, the count set; the capacity
 * stays.  As in gbp_tree_prune_dev the rows go into fresh arrays that replace
 * the tree's (pointers from gbp_tree_device_ptrs are stale afterwards) and the
 * swap is the last step: a call that returns an error leaves the tree as it
 * was (remap and stats may have been written).  Synchronises the stream:
 * before, to compare n with the device's count (GBP_E_SHAPE when they differ);
 * in between, to read the levels' sizes that decide the launches of g; and
 * after.  GBP_E_INVALID_ARG when new_root is outside [0, n).  new_root = 0
 * with edge_valid = NULL is the identity. */
int gbp_tree_reroot_dev(gbp_tree *tree, int64_t n, int32_t new_root, const uint8_t *edge_valid,
                        int32_t *remap, gbp_reroot_stats *stats, gbp_stream stream);
/* Diagnostics (tools/tree_reroot_ab.py): of the process's last successful
 * gbp_tree_reroot_dev, the device time in milliseconds between stream events
 * of its three parts (the keep rule and depth; the compaction, the move and
 * the sort by depth; g by levels, the wait for the levels' sizes included) and
 * the kernels it launched. */
int gbp_tree_reroot_last(double ms[3], int64_t *launches);
/* Synchronous.  t == NULL: no edge is tested (direction and adaptive are
 * ignored).  Otherwise stage A of the prune (gbp_tree_revalidate_dev) on t, on
 * the terrain's own stream, the FRAGILE edges re-decided with glibc
 * (*n_resolved, may be NULL), then the re-root under those decisions: the
 * robot has moved and the map has changed, in one pass.  Host remap[size of
 * the tree before] (may be NULL) and stats[1].  GBP_E_INVALID_ARG when
 * new_root is outside the tree or the direction is bad; the tree is unchanged. */
int gbp_tree_reroot_host(gbp_terrain *t, gbp_tree *tree, int32_t new_root, int direction,
                         int adaptive, int32_t *remap, gbp_reroot_stats *stats, int64_t *n_resolved);
/* The same, with the remap also left in the caller's device array
 * remap_dev[remap_cap], as gbp_tree_revalidate_keep_host leaves the prune's. */
int gbp_tree_reroot_keep_host(gbp_terrain *t, gbp_tree *tree, int32_t new_root, int direction,
                              int adaptive, int32_t *remap, int32_t *remap_dev, int64_t remap_cap,
                              gbp_reroot_stats *stats, int64_t *n_resolved);

/* ---- a tree grafted onto a root that is not one of its vertices -------------------
 * The robot is part of the way through an action or has drifted off its plan
 * (or, on the reverse-grown goal tree, the goal has moved): the next search
 * starts from a state r that no vertex holds.  What it may reuse of a tree
 * grown in `direction` are the vertices r connects to directly and what hangs
 * below them.  (Ours: the reference has no such operation.)
 *   candidates  vertex j with poseDistance(r, v[j]) <= radius, compared as
 *               neighborhoodDist compares (radius = INFINITY: every vertex)
 *   attached    a candidate for which depth 0 of attemptConnect(s_existing = r,
 *               s = v[j], t_s = poseDistance(v[j], r) / V_NOM, direction)
 *               (rrt_connect.cpp:20-75) is REACHED: t_s > KINEMATICS_RES, the
 *               connect action valid, the pair check from r in `direction`
 *               valid — the check RRT*'s rewire makes.  v[j] is not compared
 *               with the check's s_new; a vertex whose state equals r has
 *               t_s = 0 and is not attached (that root is gbp_tree_reroot_*'s)
 *   parents     every attached vertex becomes a child of r, its action the
 *               connect action, also when one of its ancestors is attached
 *   kept        vertex i when its parent chain, i included, holds an attached
 *               vertex and every edge from i up to but excluding the nearest
 *               such vertex j has edge_valid = 1 (j's own old edge is ignored):
 *               the re-root's rule at vertex n of the tree of n + 1 vertices
 *               whose vertex n is r and whose attached vertices have parent n
 * r becomes vertex 0 (ten zero action values, parent -1, as gbp_tree_init
 * writes them), the kept vertices follow in ascending old index, g is derived
 * again from r down as gbp_tree_load_host derives it; a tree whose parents
 * precede their children has them so again.  With nothing attached the tree
 * is r alone: an answer, not an error.  r itself is never tested (callers test
 * roots with gbp_valid_states_*). */
typedef struct {
  int64_t n_before;        /* vertices of the tree before the call                   */
  int64_t n_kept;          /* ... and after it, the new root included                */
  int64_t n_candidates;    /* vertices within the radius        (0 from stage B:     */
  int64_t n_checked;       /* pair checks run                    the _host entries   */
                           /*                                    count stage A's)    */
  int64_t n_attached;      /* children of the new root                               */
  int64_t n_outside;       /* dropped: no attached vertex on the parent chain        */
  int64_t n_edge_invalid;  /* dropped: below one, not attached, own edge failed      */
  int64_t n_inherited;     /* dropped: below one, only because an ancestor was       */
  int64_t depth;           /* most edges between the new root and a kept vertex      */
} gbp_graft_stats;
#define GBP_F_GRAFT_CANDIDATE (1u << 16) /* stage A: the vertex lies within the radius     */
#define GBP_F_GRAFT_CHECKED   (1u << 17) /* stage A: its connect action had a pair check   */
/* Stage A: which vertices r attaches.  n = the tree's size (GBP_E_SHAPE when
 * it is not the device's count: the call reads it, which synchronises the
 * stream); host root[8]; device attach[n] (1 = attached), actions[n][10] (row
 * j written when vertex j's check ran: the connect action), flags[n] (the
 * check's GBP_F_* word, 0 without one, | GBP_F_GRAFT_CANDIDATE |
 * GBP_F_GRAFT_CHECKED).  One launch, one wave per vertex: the distance test
 * decides whether the wave goes on to the action and the pair check.  A
 * FRAGILE decision is left to the caller, as in gbp_tree_revalidate_dev.
 * GBP_E_INVALID_ARG for a bad direction, NaN in root, a negative or NaN radius. */
int gbp_tree_graft_check_dev(gbp_terrain *t, gbp_tree *tree, int64_t n, const double *root,
                             double radius, int direction, int adaptive, uint8_t *attach,
                             double *actions, uint32_t *flags, gbp_stream stream);
/* Stage B: the graft under the caller's decisions.  Host root[8]; device
 * attach[n] (non-zero = attached), actions[n][10] (read at attached vertices),
 * edge_valid[n] (NULL: every edge holds), remap[n] = a vertex's new index or
 * -1, stats[1] (n_candidates = n_checked = 0).  Attached vertices get parent 0
 * and their row of `actions`, every other kept vertex remap[parent] and its
 * old action; the fp16 search rows, the search bounds and the successor lists
 * are rebuilt from the kept rows (attached vertices leave their old parent's
 * list and form the root's, in ascending index; the other lists keep their
 * order); the count is set.  When n + 1 exceeds the capacity the fresh arrays
 * are larger (at least twice the capacity).  As in gbp_tree_reroot_dev
 * everything goes into fresh arrays and the swap is the last step: a call that
 * returns an error leaves the tree as it was.  Synchronises the stream as
 * gbp_tree_reroot_dev does.  GBP_E_SHAPE when n is not the device's count,
 * GBP_E_INVALID_ARG for NaN in root. */
int gbp_tree_graft_dev(gbp_tree *tree, int64_t n, const double *root, const uint8_t *attach,
                       const double *actions, const uint8_t *edge_valid, int32_t *remap,
                       gbp_graft_stats *stats, gbp_stream stream);
/* Diagnostics (tools/tree_graft_ab.py): gbp_tree_reroot_last's figures of the
 * process's last successful gbp_tree_graft_dev. */
int gbp_tree_graft_last(double ms[3], int64_t *launches);
/* Both stages, synchronous, on the terrain's own stream: stage A; with
 * test_edges also the edges' decisions on t (gbp_tree_revalidate_dev: the map
 * has changed and the robot is off the tree, in one pass); one read-back of
 * the flags; the FRAGILE checks re-decided with glibc (*n_resolved, may be
 * NULL); stage B.  Host remap[size of the tree before] (may be NULL) and
 * stats[1], n_candidates and n_checked counted from stage A's flags. */
int gbp_tree_graft_host(gbp_terrain *t, gbp_tree *tree, const double *root, double radius,
                        int direction, int adaptive, int test_edges, int32_t *remap,
                        gbp_graft_stats *stats, int64_t *n_resolved);
/* The same, with the remap also left in the caller's device array
 * remap_dev[remap_cap], as gbp_tree_reroot_keep_host leaves the re-root's. */
int gbp_tree_graft_keep_host(gbp_terrain *t, gbp_tree *tree, const double *root, double radius,
                             int direction, int adaptive, int test_edges, int32_t *remap,
                             int32_t *remap_dev, int64_t remap_cap, gbp_graft_stats *stats,
                             int64_t *n_resolved);

/* ---- a tree trimmed by cost ---------------------------------------
 * A search kept alive between plans only grows: nothing above removes a vertex
 * that is still valid.  The trim drops vertices by f[i] = g[i] +
 * poseDistance(v[i], r), r the other tree's root (its v[0], read on the
 * device), summed left to right without contraction:
 *   bound   vertex i >= 1 is over the bound when f[i] > bound.  A NaN f is not;
 *           a NaN or +inf bound cuts nothing.  With bound = the held best cost
 *           this is anytime RRT*'s branch-and-bound test: with the current g no
 *           path through such a vertex beats the held one.
 *   budget  when max_keep >= 1 and n > max_keep: cut = the element of rank
 *           max_keep - 1 (0-based, ascending, NaN above +inf) among f[1 .. n),
 *           and vertex i >= 1 is over the budget when !(f[i] < cut).  A group of
 *           equal f at the cut goes whole, so at most max_keep - 1 vertices
 *           besides the root pass; max_keep = 1 leaves the root alone.
 *           Otherwise cut = +inf and nothing is over the budget.
 *   protect vertex `protect` and every ancestor of it keep their flag whatever
 *           their f (-1: none).  The two rows of a connection differ in their
 *           last bits, so the best connection's own vertex can lie a few ulp
 *           above the best cost: a session protects best_a / best_b.  With
 *           protection the tree keeps at most max_keep vertices plus the
 *           protected chain's length.
 * g falls when a later rewire finds a shorter way, so a trimmed vertex might
 * have become useful: the usual anytime-RRT* trade, and opt-in. */
typedef struct {
  int64_t n_before;       /* vertices of the tree before the call                        */
  int64_t n_kept;         /* ... and after stage B (0 from stage A alone)                 */
  int64_t n_over_bound;   /* vertices with f > bound                                      */
  int64_t n_over_budget;  /* not over the bound, but over the budget                      */
  int64_t n_protected;    /* of those two groups: on the protected chain, flag kept       */
  int64_t n_inherited;    /* dropped by stage B though their own flag is 1 (an ancestor's
                             is 0; 0 from stage A alone)                                  */
  int64_t error;          /* stage A: 1 n is not the tree's count, 2 the protected chain
                             leaves [0, n) or does not reach the root; then keep[] is 0   */
  double cut;             /* the budget's cut (+inf: no budget applied)                   */
} gbp_trim_stats;
/* Stage A: the flags.  Device keep[n] in the form gbp_tree_prune_dev takes as
 * edge_valid (keep[0] = 1), optionally device f[n] (may be NULL), device
 * stats[1].  `other` is the other tree's handle (same device); its root does
 * not come to the host.  The cut is found by a radix select over the 64-bit
 * order-preserving image of f: integer counts only, so the result does not
 * depend on scheduling; no host synchronisation between its rounds.
 * Enqueue-only on `stream`, with the exception gbp_tree_revalidate_dev
 * documents: f and the select's counts live in the buffer the tree owns for the
 * prune's rows, grown (which synchronises the device) by a call that finds it
 * too small, so two stage-A calls on one tree must not be in flight at once.
 * GBP_E_SHAPE when n exceeds the tree's capacity, GBP_E_INVALID_ARG when
 * protect is outside [-1, n).  When n is not the device's count nothing of the
 * tree is read, keep[0] = 0 and stats->error = 1; a protected chain that leaves
 * the tree gives keep[0] = 0 and stats->error = 2. */
int gbp_tree_trim_flags_dev(gbp_tree *tree, gbp_tree *other, int64_t n, double bound, int64_t max_keep,
                            int32_t protect, uint8_t *keep, double *f, gbp_trim_stats *stats,
                            gbp_stream stream);
/* Both stages, synchronous, on `stream` (no terrain, no pair check and no
 * FRAGILE re-decision are involved): stage A, its record read back, then
 * gbp_tree_prune_dev under the flags.  Host remap[size of the tree before] (may
 * be NULL) and stats[1], n_kept and n_inherited from the prune's record.  A
 * failed call leaves the tree as it was: GBP_E_INVALID_ARG for a protect
 * outside the tree or a protected chain that does not reach the root. */
int gbp_tree_trim_host(gbp_tree *tree, gbp_tree *other, double bound, int64_t max_keep, int32_t protect,
                       int32_t *remap, gbp_trim_stats *stats, gbp_stream stream);
/* The same, with the remap also left in the caller's device array
 * remap_dev[remap_cap], as gbp_tree_revalidate_keep_host leaves the prune's. */
int gbp_tree_trim_keep_host(gbp_tree *tree, gbp_tree *other, double bound, int64_t max_keep,
                            int32_t protect, int32_t *remap, int32_t *remap_dev, int64_t remap_cap,
                            gbp_trim_stats *stats, gbp_stream stream);

/* ---- the device planner loop (RRTConnectClass::runRRTConnect,
 *      rrt_connect.cpp:230-314, batch-synchronous) ---------------------------
 * One half-iteration, enqueued on `stream` without any host synchronisation:
 *   stage 0  `batch` draws of T's randomState stream (planner_class.cpp:38-76),
 *            index target_index_base + i, and isValidState(STANCE) (:254)
 *   stage 1  the valid draws, compacted in order (wave ballot + prefix, look-back)
 *   stage 2  nearest vertex of T per target, newConfig's 6 candidates per target
 *            from the extend stream (gbp_extend_batch_dev's), their pair checks,
 *            the first valid one and the acceptance test (rrt.cpp:20-101)
 *   stage 3  non-TRAPPED successors appended to T in target order
 *   stage 4  each new vertex connected to its nearest vertex of O
 *            (attemptConnect, rrt_connect.cpp:20-120), direction opposite
 *   stage 5  non-TRAPPED connections appended to O in order; the first REACHED
 *            one is recorded (meet) and every later enqueued stage is a no-op
 * A FRAGILE decision halts the sequence after its stage (status.halt, every
 * later kernel a no-op): gbp_plan_resolve_host re-decides the flagged items
 * with glibc and returns the stage to resume the halted half-iteration at
 * (first_stage).  The trees must have room for `batch` more vertices each (an
 * append past a tree's capacity is not written and sets status.error bit 1). */
#define GBP_PLAN_HALT_TARGETS 1u
#define GBP_PLAN_HALT_EXTEND  2u
#define GBP_PLAN_HALT_CONNECT 4u
#define GBP_PLAN_HALT_STAR    8u  /* RRT*: an insertion's connect check (resume stage 7) */
#define GBP_PLAN_HALT_STAR_PAIRS 16u /* RRT*: a half's neighbour pairs (status.star_pairs) exceed
                                        max_pairs: gbp_plan_star_config with at least that many,
                                        then gbp_plan_resolve_host (resume stage 6) */
typedef struct {
  uint32_t halt;          /* GBP_PLAN_HALT_* of the stage that stopped the sequence */
  uint32_t done;          /* a connection REACHED */
  uint32_t error;         /* must be 0: bit 0 a bounded device spin ran out,
                             bit 1 an append found its tree full, bit 2 (RRT*)
                             the insertion's neighbour pairs or the REACHED
                             connections exceeded the workspace, bit 3 (RRT*)
                             a successor list that is not a tree */
  int32_t halt_half;      /* the half-iteration that halted */
  int32_t n_targets;      /* valid targets of the last executed half */
  int32_t n_validate;     /* candidates launched (6 n_targets, 0 when gated) */
  int32_t n_added;        /* successors appended to T */
  int32_t added_base;     /* T's count before them */
  int32_t n_conn_added;   /* connections appended to O */
  int32_t meet_half;      /* the half-iteration whose connection REACHED */
  uint64_t meet;          /* (connection index << 32) | O vertex of the first REACHED */
  int64_t ext_base;       /* extend stream base of the last half */
  int64_t ext_counter;    /* RRTClass extend counter after it */
  int64_t stat_targets, stat_attempts, stat_added, stat_conn_added;
  int64_t stat_fragile_resolved, stat_depth_capped;
  /* the gate: sequence number of the first planner kernel launch that raised
   * halt or done (~0: none).  Every launch carries its own number and is a
   * no-op only if the gate was raised by an EARLIER launch, so all workgroups
   * of the launch that raised it still finish their items. */
  uint64_t gate_seq;
  /* the matrix-core nearest-neighbour search's fp64 re-checks (k_nn_hreduce):
   * half-chunks of 16 rows re-checked, and segments scanned in full */
  int64_t stat_nn_rechecks, stat_nn_scans;
  /* the half whose targets were compacted last, and the counters before it:
   * a compaction re-run for the same half (resumed at stage 1 after a FRAGILE
   * halt) starts from them again */
  int32_t ext_half;
  uint32_t commit_fin;    /* reserved (unused since the look-ahead search) */
  int64_t ext_prev, stat_targets_prev;
  /* reserved (unused): gbp_plan_halves_dev's drawn-ahead targets are
   * counted in the workspace's look-ahead state (gbp_internal.h gbp_plan_la) */
  int32_t pre_targets, pre_fragile;
  /* RRT*-Connect (gbp_plan_star_config): the last half's neighbour pairs
   * (new vertex, vertex before it within delta) and their connect checks
   * launched; the REACHED connections so far (shared_a / shared_b of
   * rrt_star_connect.cpp:136-175) and the cheapest of them ranked after every
   * iteration (:181-193, ties to the earliest): best_a / best_b, best_cost
   * (INFINITY: none); the connect checks of the insertions (2 per pair) and
   * the rewires */
  int32_t star_pairs, star_rows, n_shared, best_a, best_b;
  int32_t star_vrows;     /* = star_rows (round 6: the rows are the connect checks
                             themselves, k_star_check; kept for the layout) */
  double best_cost;
  int64_t stat_star_connects, stat_rewires;
} gbp_plan_status;
int gbp_plan_ws_create(gbp_terrain *t, int64_t max_batch, gbp_plan_ws **out);
int gbp_plan_ws_destroy(gbp_plan_ws *ws);
/* zeroes the status (meet = ~0) and sets the extend counter */
int gbp_plan_reset(gbp_plan_ws *ws, int64_t extend_counter, gbp_stream stream);
int gbp_plan_half_dev(gbp_terrain *t, gbp_plan_ws *ws, gbp_tree *T, gbp_tree *O, int32_t half,
                      int direction, int64_t batch, uint64_t seed, uint64_t target_stream,
                      int64_t target_index_base, int adaptive, int first_stage,
                      gbp_stream stream);
int gbp_plan_status_read(gbp_plan_ws *ws, gbp_plan_status *out, gbp_stream stream);
/* half-iterations first_half .. first_half + n_halves - 1 (half h extends tree
 * h % 2: Ta FORWARD toward target stream stream_a, Tb REVERSE toward
 * stream_b, draws from index (h / 2) * batch), the first from first_stage:
 * gbp_plan_half_dev for each.  first_stage > 0 resumes a half that halted
 * (gbp_plan_resolve_host's *resume_stage); a fresh half starts at stage 0.
 * Half numbers identify a half's draws and must increase between
 * gbp_plan_reset calls. */
int gbp_plan_halves_dev(gbp_terrain *t, gbp_plan_ws *ws, gbp_tree *Ta, gbp_tree *Tb,
                        int32_t first_half, int32_t n_halves, int64_t batch, uint64_t seed,
                        uint64_t stream_a, uint64_t stream_b, int adaptive, int first_stage,
                        gbp_stream stream);
/* RRT*-Connect (rrt_star_connect.cpp:12-67, the batched form of
 * RRTStarConnectClass::buildRRTStarConnectBatched): with enable set, every
 * half-iteration of gbp_plan_half_dev / gbp_plan_halves_dev inserts its new
 * vertices as RRT*'s extend does, between stages 3 and 4:
 *   stage 6  the neighbourhood of each new vertex among the vertices before it
 *            (stateDistance <= delta, > 0: neighborhoodDist, planner_class.cpp:
 *            173-182, in the vertex map's iteration order), and the two depth-0 connect decisions
 *            per neighbour (choose-parent attemptConnect(s_near, s_new), rewire
 *            attemptConnect(s_new, s_near)), their pair checks batched
 *   stage 7  the insertions replayed in order: choose-parent, addEdge, rewire
 *            with the g of every rewired subtree updated (graph_class.cpp:131-138)
 * and stage 5 keeps every REACHED connection (no early stop) and, after tree
 * Tb's half, ranks the cheapest with the current g values (status best_*).
 * max_pairs sizes the neighbour pairs of one half: a half with more halts
 * with GBP_PLAN_HALT_STAR_PAIRS (status.star_pairs = the count; calling this
 * again with a larger max_pairs reallocates the sets and keeps the run's
 * list of kept connections, and gbp_plan_resolve_host resumes the half at
 * stage 6).  max_shared bounds the REACHED connections of a run (status.error
 * bit 2 when exceeded).  A FRAGILE insertion check halts with
 * GBP_PLAN_HALT_STAR (resume at stage 7).  enable = 0 returns the workspace
 * to RRT-Connect. */
int gbp_plan_star_config(gbp_plan_ws *ws, int enable, double delta, int64_t max_pairs,
                         int64_t max_shared);
/* ---- RRT*'s kept connections between searches -----------------
 * The REACHED connections of a run are pairs (a, b), a vertex of Ta and one of
 * Tb, listed in the order stage 5 appended them; status n_shared is the list's
 * length and best_a / best_b / best_cost the cheapest of them.  A kept
 * connection's two vertices need not hold the same state bit for bit (vertex
 * b of a connection into Tb is the pair check's returned s_new, not a copy of
 * a's row: DESIGN 5.10), so no entry compares the rows.  All three entries
 * need RRT* configured (gbp_plan_star_config), else GBP_E_UNSUPPORTED, and
 * order themselves behind the workspace's replay stream as well as `stream`;
 * the planner call that follows must use the same `stream`.  The first call
 * after gbp_plan_star_config set or raised max_shared allocates scratch of
 * the list's size (when it replaces a smaller one it synchronises the device).
 *
 * gbp_plan_shared_read_host: pairs[min(*n, max)][2] in list order, *n = the
 * list's length, the status's best; any output may be NULL.  Synchronous. */
int gbp_plan_shared_read_host(gbp_plan_ws *ws, int64_t max, int32_t *pairs, int64_t *n,
                              int32_t *best_a, int32_t *best_b, double *best_cost,
                              gbp_stream stream);
/* Replaces the list by the n host pairs[n][2], sets n_shared and the length
 * the ranking reads, resets the best to none (best_cost = INFINITY, best_a =
 * best_b = -1) and ranks the new list with the trees' current g
 * (rrt_star_connect.cpp:181-193: NaN skipped, strictly cheaper, ties to the
 * earliest).  The pairs are checked on the device in one pass before anything
 * changes: GBP_E_INVALID_ARG, list and best as they were, when an index is
 * outside [0, its tree's count) or n exceeds max_shared.  Synchronous. */
int gbp_plan_shared_load_host(gbp_plan_ws *ws, gbp_tree *Ta, gbp_tree *Tb, int64_t n,
                              const int32_t *pairs, gbp_stream stream);
typedef struct {
  int64_t n_before;     /* pairs listed before the call                          */
  int64_t n_kept;       /* ... and after it                                      */
  int64_t n_dropped_a;  /* dropped: its vertex of Ta is gone (whatever Tb's is)  */
  int64_t n_dropped_b;  /* dropped: only its vertex of Tb is gone                */
  int64_t error;        /* 1: a listed index outside [0, n_a) / [0, n_b): list,
                           length and best are unchanged (n_kept etc. undefined) */
} gbp_shared_stats;
/* The list through a prune or a re-root of the trees.  remap_a[n_a] /
 * remap_b[n_b] are the device arrays gbp_tree_prune_dev / gbp_tree_reroot_dev
 * wrote for Ta / Tb (NULL: that tree did not change, n_* = its size); Ta and
 * Tb are the trees after the change.  Pair (a, b) is kept when remap_a[a] >= 0
 * and remap_b[b] >= 0 and becomes (remap_a[a], remap_b[b]); kept pairs keep
 * their order.  Then, in the same sequence: n_shared and the ranking's length
 * set, the best reset to none, the survivors ranked with the trees' current g,
 * device stats[1] written (may be NULL).  Enqueue-only.  n_a / n_b out of step
 * with the remaps' lengths or the trees is the caller's error. */
int gbp_plan_shared_remap_dev(gbp_plan_ws *ws, gbp_tree *Ta, gbp_tree *Tb, const int32_t *remap_a,
                              int64_t n_a, const int32_t *remap_b, int64_t n_b,
                              gbp_shared_stats *stats, gbp_stream stream);

/* ---- the joined path of two device trees (rrt_connect.cpp:386-401) ----------
 * Ta's root -> vertex ia, then Tb's vertex ib -> root without ib itself, Tb's
 * edges carrying the child's action: device states[n_states][8],
 * actions[n_states - 1][10] (both 16-byte aligned), device info[1].  One
 * workgroup: one lane walks each parent chain into the tree's level-queue
 * scratch (so no other call on either tree may be in flight), bounded by the
 * tree's count; then all lanes gather the rows.  ia = ib = -1 with a workspace
 * (RRT* configured): the status's best_a / best_b, read on the device behind
 * the workspace's replay stream; with no best connection n_states = 0 and
 * length = INFINITY.  Yaw and duration are the host's, over the returned
 * path.  Nothing is written past max_states rows. */
#define GBP_PATH_E_CHAIN 1 /* ia / ib or a parent outside its tree, or no root within count steps */
#define GBP_PATH_E_SHORT 2 /* max_states < n_states (the length needed); no row written */
typedef struct {
  int32_t n_states;   /* states of the path (0: error GBP_PATH_E_CHAIN, or no best connection) */
  int32_t n_from_a;   /* of them Ta's (root .. ia)                                              */
  int32_t n_from_b;   /* ... and Tb's (ib's parent .. root)                                     */
  int32_t error;      /* 0 or GBP_PATH_E_*                                                      */
  double length;      /* g_a[ia] + g_b[ib]                                                      */
} gbp_path_info;
int gbp_tree_path_dev(gbp_tree *Ta, int32_t ia, gbp_tree *Tb, int32_t ib, gbp_plan_ws *ws,
                      int64_t max_states, double *states, double *actions, gbp_path_info *info,
                      gbp_stream stream);
/* the same with host outputs (states / actions hold max_states rows; the
 * first n_states / n_states - 1 are written); synchronous */
int gbp_tree_path_host(gbp_tree *Ta, int32_t ia, gbp_tree *Tb, int32_t ib, gbp_plan_ws *ws,
                       int64_t max_states, double *states, double *actions, gbp_path_info *info,
                       gbp_stream stream);

/* diagnostics: per half-iteration timing events (hipEvents with timing, on
 * the streams the stages run on) while enabled; gbp_plan_stage_times adds up
 * every timed half completed so far, in microseconds:
 *   us[0] the whole half (its first launch's start to stage 5's end),
 *   us[1] stages 0-3 (targets, the extends' search, their pair checks, select,
 *         append), us[2] stage 6 (RRT*: neighbourhoods, connect checks and
 *         their pair checks), us[3] stage 7 on the replay's stream (RRT*:
 *         replay, plus the best connection's ranking after Tb's halves),
 *   us[4] stages 4-5 (the connects' search, attemptConnect, append),
 *   with n >= 7 also us[5] stage 6 up to its pair checks (neighbourhoods,
 *   connect actions) and us[6] those pair checks,
 * and *halves the number of halves summed (n >= 5; reset clears).  A half's
 * events are read once the caller has synchronised its stream (status read). */
int gbp_plan_stage_timing(gbp_plan_ws *ws, int enable);
int gbp_plan_stage_times(gbp_plan_ws *ws, double *us, int n, int64_t *halves, int reset);
/* re-decides the halted stage's FRAGILE items on the host (T, O, direction,
 * batch of the halted half) and clears the halt; *resume_stage = the stage to
 * resume that half at (-1: nothing was halted) */
int gbp_plan_resolve_host(gbp_terrain *t, gbp_plan_ws *ws, gbp_tree *T, gbp_tree *O,
                          int direction, int64_t batch, int adaptive, int *resume_stage,
                          int64_t *n_resolved, gbp_stream stream);
/* RRTClass::extend (rrt.cpp:77-102) for n targets against a device tree
 * (nearest neighbour inside): targets[n][8] on the device
 * (n_dev, if not NULL, holds the count on the device, n its maximum);
 * result[i] = TRAPPED / ADVANCED / REACHED, new_vertex[i] = the appended vertex
 * or -1; candidate j of extend i is drawn from the extend stream at index
 * (extend_base + i) * 8 + j, as gbp_extend_batch_dev.  Uses ws's scratch (n <=
 * its max_batch).  T must have room for n more vertices (gbp_tree_reserve;
 * gbp_extend_tree_host reserves itself): appends past the capacity are
 * dropped and set status.error bit 1.  If a decision is FRAGILE the append halts (status.halt =
 * GBP_PLAN_HALT_EXTEND): gbp_plan_resolve_host(.., O = NULL, ..) then
 * gbp_extend_tree_finish_dev complete it.  gbp_extend_tree_host does all of
 * that synchronously from host targets. */
int gbp_extend_tree_dev(gbp_terrain *t, gbp_plan_ws *ws, gbp_tree *T, int64_t n,
                        const double *targets, const int32_t *n_dev, int direction, int adaptive,
                        uint64_t seed, int64_t extend_base, int32_t *result, int32_t *new_vertex,
                        gbp_stream stream);
int gbp_extend_tree_finish_dev(gbp_terrain *t, gbp_plan_ws *ws, gbp_tree *T, int64_t n,
                               int direction, int32_t *result, int32_t *new_vertex,
                               gbp_stream stream);
int gbp_extend_tree_host(gbp_terrain *t, gbp_plan_ws *ws, gbp_tree *T, int64_t n,
                         const double *targets, int direction, int adaptive, uint64_t seed,
                         int64_t extend_base, int32_t *result, int32_t *new_vertex,
                         int64_t *n_resolved);

/* ---- path shortcutting (RRTConnectClass::postProcessPath,
 *      rrt_connect.cpp:139-227) ------------------------------------------------
 * The walk keeps a state, then connects it to the farthest later state that
 * attemptConnect(s, s_next, FORWARD) REACHES.  That decision depends on the two
 * states and the terrain alone (the recursion's depth 0: t_s = poseDistance /
 * V_NOM > KINEMATICS_RES, isValidAction of the connect action, one valid pair
 * check), so the decisions of all pairs of all paths of a call are made in one
 * launch and the walk is replayed over the table.
 * n_paths paths: path p is the states [path_off[p], path_off[p + 1]) of
 * states[total][8], path_off[0] = 0, at least two states each (path_off is a
 * HOST array of n_paths + 1).  Pair (i, j), i < j, of path p with n states is
 * item pair_off[p] + i (2n - i - 1) / 2 + (j - i - 1), pair_off[p] = the pairs
 * of the paths before it (row-major upper triangle; n (n - 1) / 2 per path).
 *
 * gbp_shortcut_table_dev (rrt_connect.cpp:139-227, the walk's :166 decisions):
 * states on the device; reached[item] = 1 where the connect is REACHED, else 0;
 * flags[item] = the pair check's GBP_F_OOD / NAN / FRAGILE / LIMIT bits (0
 * where none ran).  Enqueue-only on `stream`; a FRAGILE item is left to the
 * caller to re-decide. */
int gbp_shortcut_table_dev(gbp_terrain *t, int64_t n_paths, const int64_t *path_off,
                           const double *states, int adaptive, uint8_t *reached, uint32_t *flags,
                           gbp_stream stream);
/* postProcessPath (rrt_connect.cpp:139-227) for n_paths paths, host pointers,
 * synchronous: one table launch, one read-back, the FRAGILE items re-decided
 * with glibc (*n_resolved, may be NULL), then each path's walk.
 * actions[total - n_paths][10]: path p's n_p - 1 edge actions (action k leads
 * into state k + 1), the paths' consecutive.  Outputs, packed the same way:
 * path p keeps the states [out_off[p], out_off[p + 1]) of out_states (capacity
 * total: the walk never lengthens a path) and one action fewer in out_actions
 * (capacity total - n_paths); out_off[n_paths + 1].  A kept connect action is
 * the one attemptConnect forms (:53-63); a state the walk cannot connect to
 * any later one keeps its successor and original action.  path_length[p],
 * path_yaw[p], path_cost[p] as the reference leaves path_length_ / path_yaw_ /
 * path_cost_ (the cost is the length, or with cost_add_yaw_flag the sum of
 * length * length_weight + yaw * yaw_weight per edge). */
int gbp_shortcut_paths_host(gbp_terrain *t, int64_t n_paths, const int64_t *path_off,
                            const double *states, const double *actions, int adaptive,
                            int cost_add_yaw_flag, double length_weight, double yaw_weight,
                            int64_t *out_off, double *out_states, double *out_actions,
                            double *path_length, double *path_yaw, double *path_cost,
                            int64_t *n_resolved);

#ifdef __cplusplus
}
#endif
#endif /* GBP_H */
