// gbp_terrain_patch.h — the engine-free part of an in-place terrain update
// (gbp_terrain_update_*, gbp_terrain_read_host; internal to libgbp): the
// rectangle and its pair rows, where a cell lies in either source layout, the
// float round-trip check of a patch and the scatter into the handle's host
// mirror; and of a window moved by whole cells (gbp_terrain_move_host): its
// overlap and strips, the mirror's shift, nan_free after it and the detection
// of a whole-cell shift between two coordinate vectors.  No HIP here:
// csrc/gbp_terrain.hip runs the same index rules on the device, and
// tests/native/terrain_patch_probe.cpp and terrain_move_probe.cpp run these
// under sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>

#include "gbp.h"

namespace gbp_patch {

// cells [ix0, ix0 + nx) x [iy0, iy0 + ny) of an NX x NY map
struct Rect {
  int32_t ix0 = 0, iy0 = 0, nx = 0, ny = 0;
};

// r == nullptr: the whole map.  GBP_E_SHAPE when the rectangle is empty or
// leaves the map.
int resolve_rect(int NX, int NY, const gbp_rect *r, Rect *out);

// The x-pair rows [*p0, *p1) that hold a cell of the rectangle: pair p keeps
// z[p][iy] in slot 0 and z[p + 1][iy] in slot 1 (p < NX - 1), so the rows are
// [max(ix0 - 1, 0), min(ix0 + nx, NX - 1)).
void pair_rows(int NX, const Rect &r, int *p0, int *p1);

// the smallest rectangle holding both
Rect rect_union(const Rect &a, const Rect &b);

// GBP_E_INVALID_ARG for an unknown layout or a null source, GBP_E_SHAPE for a
// leading dimension below the layout's minimum (GBP_SRC_F64_XMAJOR: r.ny,
// GBP_SRC_F32_GRIDMAP: NX)
int check_source(int layout, int NX, const Rect &r, int64_t ld, const void *src);

// element index of cell (ix, iy) of the map in a source of `layout`:
//   GBP_SRC_F64_XMAJOR   (ix - ix0) * ld + (iy - iy0)
//   GBP_SRC_F32_GRIDMAP  (NX - 1 - ix) + (NY - 1 - iy) * ld   (fast_terrain_map.cpp:57-61)
inline int64_t src_index(int layout, int NX, int NY, const Rect &r, int64_t ld, int ix, int iy) {
  return layout == GBP_SRC_F32_GRIDMAP
             ? (int64_t)(NX - 1 - ix) + (int64_t)(NY - 1 - iy) * ld
             : (int64_t)(ix - r.ix0) * ld + (int64_t)(iy - r.iy0);
}

// the source's value for cell (ix, iy), widened to double
inline double src_value(int layout, int NX, int NY, const Rect &r, int64_t ld, const void *src,
                        int ix, int iy) {
  const int64_t k = src_index(layout, NX, NY, r, ld, ix, iy);
  return layout == GBP_SRC_F32_GRIDMAP ? (double)((const float *)src)[k] : ((const double *)src)[k];
}

// every value of the rectangle is NaN or float-representable (a float source
// always is)
bool round_trips(int layout, int NX, int NY, const Rect &r, int64_t ld, const void *src);

// Everything an update checks before it writes, in the order of the entry
// points: rectangle (GBP_E_SHAPE), layout and ld (check_source), then, for an
// fp32-storage handle, the round trip (GBP_E_UNSUPPORTED).  Writes *out only.
int check_patch(int NX, int NY, int storage, const gbp_rect *r, int layout, int64_t ld,
                const void *src, Rect *out);

// mirror[ix * NY + iy] = the source's value over the rectangle, rounded to
// float when the handle stores fp32 (what the device then holds)
void scatter(double *mirror, int NX, int NY, const Rect &r, int layout, int64_t ld,
             const void *src, bool f32);

// none of z[0, n) is NaN (infinities are heights like any other)
bool nan_free(const double *z, size_t n);

// The same fact about the mirror once a scatter has written rectangle r, given
// what held before it (`was`): a rectangle of non-NaN values written into a
// NaN-free map keeps it, and reading the rectangle decides; otherwise the
// whole mirror is scanned (a NaN written clears it; the values written may
// have replaced the last NaN).
bool nan_free_after(const double *mirror, int NX, int NY, const Rect &r, bool was);

// ---- a window moved by whole cells (gbp_terrain_move_host) --------------------
// New cell (ix, iy) holds what old cell (ix + sx, iy + sy) held where that cell
// lies in the old map: the overlap, in new indices.  The other new cells are
// the strips, an L of at most two rectangles: |sx| full rows, then |sy|
// columns of the rows that are left.  Overlap and strips partition the map.
// |sx| >= NX or |sy| >= NY: no overlap (overlap.nx = overlap.ny = 0) and one
// strip, the whole map; sx = sy = 0: no strip.
struct MoveRects {
  Rect overlap;
  int nstrips = 0;
  Rect strip[2];
};
MoveRects move_rects(int NX, int NY, int64_t sx, int64_t sy);

// a strip's cells in a source that holds the whole new map: the pointer a
// Rect-relative GBP_SRC_F64_XMAJOR index (src_index) starts from; a
// GBP_SRC_F32_GRIDMAP layer is indexed by the map's own cell, so it is src
inline const void *move_src(int layout, int64_t ld, const void *src, const Rect &r) {
  return layout == GBP_SRC_F32_GRIDMAP || !src
             ? src
             : (const void *)((const double *)src + (int64_t)r.ix0 * ld + r.iy0);
}

// the mirror's overlap shifted in place: mirror[ix][iy] = old mirror[ix + sx]
// [iy + sy] over m.overlap, rows in the order in which no row is read after it
// was written, each row by memmove; the strips' cells keep stale values
void shift_mirror(double *mirror, int NX, int NY, int64_t sx, int64_t sy, const MoveRects &m);

// nan_free once the strips have been scattered behind shift_mirror: kept when
// it held before and no strip cell is NaN (the overlap's cells all come from
// the old map), otherwise one full scan
bool nan_free_after_move(const double *mirror, int NX, int NY, const MoveRects &m, bool was);

// Is the coordinate vector n[0, N) the vector o[0, N) displaced by a whole
// number of cells?  h = (o[N-1] - o[0]) / (N - 1), *shift = round((n[0] - o[0])
// / h); accepted when every new position with an old counterpart, n[i] against
// o[i + shift], lies within h * rel_tol of it (with |shift| >= N there is no
// counterpart and no height is reused: accepted).  false for N < 2, h not
// positive and finite, a NaN position, or a shift that does not fit an int.
bool detect_shift(const double *o, const double *n, int N, double rel_tol, int *shift);

}  // namespace gbp_patch
