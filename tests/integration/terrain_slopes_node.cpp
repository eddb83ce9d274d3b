// terrainMapCallback on an elevation-only source (a grid_map without dx / dy /
// dz layers) with FastTerrainMap::setDeriveSlopes(true), for
// tests/test_gpu_slopes_node.py:
//   1  loadDataFromGridMap(map 0)
//   2  updateFromGridMap(map 1: the same geometry, other heights)   -> true
//   3  moveFromGridMap(map 2: the window displaced by (3, -2) cells) -> true
//   4  loadDataFromGridMap(map 3: another size): a new handle, the setting stays
// After each step readSlopes must equal, bit for bit, a whole-map deriveSlopes
// on a second FastTerrainMap loaded from the same arrays, and must not be the
// flat (0, 0, 1) a map without layers reads.  Prints one line per step; exit
// status 0 when every step matched.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gbp_planner.h"

// a minimal grid_map-shaped type (getSize, getStartIndex, getPosition, at,
// exists) with an elevation layer only: grid_map index (i, j) is cell
// (nx-1-i, ny-1-j), whose position is the origin + the cell index * res
namespace fake_grid_map {
struct Vec2i {
  int v[2];
  Vec2i(int a = 0, int b = 0) : v{a, b} {}
  int operator()(int i) const { return v[i]; }
};
struct Pos {
  double px = 0, py = 0;
  double x() const { return px; }
  double y() const { return py; }
};
struct GridMap {
  int nx = 0, ny = 0;
  double res = 0, ox = 0, oy = 0;
  std::vector<float> elevation;  // x-major
  Vec2i getSize() const { return Vec2i(nx, ny); }
  Vec2i getStartIndex() const { return Vec2i(0, 0); }
  Pos getPosition() const { return Pos(); }
  void getPosition(const Vec2i &idx, Pos &p) const {
    p.px = ox + (double)(nx - 1 - idx(0)) * res;
    p.py = oy + (double)(ny - 1 - idx(1)) * res;
  }
  float at(const char *, const Vec2i &idx) const {
    return elevation[(size_t)(nx - 1 - idx(0)) * ny + (ny - 1 - idx(1))];
  }
  bool exists(const char *name) const { return !std::strcmp(name, "elevation"); }
};
}  // namespace fake_grid_map

// the ground at world cell (cx, cy), time step t
static float ground(int cx, int cy, int t) {
  return (float)(0.05 * std::sin(0.37 * cx + 0.1 * t) + 0.04 * std::cos(0.23 * cy) +
                 0.002 * ((cx * 7 + cy * 13 + t * 5) % 11));
}

static fake_grid_map::GridMap window(int nx, int ny, int cx0, int cy0, int t) {
  fake_grid_map::GridMap m;
  m.nx = nx;
  m.ny = ny;
  m.res = 0.02;
  m.ox = cx0 * m.res;
  m.oy = cy0 * m.res;
  m.elevation.resize((size_t)nx * ny);
  for (int i = 0; i < nx; i++)
    for (int j = 0; j < ny; j++) m.elevation[(size_t)i * ny + j] = ground(cx0 + i, cy0 + j, t);
  return m;
}

static bool step(const char *name, gbp_amd::FastTerrainMap &terrain, const fake_grid_map::GridMap &m) {
  std::vector<double> x(m.nx), y(m.ny), z(m.elevation.begin(), m.elevation.end());
  for (int i = 0; i < m.nx; i++) x[i] = m.ox + (double)i * m.res;
  for (int j = 0; j < m.ny; j++) y[j] = m.oy + (double)j * m.res;
  gbp_amd::FastTerrainMap fresh(terrain.device());
  fresh.loadDataFlat(m.nx, m.ny, x.data(), y.data(), z.data(), nullptr, nullptr, nullptr);
  fresh.deriveSlopes(true);
  std::vector<double> got[3], want[3];
  terrain.readSlopes(got[0], got[1], got[2]);
  fresh.readSlopes(want[0], want[1], want[2]);
  bool same = true, flat = true;
  for (int k = 0; k < 3; k++) {
    same = same && got[k].size() == want[k].size() &&
           !std::memcmp(got[k].data(), want[k].data(), got[k].size() * sizeof(double));
    for (double v : got[k]) flat = flat && v == (k == 2 ? 1.0 : 0.0);
  }
  std::printf("%s: %s%s\n", name, same ? "same" : "DIFFERENT", flat ? " FLAT" : "");
  return same && !flat;
}

int main() {
  const int nx = 70, ny = 131;
  gbp_amd::FastTerrainMap terrain(0);
  terrain.setDeriveSlopes(true);  // once, before the first map
  bool ok = true;
  const fake_grid_map::GridMap m0 = window(nx, ny, 10, 10, 0);
  terrain.loadDataFromGridMap(m0);
  gbp_terrain *h = terrain.handle();
  ok = step("load", terrain, m0) && ok;
  const fake_grid_map::GridMap m1 = window(nx, ny, 10, 10, 1);
  ok = terrain.updateFromGridMap(m1) && terrain.handle() == h && ok;
  ok = step("update", terrain, m1) && ok;
  const fake_grid_map::GridMap m2 = window(nx, ny, 13, 8, 1);
  ok = terrain.moveFromGridMap(m2) && terrain.handle() == h && ok;
  ok = step("move", terrain, m2) && ok;
  const fake_grid_map::GridMap m3 = window(nx + 1, ny - 3, 0, 0, 2);
  ok = !terrain.updateFromGridMap(m3) && ok;  // another size: a reload
  ok = step("reload", terrain, m3) && ok;
  // the setting went to the new handle: an update in place stays derived
  const fake_grid_map::GridMap m4 = window(nx + 1, ny - 3, 0, 0, 3);
  ok = terrain.updateFromGridMap(m4) && ok;
  ok = step("update after reload", terrain, m4) && ok;
  return ok ? 0 : 1;
}
