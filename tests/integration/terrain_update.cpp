// terrainMapCallback on a living FastTerrainMap (global_body_planner.cpp:37-44):
// updateFromGridMap keeps the engine handle when the new map has the loaded
// map's geometry and reloads otherwise; either way getGroundHeight equals a
// freshly loaded map's, bit for bit.  updateDataFlat / updateData patch a
// rectangle and the whole map.  Built and run by tests/test_gpu_terrain_update.py
// (exit 0 = all equal).
#include <cstdio>
#include <cstring>
#include <vector>

#include "gbp_planner_compat.h"

// a minimal grid_map-shaped type (getSize, getStartIndex, getPosition, at, exists)
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
  int nx, ny;
  double res;
  std::vector<float> z;  // grid_map index (i, j) -> z[i*ny + j]
  Vec2i getSize() const { return Vec2i(nx, ny); }
  Vec2i getStartIndex() const { return Vec2i(0, 0); }
  Pos getPosition() const { return Pos(); }
  void getPosition(const Vec2i &idx, Pos &p) const {
    p.px = (nx - 1 - idx(0)) * res;
    p.py = (ny - 1 - idx(1)) * res;
  }
  float at(const char *layer, const Vec2i &idx) const {
    (void)layer;
    return z[(size_t)idx(0) * ny + idx(1)];
  }
  bool exists(const char *layer) const {
    (void)layer;
    return false;
  }
};
}  // namespace fake_grid_map

static fake_grid_map::GridMap make_map(int nx, int ny, double res, unsigned seed) {
  fake_grid_map::GridMap m{nx, ny, res, {}};
  m.z.resize((size_t)nx * ny);
  unsigned s = seed;
  for (float &v : m.z) {
    s = s * 1664525u + 1013904223u;
    v = (float)((s >> 8) & 0xFFFF) / 65536.0f * 0.4f;
  }
  return m;
}

// the heights of both maps at points inside every cell, compared bit for bit
static int compare(FastTerrainMap &a, FastTerrainMap &b, int nx, int ny, double res) {
  std::vector<double> xy;
  for (int i = 0; i + 1 < nx; i++)
    for (int j = 0; j + 1 < ny; j++) {
      xy.push_back((i + 0.3) * res);
      xy.push_back((j + 0.6) * res);
    }
  const int64_t n = (int64_t)xy.size() / 2;
  std::vector<double> ha(n), hb(n);
  std::vector<uint8_t> na(n), nb(n);
  a.getGroundHeightBatch(n, xy.data(), ha.data(), na.data());
  b.getGroundHeightBatch(n, xy.data(), hb.data(), nb.data());
  int bad = 0;
  for (int64_t k = 0; k < n; k++)
    bad += std::memcmp(&ha[k], &hb[k], sizeof(double)) != 0 || na[k] != nb[k];
  return bad;
}

int main() {
  const int nx = 45, ny = 31;
  const double res = 0.05;
  const fake_grid_map::GridMap m0 = make_map(nx, ny, res, 1), m1 = make_map(nx, ny, res, 2);
  FastTerrainMap terrain_;
  terrain_.loadDataFromGridMap(m0);
  gbp_terrain *h0 = terrain_.handle();

  // same geometry: updated in place, the handle stays
  if (!terrain_.updateFromGridMap(m1)) return 2;
  if (terrain_.handle() != h0) return 3;
  {
    FastTerrainMap fresh;
    fresh.loadDataFromGridMap(m1);
    if (compare(terrain_, fresh, nx, ny, res)) return 4;
    FastTerrainMap old;
    old.loadDataFromGridMap(m0);
    if (!compare(terrain_, old, nx, ny, res)) return 5;  // the update did something
  }

  // a rectangle through updateDataFlat, then the whole map through updateData
  {
    std::vector<double> z((size_t)nx * ny);
    for (int i = 0; i < nx; i++)
      for (int j = 0; j < ny; j++)
        z[(size_t)i * ny + j] = (double)m1.z[(size_t)(nx - 1 - i) * ny + (ny - 1 - j)];
    const int ix0 = 7, iy0 = 5, pnx = 33, pny = 9;
    std::vector<double> patch((size_t)pnx * pny);
    for (int i = 0; i < pnx; i++)
      for (int j = 0; j < pny; j++) {
        patch[(size_t)i * pny + j] = 0.25 + 0.125 * ((i + j) % 3);
        z[(size_t)(ix0 + i) * ny + iy0 + j] = patch[(size_t)i * pny + j];
      }
    terrain_.updateDataFlat(ix0, iy0, pnx, pny, patch.data(), nullptr, nullptr, nullptr);
    if (terrain_.handle() != h0) return 6;
    FastTerrainMap fresh;
    fresh.loadDataFlat(nx, ny, terrain_.getXData().data(), terrain_.getYData().data(), z.data(),
                       nullptr, nullptr, nullptr);
    if (compare(terrain_, fresh, nx, ny, res)) return 7;

    std::vector<std::vector<double>> zz(nx, std::vector<double>(ny)), none;
    for (int i = 0; i < nx; i++)
      for (int j = 0; j < ny; j++) zz[i][j] = z[(size_t)i * ny + j] = 0.5 * ((i * 7 + j * 3) % 5);
    terrain_.updateData(zz, none, none, none);
    if (terrain_.handle() != h0) return 8;
    FastTerrainMap fresh2;
    fresh2.loadDataFlat(nx, ny, terrain_.getXData().data(), terrain_.getYData().data(), z.data(),
                        nullptr, nullptr, nullptr);
    if (compare(terrain_, fresh2, nx, ny, res)) return 9;
  }

  // changed geometry (another resolution, another size): reloaded
  const fake_grid_map::GridMap m2 = make_map(nx, ny, 0.1, 3), m3 = make_map(nx + 1, ny, res, 4);
  if (terrain_.updateFromGridMap(m2)) return 10;
  {
    FastTerrainMap fresh;
    fresh.loadDataFromGridMap(m2);
    if (compare(terrain_, fresh, nx, ny, 0.1)) return 11;
  }
  if (terrain_.updateFromGridMap(m3)) return 12;
  {
    FastTerrainMap fresh;
    fresh.loadDataFromGridMap(m3);
    if (compare(terrain_, fresh, nx + 1, ny, res)) return 13;
  }
  // and from there on in place again
  const fake_grid_map::GridMap m4 = make_map(nx + 1, ny, res, 5);
  gbp_terrain *h3 = terrain_.handle();
  if (!terrain_.updateFromGridMap(m4) || terrain_.handle() != h3) return 14;
  {
    FastTerrainMap fresh;
    fresh.loadDataFromGridMap(m4);
    if (compare(terrain_, fresh, nx + 1, ny, res)) return 15;
  }
  std::printf("terrain_update ok\n");
  return 0;
}
