// terrainMapCallback on a robot-centred map that scrolls by whole cells, under a
// living ReplanSession (include/gbp_planner.h), for
// tests/test_gpu_terrain_move_session.py, which compares every record with the
// oracle's and tests/prune_ref.py's values:
//   1  loadDataFromGridMap(map 0), begin + search(H halves)
//   2  moveFromGridMap(map 1: the window displaced by whole cells, its
//      positions recomputed from the new origin), mapChanged
//   3  search(H2 halves)
//   4  end; moveFromGridMap on a window displaced by a third of a cell and on a
//      map of another size: both reload (false)
//
//   terrain_move_node <input.bin> <output.bin>
// input:  int32 nx ny; f64 res; two maps, each f64 origin_x origin_y and
//         z dx dy dz [nx ny] x-major f64 (float-representable); start[8] goal[8]
//         f64; int32 batch H H2; uint64 seed
// output: records (uint32 name length, name, char 'd' | 'i' | 'q', int64 count, data)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gbp_planner_compat.h"

using gbp_amd::BatchStats;
using gbp_amd::TreeDump;

// a minimal grid_map-shaped type (getSize, getStartIndex, getPosition, at,
// exists) over x-major arrays: grid_map index (i, j) is cell (nx-1-i, ny-1-j),
// whose position is the origin + the cell index * res
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
  std::vector<double> layer[4];  // elevation, dx, dy, dz
  Vec2i getSize() const { return Vec2i(nx, ny); }
  Vec2i getStartIndex() const { return Vec2i(0, 0); }
  Pos getPosition() const { return Pos(); }
  void getPosition(const Vec2i &idx, Pos &p) const {
    p.px = ox + (double)(nx - 1 - idx(0)) * res;
    p.py = oy + (double)(ny - 1 - idx(1)) * res;
  }
  float at(const char *name, const Vec2i &idx) const {
    const int k = !std::strcmp(name, "elevation") ? 0 : !std::strcmp(name, "dx") ? 1
                  : !std::strcmp(name, "dy") ? 2 : 3;
    return (float)layer[k][(size_t)(nx - 1 - idx(0)) * ny + (ny - 1 - idx(1))];
  }
  bool exists(const char *) const { return true; }
};
}  // namespace fake_grid_map

static FILE *out_ = nullptr;

template <class T>
static void put(const std::string &name, char type, const T *data, size_t count) {
  const uint32_t len = (uint32_t)name.size();
  const int64_t n = (int64_t)count;
  std::fwrite(&len, 4, 1, out_);
  std::fwrite(name.data(), 1, len, out_);
  std::fwrite(&type, 1, 1, out_);
  std::fwrite(&n, 8, 1, out_);
  if (count) std::fwrite(data, sizeof(T), count, out_);
}
static void put_i(const std::string &name, std::vector<int64_t> v) { put(name, 'q', v.data(), v.size()); }

static void put_trees(const std::string &tag, ReplanSession &s) {
  TreeDump d;
  s.dump(d);
  for (int k = 0; k < 2; k++) {
    const std::string t = tag + (k ? ".b." : ".a.");
    put(t + "v", 'd', d.v[k].empty() ? nullptr : d.v[k][0].data(), 8 * d.v[k].size());
    put(t + "act", 'd', d.a[k].empty() ? nullptr : d.a[k][0].data(), 10 * d.a[k].size());
    put(t + "parent", 'i', d.parent[k].data(), d.parent[k].size());
    put(t + "g", 'd', d.g[k].data(), d.g[k].size());
  }
}

template <class T>
static std::vector<T> get(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
    std::fprintf(stderr, "short input\n");
    std::exit(3);
  }
  return v;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  out_ = std::fopen(argv[2], "wb");
  if (!f || !out_) return 2;
  const auto dims = get<int32_t>(f, 2);
  const int nx = dims[0], ny = dims[1];
  const double res = get<double>(f, 1)[0];
  fake_grid_map::GridMap m[2];
  for (auto &g : m) {
    const auto o = get<double>(f, 2);
    g.nx = nx;
    g.ny = ny;
    g.res = res;
    g.ox = o[0];
    g.oy = o[1];
    for (auto &l : g.layer) l = get<double>(f, (size_t)nx * ny);
  }
  const auto sg = get<double>(f, 16);
  const auto cfg = get<int32_t>(f, 3);
  const uint64_t seed = get<uint64_t>(f, 1)[0];
  std::fclose(f);
  State start, goal;
  for (int k = 0; k < 8; k++) {
    start[k] = sg[k];
    goal[k] = sg[8 + k];
  }
  const int batch = cfg[0], H = cfg[1], H2 = cfg[2];
  try {
    FastTerrainMap terrain_;
    terrain_.loadDataFromGridMap(m[0]);
    gbp_terrain *h0 = terrain_.handle();
    ReplanSession s;
    s.begin(terrain_, start, goal, batch, 3.0, seed);
    BatchStats st1;
    s.search(1e9, H, &st1);
    put_trees("s1", s);
    put_i("s1.counters", {st1.halves, s.nextHalf(), s.extendCounter()});
    // 2: the window scrolls under the resident trees
    const bool moved = terrain_.moveFromGridMap(m[1]);
    put_i("move", {moved ? 1 : 0, terrain_.handle() == h0 ? 1 : 0});
    put("move.x", 'd', terrain_.getXData().data(), terrain_.getXData().size());
    put("move.y", 'd', terrain_.getYData().data(), terrain_.getYData().size());
    PruneStats ps[2];
    s.mapChanged(terrain_, ps);
    for (int k = 0; k < 2; k++)
      put_i(k ? "s2.prune.b" : "s2.prune.a",
            {ps[k].n_before, ps[k].n_kept, ps[k].n_edge_invalid, ps[k].n_inherited});
    put_trees("s2", s);
    // 3: the search goes on
    BatchStats st3;
    s.search(1e9, H2, &st3);
    put_trees("s3", s);
    put_i("s3.counters", {st3.halves, s.nextHalf(), s.extendCounter(), terrain_.handle() == h0 ? 1 : 0});
    s.end();
    // 4: a third of a cell, then another size: no height is reused
    fake_grid_map::GridMap frac = m[1];
    frac.ox += res / 3;
    const bool r1 = terrain_.moveFromGridMap(frac);
    const double x0 = terrain_.getXData()[0];
    fake_grid_map::GridMap wide = m[1];
    wide.nx = nx + 1;
    for (auto &l : wide.layer) l.assign((size_t)(nx + 1) * ny, 0.25);
    const bool r2 = terrain_.moveFromGridMap(wide);
    put_i("reload", {r1 ? 1 : 0, r2 ? 1 : 0, (int64_t)terrain_.getXData().size(),
                     x0 == frac.ox ? 1 : 0});
    // and from there on in place again
    fake_grid_map::GridMap next = wide;
    next.oy -= 2 * res;
    gbp_terrain *h2 = terrain_.handle();
    const bool r3 = terrain_.moveFromGridMap(next);
    const double xy[2] = {next.ox + 3.5 * res, next.oy + 1.5 * res};
    put_i("again", {r3 ? 1 : 0, terrain_.handle() == h2 ? 1 : 0,
                    terrain_.getGroundHeight(xy[0], xy[1]) == 0.25 ? 1 : 0});
  } catch (const std::exception &e) {
    std::fprintf(stderr, "terrain_move_node: %s\n", e.what());
    return 1;
  }
  std::fclose(out_);
  return 0;
}
