/*
 * STAND-IN for <grid_map_core/grid_map_core.hpp>, test infrastructure only.
 * This is NOT grid_map: it declares the members of its public interface that
 * FastTerrainMap::loadDataFromGridMap names (GridMap::getSize / getPosition /
 * exists / at, Index, Position) so that the reference's sources compile where
 * grid_map is not installed.  The parity driver never calls
 * loadDataFromGridMap: grid_map's own CSV -> geometry path stays unpinned.
 */
#ifndef GBP_STANDIN_GRID_MAP_CORE
#define GBP_STANDIN_GRID_MAP_CORE

#include <array>
#include <map>
#include <string>
#include <vector>

namespace grid_map {

struct Index {
  int i[2];
  Index() : i{0, 0} {}
  Index(int a, int b) : i{a, b} {}
  int operator()(int k) const { return i[k]; }
};
typedef Index Size;

struct Position {
  double p[2];
  Position() : p{0.0, 0.0} {}
  double x() const { return p[0]; }
  double y() const { return p[1]; }
};

class GridMap {
 public:
  Size size;
  double resolution = 1.0;
  Position centre;
  std::map<std::string, std::vector<float>> layers; /* row-major [size(0)][size(1)] */

  const Size &getSize() const { return size; }
  bool exists(const std::string &layer) const { return layers.count(layer) != 0; }
  float &at(const std::string &layer, const Index &idx) {
    return layers[layer][idx(0) * size(1) + idx(1)];
  }
  /* cell centres, index 0 at the largest coordinate (grid_map's convention) */
  bool getPosition(const Index &idx, Position &pos) const {
    for (int k = 0; k < 2; k++)
      pos.p[k] = centre.p[k] + (0.5 * size(k) - 0.5 - idx(k)) * resolution;
    return idx(0) >= 0 && idx(0) < size(0) && idx(1) >= 0 && idx(1) < size(1);
  }
};

}  // namespace grid_map

#endif
