// gbp_planner.h — C++ host mirror of the reference planner API over the C ABI.
//
// Same class / function names, argument meanings and return conventions as
// the reference (include/global_body_planner/{fast_terrain_map,planning_utils,
// planner_class,rrt,rrt_connect}.h), with every state-validity evaluation,
// terrain query, nearest-neighbour scan and candidate sampling executed by the
// HIP engine (include/gbp.h).  Namespace gbp_amd; include gbp_planner_compat.h
// for the reference's global names (the drop-in under the ROS node, see
// INTEGRATION.md).  No ROS / grid_map / Eigen dependency.
//
// Extensions beyond the reference surface (all batch-synchronous, B = 1
// reproduces the sequential algorithm on the engine's counter-based RNG):
//   planning_utils::isValidStateActionPairBatch, FastTerrainMap::*Batch,
//   PlannerClass::getNearestNeighborBatch, RRTConnectClass::buildRRTConnectBatched.
#pragma once

#include <array>
#include <chrono>
#include <stdexcept>
#include <type_traits>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "gbp.h"

namespace gbp_amd {

namespace planning_utils {
// include/global_body_planner/planning_utils.h:21-66 (constexpr: csrc/host/
// gbp_planning_math.cpp asserts each equal to the engine's own statement)
constexpr double H_MAX = 0.4;
constexpr double H_MIN = 0.075;
constexpr double V_MAX = 2.0;
constexpr double V_NOM = 0.75;
constexpr double P_MAX = 1.0;
constexpr double DP_MAX = 3.0;
constexpr double ANG_ACC_MAX = 7.0;
constexpr double ROBOT_L = 0.3;
constexpr double ROBOT_W = 0.3;
constexpr double ROBOT_H = 0.05;
constexpr double M_CONST = 13;
constexpr double G_CONST = 9.81;
constexpr double F_MAX = 637;
constexpr double MU = 1.0;
constexpr double T_S_MIN = 0.3;
constexpr double T_S_MAX = 0.3;
constexpr double T_F_MIN = 0.0;
constexpr double T_F_MAX = 0.5;
constexpr double KINEMATICS_RES = 0.05;
constexpr double BACKUP_TIME = 0.2;
constexpr double BACKUP_RATIO = 0.5;
constexpr int NUM_GEN_STATES = 6;
constexpr double GOAL_BOUNDS = 0.5;
constexpr int FLIGHT = 0;
constexpr int STANCE = 1;
constexpr int CONNECT_STANCE = 2;
constexpr int FORWARD = 0;
constexpr int REVERSE = 1;
constexpr int POSEDIM = 3;
constexpr int STATEDIM = 8;
constexpr int ACTIONDIM = 10;
typedef std::array<double, STATEDIM> State;
typedef std::array<double, ACTIONDIM> Action;
typedef std::pair<State, Action> StateActionPair;
constexpr double INFTY = 1.7976931348623157e308;
constexpr double MY_PI = 3.14159;
}  // namespace planning_utils

using planning_utils::Action;
using planning_utils::State;

#define GBP_PLANNER_TRAPPED 0
#define GBP_PLANNER_ADVANCED 1
#define GBP_PLANNER_REACHED 2

// Thrown only by constructors / loaders when the engine reports an error
// (the reference's hot path has no error channel; the C ABI returns codes).
struct EngineError : std::runtime_error {
  int status;
  EngineError(int s, const std::string &what);
};

// ---- terrain ingest without ROS ---------------------------------------------
// TerrainMapPublisher::loadCSV (terrain_map_publisher.cpp:290-327): comma
// separated doubles per line, '#' lines skipped, unparsable fields reported
// on stdout and skipped (stod("nan") parses)
std::vector<std::vector<double>> loadCSV(const std::string &filename);

// The arrays FastTerrainMap holds after the reference's CSV -> grid_map ->
// FastTerrainMap path: TerrainMapPublisher::loadMapFromCSV (:330-370) sets a
// grid_map geometry with a FLOAT resolution (:343-346) and float layers
// (x-major transpose at :363-368); FastTerrainMap::loadDataFromGridMap
// (fast_terrain_map.cpp:31-91) reads the cell-centre positions back in
// reversed index order and casts the layers float -> double.  grid_map_core's
// setGeometry / getPosition arithmetic (GridMap.cpp, GridMapMath.cpp; not in
// this image) is restated: size = round(length / res), length = size * res,
// position(index) = (map_position + (0.5 length - 0.5 res)) + res * (-index).
struct TerrainArrays {
  int x_size = 0, y_size = 0;
  std::vector<double> x, y;           // ascending (x_data_, y_data_)
  std::vector<double> z, dx, dy, dz;  // x-major [x_size][y_size]
};
// dir holds xdata.csv, ydata.csv, zdata.csv, dxdata.csv, dydata.csv, dzdata.csv
// (data/<terrain_type>/ in the reference); throws std::runtime_error on a
// missing file or non-square cells (:347-348)
TerrainArrays terrainArraysFromCSV(const std::string &dir);

// ---- FastTerrainMap (fast_terrain_map.h:14-120) ------------------------------
class FastTerrainMap {
 public:
  explicit FastTerrainMap(int device = 0);
  // wrap an existing engine handle (not owned: the caller destroys it)
  static FastTerrainMap borrow(gbp_terrain *handle);
  FastTerrainMap(FastTerrainMap &&o) noexcept;
  ~FastTerrainMap();
  FastTerrainMap(const FastTerrainMap &) = delete;
  FastTerrainMap &operator=(const FastTerrainMap &) = delete;

  // fast_terrain_map.cpp:10-28 (x-major nested vectors, as the reference)
  void loadData(int x_size, int y_size, std::vector<double> x_data, std::vector<double> y_data,
                std::vector<std::vector<double>> z_data, std::vector<std::vector<double>> dx_data,
                std::vector<std::vector<double>> dy_data, std::vector<std::vector<double>> dz_data);
  // flat x-major variant (no nested-vector copies); dx/dy/dz may be null
  void loadDataFlat(int x_size, int y_size, const double *x, const double *y, const double *z,
                    const double *dx, const double *dy, const double *dz);
  // fast_terrain_map.cpp:31-91 for any map type exposing the grid_map calls
  // used there (getSize, getPosition, at, exists); see INTEGRATION.md
  template <class GridMap>
  void loadDataFromGridMap(const GridMap &map);
  // the node's map_data_source "csv" path without ROS (terrainArraysFromCSV)
  void loadMapFromCSV(const std::string &dir);

  // New heights for the loaded map, in place (gbp_terrain_update_host): the
  // engine handle, its options, sampling configuration and workspaces and the
  // planner workspaces created for it stay; the geometry and the storage type
  // do not change (heights an fp32 handle cannot hold throw).  Cells [ix0, ix0 +
  // pnx) x [iy0, iy0 + pny), flat x-major z[i * pny + j]; dx/dy/dz all three or
  // null (null: the handle's slope layers stay as they are).
  void updateDataFlat(int ix0, int iy0, int pnx, int pny, const double *z, const double *dx,
                      const double *dy, const double *dz);
  // the whole map from x-major nested vectors (slope layers when all three
  // have x_size rows, as loadData)
  void updateData(const std::vector<std::vector<double>> &z_data,
                  const std::vector<std::vector<double>> &dx_data,
                  const std::vector<std::vector<double>> &dy_data,
                  const std::vector<std::vector<double>> &dz_data);
  // terrainMapCallback (global_body_planner.cpp:37-44) on a map that keeps its
  // geometry: when the map's size, every x / y position and the presence of
  // slope layers equal the loaded map's bit for bit, the heights are updated
  // in place and true is returned; otherwise loadDataFromGridMap(map), false.
  template <class GridMap>
  bool updateFromGridMap(const GridMap &map);

  // The loaded map's window moved by (sx, sy) whole cells, in place
  // (gbp_terrain_move_host): new cell (i, j) keeps what old cell (i + sx, j +
  // sy) held where the old map has that cell, every other cell is read from
  // z (and dx / dy / dz: all three or null), the WHOLE new map, flat x-major
  // z[i * y_size + j]; x[x_size], y[y_size] are the new coordinates.  The
  // handle, its options, sampling and workspaces and the planner workspaces
  // created for it stay, and so may a ReplanSession: mapChanged after the move
  // prunes what the new window no longer holds.  Null slope layers for a map
  // loaded with them: the kept cells' slopes move along, the new cells read
  // (0, 0, 1).
  void moveDataFlat(int64_t sx, int64_t sy, const double *x, const double *y, const double *z,
                    const double *dx, const double *dy, const double *dz);
  // terrainMapCallback on a robot-centred map that scrolls by whole cells
  // (grid_map's move; start index 0 as loadDataFromGridMap).  The map's size
  // and the presence of slope layers must equal the loaded map's, and with
  // sx = round((x_new[0] - x_old[0]) / h), h = (x_old[nx-1] - x_old[0]) / (nx -
  // 1) (sy likewise) every new position that has an old counterpart must lie
  // within h / 1024 of it (gbp_coord_shift): then moveDataFlat(sx, sy, ...)
  // and true.  Otherwise (another size, a changed spacing, a displacement by a
  // fraction of a cell) loadDataFromGridMap(map) and false.
  template <class GridMap>
  bool moveFromGridMap(const GridMap &map);

  // Slope layers derived on the device from the heights the handle holds
  // (gbp_terrain_derive_slopes_host, the rule of gbp.h: central differences,
  // (-gx, -gy, 1) / |.|, one-sided beside the map's edge and beside NaN),
  // for sources that carry an elevation layer and no dx / dy / dz.
  // deriveSlopes derives the whole map now; round_f32 rounds each component
  // through float, what a grid_map layer would hold.
  void deriveSlopes(bool round_f32 = true);
  // Off by default.  While on, loadData*, loadDataFromGridMap, updateData*,
  // updateFromGridMap, moveDataFlat and moveFromGridMap take the source's
  // layers when it has them, as always, and derive the layers when it has none,
  // instead of leaving (0, 0, 1) or stale values (GBP_OPT_DERIVE_SLOPES on the
  // handle: an update re-derives its rectangle and the nodes next to it, a
  // move the whole map).  Turning it on for a loaded map without layers
  // derives them now.  The setting survives a reload into a new handle.  On a
  // map made by borrow() it throws EngineError(GBP_E_UNSUPPORTED): the handle's
  // layers and options are its owner's (gbp_terrain_set_option there).
  void setDeriveSlopes(bool on, bool round_f32 = true);
  // the layers the device holds, flat x-major [x_size * y_size] each
  void readSlopes(std::vector<double> &dx, std::vector<double> &dy, std::vector<double> &dz);

  double getGroundHeight(const double x, const double y);               // :94-132
  bool heightIsNan(const double x, const double y);                     // :135-157
  std::array<double, 3> getSurfaceNormal(const double x, const double y);  // :160-213
  const std::vector<double> &getXData() const { return x_data_; }       // :216-218
  const std::vector<double> &getYData() const { return y_data_; }       // :221-223

  // batched queries: xy[n][2]
  void getGroundHeightBatch(int64_t n, const double *xy, double *h, uint8_t *is_nan);
  void getSurfaceNormalBatch(int64_t n, const double *xy, double *normal);

  gbp_terrain *handle() const { return handle_; }
  int device() const { return device_; }

 private:
  int device_;
  gbp_terrain *handle_ = nullptr;
  bool owned_ = true;
  bool slopes_ = false;  // the handle was loaded with slope layers
  bool layers_ = false;  // it holds slope layers: loaded, or derived since
  bool derive_ = false, derive_f32_ = true;  // setDeriveSlopes
  int x_size_ = 0, y_size_ = 0;
  std::vector<double> x_data_, y_data_;
};

namespace planning_utils {
// planning_utils.cpp:97-132, planning_utils.h:133-155
State interp(State q1, State q2, double x);
double poseDistance(const State &q1, const State &q2);
double stateDistance(const State &q1, const State &q2);
double stateYawDistance(const State &q1, const State &q2);
double stateDistance(const State &q1, const State &q2, bool cost_add_yaw_flag,
                     double cost_add_yaw_length_weight, double cost_add_yaw_yaw_weight);
bool isWithinBounds(State s1, State s2);
// planning_utils.cpp:237-370 (host arithmetic, identical expressions)
State applyStance(State s, Action a, double t);
State applyStance(State s, Action a);
State applyFlight(State s, double t_f);
State applyAction(State s, Action a);
State applyStanceReverse(State s, Action a, double t);
State applyStanceReverse(State s, Action a);
std::array<double, 3> rotate_grf(std::array<double, 3> surface_norm, std::array<double, 3> grf);
// planning_utils.cpp:519-556 (host arithmetic)
bool isValidAction(Action a);
// planning_utils.cpp:562-635 — evaluated by the engine
bool isValidState(State s, FastTerrainMap &terrain, int phase);
// planning_utils.cpp:645-881 — evaluated by the engine; s_new / t_new are
// written only where the reference writes them
bool isValidStateActionPair(State s, Action a, FastTerrainMap &terrain, State &s_new, double &t_new,
                            bool state_action_pair_check_adaptive_step_size_flag);
bool isValidStateActionPair(State s, Action a, FastTerrainMap &terrain, State &s_new, double &t_new);
bool isValidStateActionPair(State s, Action a, FastTerrainMap &terrain);
bool isValidStateActionPairAdaptiveStepSize(State s, Action a, FastTerrainMap &terrain,
                                            State &s_new, double &t_new);
bool isValidStateActionPairReverse(State s, Action a, FastTerrainMap &terrain, State &s_new,
                                   double &t_new, bool state_action_pair_check_adaptive_step_size_flag);
bool isValidStateActionPairReverse(State s, Action a, FastTerrainMap &terrain, State &s_new,
                                   double &t_new);
bool isValidStateActionPairReverse(State s, Action a, FastTerrainMap &terrain);
bool isValidStateActionPairReverseAdaptiveStepSize(State s, Action a, FastTerrainMap &terrain,
                                                   State &s_new, double &t_new);
// the hot path, batched: one engine launch for n pairs (direction per pair)
void isValidStateActionPairBatch(const std::vector<State> &s, const std::vector<Action> &a,
                                 const std::vector<uint8_t> &direction, FastTerrainMap &terrain,
                                 bool adaptive, std::vector<uint8_t> &valid,
                                 std::vector<State> &s_new, std::vector<double> &t_new,
                                 std::vector<uint32_t> *flags = nullptr);
// planning_utils.cpp:379-515 on the engine's counter-based stream (the
// reference's rand() / clock-seeded engines are not reproducible): draw k of
// the process's free-function stream (seed setRandomSeed, index k counting up
// per thread), sampled by the engine on device 0 (gbp_sample_actions_dir_host)
Action getRandomAction(std::array<double, 3> surf_norm, int direction,
                       bool action_direction_sampling_flag,
                       double action_direction_sampling_probability_threshold, State s,
                       State s_near);                                       // :379-391
Action getRandomAction(std::array<double, 3> surf_norm);                    // :392-442
Action getRandomActionDirection(std::array<double, 3> surf_norm, State s_from,
                                State s_to);                                // :443-515
void setRandomSeed(uint64_t seed);
// planning_utils.cpp:142-193
void interpStateActionPair(State s, Action a, double t0, double dt,
                           std::vector<State> &interp_path, std::vector<double> &interp_t,
                           std::vector<int> &interp_phase);
void getInterpPath(std::vector<State> state_sequence, std::vector<Action> action_sequence,
                   double dt, std::vector<State> &interp_path, std::vector<double> &interp_t,
                   std::vector<int> &interp_phase);
}  // namespace planning_utils

struct TreeView;  // csrc/host/gbp_tree_path.h
struct JoinedPath;

// A device allocation owned by its holder (gbp_device_alloc / gbp_device_free):
// move-only, freed in the destructor.
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer &&o) noexcept { *this = std::move(o); }
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept;
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer &operator=(const DeviceBuffer &) = delete;
  ~DeviceBuffer();
  // room for n elements of elem_bytes: a new allocation of max(min_elems,
  // capacity) elements doubled until n fit, holding nothing valid (valid = 0)
  void reserve(int device, int64_t n, size_t elem_bytes, int64_t min_elems, const char *what);
  template <class T = void>
  T *data() const { return static_cast<T *>(p_); }
  int64_t capacity() const { return cap_; }
  int64_t valid = 0;  // leading elements that hold the holder's current data

 private:
  void *p_ = nullptr;
  int64_t cap_ = 0;
};

// ---- GraphClass + PlannerClass (graph_class.h, planner_class.h) --------------
// Vertices live in host vectors AND in a device mirror (flat double[V][8]) that
// the nearest-neighbour kernel scans.
class PlannerClass {
 public:
  explicit PlannerClass(int device = 0);

  void init(State s, bool cost_add_yaw_flag = false, double cost_add_yaw_length_weight = 1,
            double cost_add_yaw_yaw_weight = 1);                           // graph_class.cpp:141-152
  void addVertex(int index, State s);                                      // :28-31
  State getVertex(int index) const { return vertices_[index]; }            // :18-20
  int getNumVertices() const { return (int)vertices_.size(); }             // :23-25
  void addEdge(int idx1, int idx2);                                        // :36-42
  void removeEdge(int idx1, int idx2);                                     // :44-58
  int getPredecessor(int idx) const;                                       // :62-68
  std::vector<int> getSuccessors(int idx) const { return successors_[idx]; }
  void addAction(int idx, Action a) { actions_[idx] = a; }                 // :75-77
  Action getAction(int idx) const { return actions_[idx]; }
  double getGValue(int idx) const { return g_[idx]; }
  double getYValue(int idx) const { return y_[idx]; }
  void updateGYValue(int idx, double g_val, double y_val);                 // :131-138

  // planner_class.cpp:38-76 on the engine sampler (stream = this tree's id)
  State randomState(FastTerrainMap &terrain);
  // planner_class.cpp:22-35: randomStateDirection with probability p, else
  // randomState (one draw of this tree's stream either way)
  State randomState(FastTerrainMap &terrain, bool state_direction_sampling_flag,
                    double state_direction_sampling_probability_threshold,
                    bool speed_direction_flag, State s_from, State s_to);
  // planner_class.cpp:82-148
  State randomStateDirection(FastTerrainMap &terrain, State s_from, State s_to,
                             bool speed_direction_flag);
  // n consecutive randomState draws of this tree's stream in one launch
  std::vector<State> randomStateBatch(FastTerrainMap &terrain, int n);
  // ... with the direction-biased variant of cfg (s_from / s_to for all n)
  std::vector<State> randomStateBatch(FastTerrainMap &terrain, int n, const gbp_sampling &cfg,
                                      const State &s_from, const State &s_to);
  // planner_class.cpp:185-200 on the engine (ties -> lowest index)
  int getNearestNeighbor(State q);
  std::vector<int> getNearestNeighborBatch(const std::vector<State> &q);
  std::vector<int> neighborhoodDist(State q, double dist);                 // :173-182
  // neighborhoodDist for many queries in one launch; query k only sees
  // vertices with index < limit[k] (limit empty: all), ascending index
  std::vector<std::vector<int>> neighborhoodDistBatch(const std::vector<State> &q, double dist,
                                                      const std::vector<int> &limit = {});
  // :151-171: the engine's k-nearest wavefront scan (N <= GBP_KNN_MAX, plain
  // stateDistance), else (cost_add_yaw's weighted distance) a host sort
  std::vector<int> neighborhoodN(State q, int N);

  void setStream(uint64_t seed, uint64_t stream_id) {
    seed_ = seed;
    stream_id_ = stream_id;
  }
  const std::vector<State> &vertices() const { return vertices_; }
  // the host arrays as the path join reads them (csrc/host/gbp_tree_path.h)
  TreeView treeView() const;

 private:
  void sync_device();
  void sync_yaw();  // the vertices' glibc yaws on the device (cost_add_yaw neighborhoodN)
  void ensure_scratch(int64_t nq);
  int device_;
  std::vector<State> vertices_;
  std::vector<Action> actions_;
  std::vector<int> parent_;
  std::vector<std::vector<int>> successors_;
  std::vector<double> g_, y_;
  bool cost_add_yaw_flag_ = false;
  double cost_add_yaw_length_weight_ = 1, cost_add_yaw_yaw_weight_ = 1;
  // The device side is a cache of the host vectors, refilled on demand: a
  // copy of a tree starts without one.
  struct Mirror {
    DeviceBuffer vertices;  // [V][8]
    DeviceBuffer yaw;       // atan2(v[4], v[3]) per vertex (glibc), uploaded on demand
    DeviceBuffer scratch;   // nearest-neighbour queries [q][8] + indices [q]
    DeviceBuffer nbr;       // neighbourhood queries + output lists (bytes)
    Mirror() = default;
    Mirror(Mirror &&) = default;
    Mirror &operator=(Mirror &&) = default;
    Mirror(const Mirror &) {}
    Mirror &operator=(const Mirror &o) { return this == &o ? *this : *this = Mirror(); }
  } d_;
  uint64_t seed_ = 1, stream_id_ = 100;
  int64_t draws_ = 0;
};

// ---- RRTClass / RRTConnectClass (rrt.h, rrt_connect.h) -------------------------
class RRTClass {
 public:
  RRTClass() = default;
  virtual ~RRTClass() = default;
  // rrt.cpp:20-70 (candidates drawn from the engine stream, checked in one launch)
  bool newConfig(State s, State s_near, State &s_new, Action &a_new, FastTerrainMap &terrain,
                 int direction);
  // rrt.cpp:77-102
  virtual int extend(PlannerClass &T, State s, FastTerrainMap &terrain, int direction);
  std::vector<int> pathFromStart(PlannerClass &T, int idx);                // rrt.cpp:107-118
  std::vector<State> getStateSequence(PlannerClass &T, std::vector<int> path);
  std::vector<Action> getActionSequence(PlannerClass &T, std::vector<int> path);
  // rrt.cpp:154-169 (same 10 outputs)
  void getStatistics(double &plan_time, int &success_var, int &vertices_generated,
                     double &time_to_first_solve, std::vector<double> &length_vector,
                     std::vector<double> &yaw_vector, std::vector<double> &cost_vector,
                     std::vector<double> &cost_vector_times, double &path_duration,
                     std::vector<std::vector<double>> &allStatePosition);
  void printPath(PlannerClass &T, std::vector<int> path);                  // rrt.cpp:143-152
  void saveStateSequence(PlannerClass &T);                                 // rrt.cpp:253-265
  // rrt.cpp:268-280 (params.yaml:21-27, off by default): newConfig's
  // candidates and every search's targets (sequential, batched and
  // device-resident) draw the direction-biased variants when a flag is on
  // (gbp_sampling, applied to the terrain handle the search runs on)
  void set_action_direction_sampling(bool flag, double threshold) {
    action_direction_sampling_flag_ = flag;
    action_direction_sampling_probability_threshold_ = threshold;
  }
  void set_state_direction_sampling(bool flag, double threshold, bool speed_direction_flag) {
    state_direction_sampling_flag_ = flag;
    state_direction_sampling_probability_threshold_ = threshold;
    state_direction_sampling_speed_direction_flag_ = speed_direction_flag;
  }
  // informed sampling (gbp.h gbp_informed; 0 = off, the reference's behaviour):
  // the batched and the device-resident searches draw their targets inside the
  // ellipse of (s_start, s_goal, cost), fixed for the whole run, so both draw
  // the same targets; any cost at or above a known path's is admissible
  void set_informed_cost(double cost) { informed_cost_ = cost; }
  double informedCost() const { return informed_cost_; }
  void print_setting_parameters();
  void set_state_action_pair_check_adaptive_step_size_flag_(bool f) {
    state_action_pair_check_adaptive_step_size_flag_ = f;
  }
  void set_cost_add_yaw(bool flag, double lw, double yw) {
    cost_add_yaw_flag_ = flag;
    cost_add_yaw_length_weight_ = lw;
    cost_add_yaw_yaw_weight_ = yw;
  }
  void setSeed(uint64_t seed) { seed_ = seed; }
  // wall clock from the start of the build call to the first goal (the
  // reference's elapsed_to_first restarts with every tree pair)
  double wallTimeToFirst() const { return wall_to_first_; }
  // the last build's path cost / its history (rrt_connect.h getters' data)
  double pathCost() const { return path_cost_; }
  double pathLength() const { return path_length_; }
  double pathYaw() const { return path_yaw_; }
  // the reference's path cost: length, or the cost_add_yaw weighted sum
  // (rrt_connect.cpp:304-313, :193-215)
  double weightedCost(double length, double yaw) const {
    return cost_add_yaw_flag_ ? length * cost_add_yaw_length_weight_ + yaw * cost_add_yaw_yaw_weight_
                              : length;
  }
  const std::vector<double> &costHistory() const { return cost_vector_; }
  // this planner's direction-sampling parameters as the engine's gbp_sampling
  gbp_sampling samplingConfig() const;

 protected:
  // installs samplingConfig() on the terrain handle (the candidate sampler and
  // the device loop's targets read it there)
  void applySampling(FastTerrainMap &terrain) const;
  // set_informed_cost's ellipse on the terrain handle for the lifetime of the
  // object (a build call); the handle's own setting comes back afterwards.
  // With the cost off nothing is touched.
  class InformedScope {
   public:
    InformedScope(const RRTClass &p, FastTerrainMap &terrain, const State &s_start,
                  const State &s_goal);
    ~InformedScope();
    InformedScope(const InformedScope &) = delete;
    InformedScope &operator=(const InformedScope &) = delete;

   private:
    gbp_terrain *t_;
    gbp_informed saved_{};
    bool set_ = false;
  };
  double informed_cost_ = 0;
  // a search's two trees from their roots: Ta at s_start drawing from Philox
  // stream stream_a of this planner's seed, Tb at s_goal from stream_b
  void initTreePair(PlannerClass &Ta, PlannerClass &Tb, const State &s_start, const State &s_goal,
                    uint64_t stream_a, uint64_t stream_b) const;
  // hands out a search's joined path and reports its length, yaw, cost
  // (rrt_connect.cpp:304-313) and duration
  void reportPath(JoinedPath &&path, std::vector<State> &state_sequence,
                  std::vector<Action> &action_sequence);
  bool goal_found = false;
  std::chrono::duration<double> elapsed_total{0};
  std::chrono::duration<double> elapsed_to_first{0};
  double wall_to_first_ = -1;
  int success_ = 0;
  int num_vertices = 0;
  double path_length_ = 0, path_yaw_ = 0, path_cost_ = 0;
  std::vector<double> length_vector_, yaw_vector_, cost_vector_, cost_vector_times_;
  double path_duration_ = 0;
  std::vector<std::vector<double>> allStatePosition_;
  bool action_direction_sampling_flag_ = false;
  double action_direction_sampling_probability_threshold_ = 0.15;
  bool state_direction_sampling_flag_ = false;
  double state_direction_sampling_probability_threshold_ = 0.05;
  bool state_direction_sampling_speed_direction_flag_ = false;
  bool state_action_pair_check_adaptive_step_size_flag_ = false;
  bool cost_add_yaw_flag_ = false;
  double cost_add_yaw_length_weight_ = 1, cost_add_yaw_yaw_weight_ = 1;
  uint64_t seed_ = 20251018;
  int64_t extend_counter_ = 0;
};

// The final trees of a batched / device-resident search (for callers that
// replay it, e.g. against a CPU restatement): Ta = [0], Tb = [1].
struct TreeDump {
  std::vector<State> v[2];
  std::vector<Action> a[2];
  std::vector<int32_t> parent[2];
  std::vector<double> g[2];
};

struct BatchStats {
  int64_t max_halves = 0;     // in: stop after this many half-iterations (0 = no limit)
  TreeDump *dump = nullptr;   // in: receives the final trees when set
  // in (device loop): called after every group of halves with this rank's own
  // verdict (local_stop: found, out of time or halves) and whether it found a
  // path; returns nonzero to stop — config 4's ranks answer it with one
  // all_reduce(MAX) of local_stop, so they stop together
  int (*stop_poll)(void *ctx, int local_stop, int found) = nullptr;
  void *stop_ctx = nullptr;
  int64_t polls = 0;          // stop polls made
  int stopped_by_peer = 0;    // the poll stopped a search this rank would have continued
  int64_t halves = 0;         // half-iterations run
  int32_t meet_a = -1, meet_b = -1;  // the joined vertices (RRT*: the best pair)
  int64_t iterations = 0, targets = 0, extends = 0, attempts_checked = 0, connects = 0;
  int64_t vertices_a = 0, vertices_b = 0;
  int64_t rewires = 0, solutions = 0;
  int64_t depth_capped = 0;   // connects stopped at GBP_CONNECT_MAX_DEPTH (TRAPPED)
  int64_t status_reads = 0;   // device loop: host synchronisations
  int64_t fragile_resolved = 0;  // attempts re-decided on the host (GBP_F_RESOLVED)
  int64_t halts[4] = {0, 0, 0, 0};  // device loop: FRAGILE halts in the targets / extend /
                                    // connect / RRT* insertion stage (GBP_PLAN_HALT_*)
  int64_t star_grows = 0;           // device RRT*: insertion sets grown (GBP_PLAN_HALT_STAR_PAIRS)
  int64_t nn_rechecks = 0, nn_scans = 0;  // device loop with GBP_OPT_NN_STATS: the matrix-core
                                          // search's fp64 half-chunk re-checks / segment scans
  double extent_a[4] = {0, 0, 0, 0}, extent_b[4] = {0, 0, 0, 0};  // x_min x_max y_min y_max
  // in (device loop): a warm start, i.e. a replayable continuation of a search
  // (0 vertices = from the roots).  Tree k starts as warm_n[k] vertices (root
  // first, parents before children; g derived as graph_class.cpp:36-42 does),
  // the first half-iteration is warm_half (its targets are the draws a search
  // from the roots would make there) and the candidate stream starts at extend
  // index warm_extend.  max_halves then counts the continuation's halves.
  int64_t warm_n[2] = {0, 0};
  const double *warm_v[2] = {nullptr, nullptr};
  const double *warm_a[2] = {nullptr, nullptr};
  const int32_t *warm_parent[2] = {nullptr, nullptr};
  int64_t warm_half = 0, warm_extend = 0;
  // in (buildRRTStarConnectDevice's warm start): the kept connections the
  // continuation starts with, warm_shared_n pairs (vertex of tree 0, vertex of
  // tree 1) in list order, loaded and ranked on the device
  // (gbp_plan_shared_load_host) once the warm trees are: the search then
  // continues the earlier run's list and best instead of starting a new
  // ranking.  Without it a warm start begins with no connection, as before.
  const int32_t *warm_shared = nullptr;
  int64_t warm_shared_n = 0;
  // in (buildRRTStarConnectDevice): receives the final list of kept connections when set
  std::vector<std::array<int32_t, 2>> *shared_dump = nullptr;
  // diagnostics (device loop): time each half-iteration's stage groups
  // (gbp_plan_stage_timing) into stage_us (half, stages 0-3, 6, 7, 4-5)
  bool stage_timing = false;
  double stage_us[7] = {0, 0, 0, 0, 0, 0, 0};
  int64_t stage_halves = 0;
};

// What RRTConnectClass::revalidateTrees did to one tree (gbp_prune_stats,
// include/gbp.h, and the FRAGILE edges re-decided on the host with glibc).
struct PruneStats {
  int64_t n_before = 0;        // vertices before the prune
  int64_t n_kept = 0;          // ... and after it
  int64_t n_edge_invalid = 0;  // pruned vertices whose own edge failed on the new map
  int64_t n_inherited = 0;     // pruned only because an ancestor was
  int64_t fragile_resolved = 0;
};

// What RRTConnectClass::rerootStartTree did (gbp_reroot_stats, include/gbp.h,
// and the FRAGILE edges re-decided on the host with glibc).
struct RerootStats {
  int64_t n_before = 0;        // vertices of the start tree before
  int64_t n_kept = 0;          // ... and after: the new root and what stays below it
  int64_t n_outside = 0;       // dropped: not below the new root
  int64_t n_edge_invalid = 0;  // dropped: below it, own edge failed on the map
  int64_t n_inherited = 0;     // dropped: below it, only because an ancestor was
  int64_t depth = 0;           // most edges between the new root and a kept vertex
  int64_t fragile_resolved = 0;
};

// What RRTConnectClass::graftStartTree and ReplanSession::robotOff / goalAt
// did (gbp_graft_stats, include/gbp.h, and the FRAGILE checks and edges
// re-decided on the host with glibc).
struct GraftStats {
  int64_t n_before = 0;        // vertices of the tree before
  int64_t n_kept = 0;          // ... and after: the new root and what hangs below it
  int64_t n_candidates = 0;    // vertices within the radius of the new root
  int64_t n_checked = 0;       // pair checks run for them
  int64_t n_attached = 0;      // children of the new root
  int64_t n_outside = 0;       // dropped: no attached vertex on the parent chain
  int64_t n_edge_invalid = 0;  // dropped: below one, own edge failed on the map
  int64_t n_inherited = 0;     // dropped: below one, only because an ancestor was
  int64_t depth = 0;           // most edges between the new root and a kept vertex
  int64_t fragile_resolved = 0;
};

class RRTConnectClass : public RRTClass {
 public:
  // rrt_connect.cpp:20-84 (recursive; the pair checks run on the engine)
  int attemptConnect(State s_existing, State s, double t_s, State &s_new, Action &a_new,
                     FastTerrainMap &terrain, int direction);
  // rrt_connect.cpp:85-91
  int attemptConnect(State s_existing, State s, State &s_new, Action &a_new, FastTerrainMap &terrain,
                     int direction);
  int connect(PlannerClass &T, State s, FastTerrainMap &terrain, int direction);  // :98-120
  std::vector<Action> getActionSequenceReverse(PlannerClass &T, std::vector<int> path);
  void postProcessPath(std::vector<State> &state_sequence, std::vector<Action> &action_sequence,
                       FastTerrainMap &terrain);                                    // :139-227
  void runRRTConnect(PlannerClass &Ta, PlannerClass &Tb, FastTerrainMap &terrain);  // :230-314
  void buildRRTConnect(FastTerrainMap &terrain, State s_start, State s_goal,
                       std::vector<State> &state_sequence, std::vector<Action> &action_sequence,
                       double max_time);                                            // :323-467

  // Batch-synchronous RRT-Connect: each half-iteration draws `batch` targets,
  // extends the tree toward all of them against the current snapshot (one
  // engine launch, 6 candidates each), inserts the non-TRAPPED successors in
  // target order, then connects every new vertex to the other tree with the
  // recursive attemptConnect run as lock-step rounds (one launch per round).
  // batch = 1 is runRRTConnect.  Stops at the first solution or max_time.
  bool buildRRTConnectBatched(FastTerrainMap &terrain, State s_start, State s_goal, int batch,
                              double max_time, std::vector<State> &state_sequence,
                              std::vector<Action> &action_sequence, BatchStats *stats = nullptr);

  // buildRRTConnectBatched with the whole search resident on the device
  // (include/gbp.h "device planner loop"): both trees live in HBM, every
  // half-iteration (targets, nearest neighbours, extends, appends, connects)
  // is one stream-ordered kernel sequence with no host round trip, and the
  // host reads one status record per group of half-iterations.  Same RNG
  // streams, same insertion order, same FRAGILE re-decisions as
  // buildRRTConnectBatched: for a given (seed, batch) both build the same trees
  // and return the same path.
  bool buildRRTConnectDevice(FastTerrainMap &terrain, State s_start, State s_goal, int batch,
                             double max_time, std::vector<State> &state_sequence,
                             std::vector<Action> &action_sequence, BatchStats *stats = nullptr,
                             uint64_t stream_a = 101, uint64_t stream_b = 102);

  // buildRRTConnect's anytime restarts (rrt_connect.cpp:323-467) on the
  // batch-synchronous half-iterations: fresh trees every restart, a restart
  // ends after anytime_horizon seconds (poseDistance(start, goal) /
  // planning_rate_estimate, x horizon_expansion_factor per restart) or at its
  // first REACHED connect; every solution is post-processed and the cheapest
  // (path_cost_) kept.  Stops once a solution exists and max_time_opt has
  // passed, or at max_time without one.  Returns the best path.
  // device_loop: each restart's search runs device-resident (buildRRTConnectDevice).
  bool buildRRTConnectBatchedAnytime(FastTerrainMap &terrain, State s_start, State s_goal,
                                     int batch, double max_time, double max_time_opt,
                                     std::vector<State> &state_sequence,
                                     std::vector<Action> &action_sequence,
                                     BatchStats *stats = nullptr, bool device_loop = false);

  // How buildRRTConnect (the call GlobalBodyPlanner::callPlanner makes,
  // global_body_planner.cpp:115) searches: batch > 0 (default 1024) runs its
  // restart loop on the device-resident batched search with that many random
  // targets per half-iteration; 0 runs the reference's sequential
  // runRRTConnect, one engine call per extend / connect.
  void set_engine_batch(int batch) { engine_batch_ = batch; }
  int engine_batch() const { return engine_batch_; }
  // postProcessPath's connect decisions as one table launch
  // (gbp_shortcut_paths_host) instead of one attemptConnect per popped
  // candidate: the same kept states, actions and path_length_ / path_yaw_ /
  // path_cost_.  Off by default.
  void set_post_process_device(bool on) { post_process_device_ = on; }
  bool post_process_device() const { return post_process_device_; }

  // The map changed (the node's terrainMapCallback, global_body_planner.cpp:37-44,
  // loads a new one): what of an earlier search's trees (BatchStats::dump; Ta
  // grown FORWARD, Tb REVERSE) a search on `terrain` may start from.  Each tree
  // is loaded into HBM and pruned there (gbp_tree_revalidate_host, with this
  // object's adaptive-step flag): a vertex stays when every edge between it and
  // the root still passes its pair check on `terrain`; the roots are kept
  // untested.  `trees` is left holding the survivors, ready for
  // BatchStats::warm_*; remap (optional, one vector per tree) receives each old
  // vertex's new index or -1, for callers that carry vertex indices of their
  // own (RRT*'s kept connections) across the prune.  Both trees are decided
  // before either is changed: a call that throws (EngineError) leaves trees,
  // stats and remap as they were.
  void revalidateTrees(FastTerrainMap &terrain, TreeDump &trees, PruneStats stats[2],
                       std::vector<int32_t> remap[2] = nullptr);

  // The robot moved: at the next call it stands on `vertex` of the start tree
  // (tree 0 of an earlier search's dump, grown FORWARD; gbp_tree_path.h finds
  // the vertex of a path state).  The tree is loaded into HBM and re-rooted
  // there (gbp_tree_reroot_host): `vertex` becomes vertex 0, the subtree below
  // it follows in ascending old index, and the rest goes, because the dynamics
  // are not reversible.  With test_edges the map changed as well: the edges
  // are tested FORWARD on `terrain` (this object's adaptive-step flag, FRAGILE
  // ones re-decided with glibc) and a vertex stays only when every edge
  // between it and the new root holds.  Tree 0 of `trees` is left holding the
  // survivors with g derived again from the new root, ready for
  // BatchStats::warm_* of a search from trees.v[0][0]; tree 1 is not touched
  // (revalidateTrees prunes it when the map changed).  remap (optional)
  // receives each old vertex's new index or -1.  A call that throws
  // (EngineError) leaves trees, stats and remap as they were.
  void rerootStartTree(FastTerrainMap &terrain, TreeDump &trees, int32_t vertex, RerootStats &stats,
                       std::vector<int32_t> *remap = nullptr, bool test_edges = false);

  // The robot is off the tree: at the next call it stands on state `s`, which
  // need not be a vertex (part of the way through an action, or drifted off
  // the plan).  Tree 0 of `trees` is loaded into HBM and grafted there
  // (gbp_tree_graft_host, FORWARD): every vertex within `radius` that s
  // connects to directly on `terrain` becomes a child of s by that connect
  // action, and a vertex stays when such a vertex lies on its parent chain
  // (with test_edges: and every edge up to the nearest one holds on
  // `terrain`).  Tree 0 is left holding s as vertex 0 and the survivors in
  // ascending old index with g derived again, ready for BatchStats::warm_* of a
  // search from s; with nothing attached it holds s alone.  s itself is the
  // caller's to test (isValidState).  tree 1 is not touched.  remap (optional)
  // receives each old vertex's new index or -1.  A call that throws
  // (EngineError) leaves trees, stats and remap as they were.
  void graftStartTree(FastTerrainMap &terrain, TreeDump &trees, const State &s, double radius,
                      GraftStats &stats, std::vector<int32_t> *remap = nullptr,
                      bool test_edges = false);

  // attemptConnect for many independent pairs (lock-step rounds, one engine
  // launch per recursion depth); s_new / a_new are in/out per pair
  void attemptConnectBatchPublic(const std::vector<State> &s_existing, const std::vector<State> &s,
                                 std::vector<double> t_s, FastTerrainMap &terrain, int direction,
                                 std::vector<int> &result, std::vector<State> &s_new,
                                 std::vector<Action> &a_new) {
    attemptConnectBatch(s_existing, s, std::move(t_s), terrain, direction, result, s_new, a_new,
                        nullptr);
  }

 protected:
  double anytime_horizon = 0;
  const double planning_rate_estimate = 16.0;
  double horizon_expansion_factor = 1.2;
  const int max_time_solve = 4000;
  int engine_batch_ = 1024;
  bool post_process_device_ = false;

  // rrt_connect.cpp:398-414: post-process a found path and, when it is cheaper
  // than cost_so_far, make it the new cost_so_far and add it to the length /
  // yaw / cost histories.  Returns whether it was kept; the caller then stores
  // its best and pushes the time into cost_vector_times_.
  bool keepIfCheaper(std::vector<State> &state_sequence, std::vector<Action> &action_sequence,
                     FastTerrainMap &terrain, double &cost_so_far);

  // lock-step attemptConnect for many (s_existing, s, t_s) triples; with
  // max_depth = 0 only REACHED is decided (callers that test == REACHED)
  void attemptConnectBatch(const std::vector<State> &s_existing, const std::vector<State> &s,
                           std::vector<double> t_s, FastTerrainMap &terrain, int direction,
                           std::vector<int> &result, std::vector<State> &s_new,
                           std::vector<Action> &a_new, BatchStats *stats,
                           int max_depth = GBP_CONNECT_MAX_DEPTH);
  // connect each vertex `added` of T to the other tree O (rrt_connect.cpp:98-120,
  // in order, NN against O's snapshot); returns the (T vertex, O vertex) pairs
  // whose connect REACHED
  std::vector<std::pair<int, int>> connectBatch(PlannerClass &T, PlannerClass &O,
                                                FastTerrainMap &terrain, int dir,
                                                const std::vector<int> &added, BatchStats *stats);
  // draw `batch` targets, keep the STANCE-valid ones, extend T toward all of
  // them against T's snapshot; returns the inserted vertices (in target order),
  // their nearest vertices and actions.  With O, the targets are
  // randomState(terrain, state_direction_sampling_*, s_from, s_to) with the
  // reference's s_from / s_to (rrt_connect.cpp:248-252, :283-287) as the
  // trees stand when the half starts; without, plain randomState (RRT*).
  void extendBatch(PlannerClass &T, FastTerrainMap &terrain, int dir, int batch,
                   std::vector<int> &added, std::vector<int> &nearest, std::vector<Action> &a_new,
                   bool insert, BatchStats *stats, const PlannerClass *O = nullptr);
  int halfIterationBatched(PlannerClass &T, PlannerClass &O, FastTerrainMap &terrain, int dir,
                           int batch, int &meet_t, int &meet_o, BatchStats *stats);
};

// ---- RRTStarConnectClass (rrt_star_connect.h, rrt_star_connect.cpp) ------------
class RRTStarConnectClass : public RRTConnectClass {
 public:
  // rrt_star_connect.cpp:11-67: newConfig, then choose-parent among the
  // vertices within delta and rewire them through s_new (connects on the engine)
  int extend(PlannerClass &T, State s, FastTerrainMap &terrain, int direction) override;
  // rrt_star_connect.cpp:70-89
  void getStateAndActionSequences(PlannerClass &Ta, PlannerClass &Tb, int shared_a_idx,
                                  int shared_b_idx, std::vector<State> &state_sequence,
                                  std::vector<Action> &action_sequence);
  // rrt_star_connect.cpp:91-205
  void buildRRTStarConnect(FastTerrainMap &terrain, State s_start, State s_goal,
                           std::vector<State> &state_sequence,
                           std::vector<Action> &action_sequence, double max_time);
  // Batch-synchronous RRT*-Connect: as buildRRTConnectBatched, with every new
  // vertex inserted by choose-parent + rewire (its neighbourhood = the vertices
  // within delta that precede it, as in the sequential algorithm); all
  // neighbourhood scans of a batch run in one launch and all their connects in
  // one pair-check launch, the tree updates then replay sequentially in order.
  // Runs until max_time after the first solution (anytime), keeping the best.
  bool buildRRTStarConnectBatched(FastTerrainMap &terrain, State s_start, State s_goal, int batch,
                                  double max_time, std::vector<State> &state_sequence,
                                  std::vector<Action> &action_sequence, BatchStats *stats = nullptr);
  // The same search resident on the device: gbp_plan_halves_dev with the RRT*
  // insertion stages (gbp_plan_star_config: neighbourhoods, connect checks and
  // the ordered choose-parent / rewire replay in HBM, no per-vertex host
  // loop); same trees, counters and best connection as buildRRTStarConnectBatched
  // for the same seed and batch.  Runs pairs of half-iterations until max_time
  // (or stats->max_halves), reading the status once per group.
  bool buildRRTStarConnectDevice(FastTerrainMap &terrain, State s_start, State s_goal, int batch,
                                 double max_time, std::vector<State> &state_sequence,
                                 std::vector<Action> &action_sequence, BatchStats *stats = nullptr);
  double bestCost() const { return best_cost_; }
  int64_t rewires() const { return rewires_; }

 protected:
  const double delta = 3.0;  // rrt_star_connect.h:59
  double best_cost_ = INFINITY_COST;
  int64_t rewires_ = 0;
  static constexpr double INFINITY_COST = 1.7976931348623157e308;

 private:
  // choose-parent + rewire for the new vertices `added` of T (in order)
  void insertStar(PlannerClass &T, FastTerrainMap &terrain, int dir, const std::vector<int> &added,
                  const std::vector<int> &nearest, const std::vector<Action> &a_new,
                  BatchStats *stats);
};

// ---- ReplanSession: RRT*-Connect kept alive on the device between plans ---------
// What gbp_plan_shared_remap_dev did to the list of kept connections.
struct SharedStats {
  int64_t n_before = 0;     // connections listed before
  int64_t n_kept = 0;       // ... and after
  int64_t n_dropped_a = 0;  // dropped: its start-tree vertex is gone
  int64_t n_dropped_b = 0;  // dropped: only its goal-tree vertex is gone
};

// What ReplanSession::trim did to one tree (gbp_trim_stats, include/gbp.h).
struct TrimStats {
  int64_t n_before = 0;       // vertices before the trim
  int64_t n_kept = 0;         // ... and after it
  int64_t n_over_bound = 0;   // vertices with g + h above the held best cost
  int64_t n_over_budget = 0;  // not over the bound, but outside the vertex budget
  int64_t n_protected = 0;    // of those two groups: on the best connection's chain, kept
  int64_t n_inherited = 0;    // dropped only because an ancestor was
  double cut = std::numeric_limits<double>::infinity();  // the budget's cut in g + h (+inf: none applied)
};

// The node's loop (terrainMapCallback, then callPlanner on every tick,
// global_body_planner.cpp:37-131) against one search that stays in HBM: the
// stream, the plan workspace, both trees and RRT*'s list of kept connections
// outlive a call.  The search is buildRRTStarConnectDevice's (algorithm 5: the
// one that keeps many connections and runs anytime); an RRT-Connect session
// is not offered.  Planner settings (seed aside: begin takes it) are this
// object's, set through RRTStarConnectClass's setters before begin.
//   begin      sets the search up as buildRRTStarConnectDevice does.
//   search     runs pairs of half-iterations until max_time or max_halves of
//              this call; halves and the extend counter go on from the last
//              call.  A session that has only called begin and search holds
//              the trees, list and best of buildRRTStarConnectDevice with the
//              same arguments.  Returns whether a connection is held.
//   mapChanged the terrain handle was updated in place (updateData /
//              updateDataFlat) or its window moved (moveDataFlat /
//              moveFromGridMap: the handle is the same one, so the session
//              goes on; a vertex whose edge now leaves the window is
//              GBP_F_OOD, hence invalid, hence pruned like any other, and the
//              roots are never tested: keeping them inside the window is the
//              caller's): both trees are pruned where they are and the
//              list is carried through the prunes' device remaps and ranked
//              again.  Neither the remaps nor the list come to the host; the
//              prune's own read-back (the edges' decisions and flags, for
//              the FRAGILE re-decision) stays.
//   robotAt    the robot stands on a vertex of the start tree (or on a state
//              of the current best path): the start tree is re-rooted there,
//              with test_edges its edges tested on the map as well, and the
//              list carried through that remap.  The State form costs more
//              than the vertex form: it extracts the best path (bestPath),
//              reads the start tree's parent array (4 bytes per vertex, no
//              state, action or g) for the chain's vertex indices
//              (startTreePath) and takes the first path state equal to s bit
//              for bit, as findStateAmong does on a dumped tree.  A caller
//              that tracks vertex indices should pass the vertex.
//   robotOff   the robot stands on a state that is no vertex: the start tree
//              is grafted onto it (gbp_tree_graft_keep_host, FORWARD, the
//              vertices within `radius` checked), with test_edges its edges
//              tested on the map as well, and the list carried through that
//              remap and ranked again (g has changed).  s is tested first,
//              isValidState(s, STANCE): false, with nothing changed, when it
//              fails.  With nothing attached the start tree is s alone and the
//              list empty: the next search grows it again.
//   goalAt     the same for a goal that moved, on the goal tree (REVERSE); s
//              may be valid in STANCE or in FLIGHT, as a goal root may be.
//   trim       bounds the trees: both are trimmed where they are
//              (gbp_tree_trim_keep_host), tree a toward b's root and tree b
//              toward a's, with bound = the held best cost (+inf when none is
//              held), at most max_vertices vertices per tree (0: no budget)
//              and the best connection's vertices best_a / best_b protected;
//              the list is then carried through both device remaps as
//              mapChanged carries it.  No terrain is involved.  The guarantee:
//              bestPath and the best cost are bit-identical before and after a
//              trim (a trim moves rows and changes no g, and the best
//              connection's two chains are kept whatever their f; with the
//              budget a tree may therefore keep max_vertices plus its chain's
//              length).  The heuristic's limit: g falls when a later rewire
//              finds a shorter way, so a trimmed vertex might have become
//              useful: the usual anytime-RRT* trade, and opt-in.
//   setTreeLimit  search then bounds the trees by itself: once per group of
//              halves, after the group's status read, when either tree holds
//              more than max_vertices it calls trim(trim_to).  Requires 1 <=
//              trim_to <= max_vertices; max_vertices = 0 (the default) is off
//              and changes nothing for a caller that never sets it.  The limit
//              is the object's: it outlives begin and end.
//   search's BatchStats: halves and iterations are added per call; rewires,
//              solutions, targets, extends, attempts_checked, connects,
//              fragile_resolved, depth_capped, vertices_* and meet_* are set
//              to the session's totals so far (the device status counts
//              from begin), so a caller summing calls must not add them.
//              costHistory() grows as in a build: the best cost once per
//              group of halves when it improved, and after a carry that
//              changed it.
//   bestPath   the joined path of the best kept connection, extracted on the
//              device (gbp_tree_path_host; one row of the goal tree is read
//              for the yaw sum, neither tree); fills pathLength / pathYaw /
//              pathCost as a build does.  False when no connection is held.
// The synchronous tree entries run on the terrain's own stream: the session
// synchronises its stream before them and they return synchronised.
class ReplanSession : public RRTStarConnectClass {
 public:
  ReplanSession();
  ~ReplanSession();
  ReplanSession(const ReplanSession &) = delete;
  ReplanSession &operator=(const ReplanSession &) = delete;
  void begin(FastTerrainMap &terrain, State s_start, State s_goal, int batch, double delta = 3.0,
             uint64_t seed = 20251018);
  bool search(double max_time, int64_t max_halves = 0, BatchStats *stats = nullptr);
  void mapChanged(FastTerrainMap &terrain, PruneStats stats[2], SharedStats *shared = nullptr);
  void robotAt(int32_t vertex, RerootStats &stats, SharedStats *shared = nullptr,
               bool test_edges = false);
  void robotAt(const State &s, RerootStats &stats, SharedStats *shared = nullptr,
               bool test_edges = false);
  bool robotOff(const State &s, double radius, GraftStats &stats, SharedStats *shared = nullptr,
                bool test_edges = false);
  bool goalAt(const State &s, double radius, GraftStats &stats, SharedStats *shared = nullptr,
              bool test_edges = false);
  // stats (may be null): tree a's record in [0], tree b's in [1]
  void trim(int64_t max_vertices, TrimStats stats[2], SharedStats *shared = nullptr);
  void setTreeLimit(int64_t max_vertices, int64_t trim_to);
  int64_t treeLimit() const { return tree_limit_; }
  int64_t treeTrimTo() const { return tree_trim_to_; }
  int64_t trimsBySearch() const { return trims_by_search_; }  // trims the limit has caused
  // Informed sampling (gbp.h gbp_informed), off by default; the
  // object's, like the tree limit: it outlives begin and end.  When on, the
  // session keeps the ellipse of (tree a's root, tree b's root, the status's
  // best cost, the map's bounds) on the terrain handle: computed once per
  // group of halves after the group's status read (where the tree limit is
  // tested) and after mapChanged, both robotAt, robotOff, goalAt and trim;
  // while no connection is held the handle's ellipse is off and the search is
  // the plain one, bit for bit.  The value is up to one group stale; the best
  // cost only falls and any cost at or above it is admissible.  It changes
  // only between groups, so a search of a given number of halves is
  // reproducible.  end() puts back what the handle held at begin (the terrain
  // must be alive then); the destructor does not touch the handle, so a session
  // destroyed without end() leaves its last ellipse there.  Turning it off
  // restores the handle's setting at once.
  void setInformed(bool on);
  bool informed() const { return informed_; }
  gbp_informed informedState() const;  // the handle's ellipse in force
  bool bestPath(std::vector<State> &state_sequence, std::vector<Action> &action_sequence);
  void dump(TreeDump &trees);
  // the kept connections in list order; best (optional): {best_a, best_b} or {-1, -1}
  void sharedConnections(std::vector<std::array<int32_t, 2>> &pairs,
                         std::array<int32_t, 2> *best = nullptr, double *best_cost = nullptr);
  void end();
  bool active() const { return impl_ != nullptr; }
  int32_t nextHalf() const;        // the half-iteration the next search starts with
  int64_t extendCounter() const;   // the candidate stream's next extend index

 private:
  struct Impl;
  Impl *impl_ = nullptr;
  int64_t tree_limit_ = 0, tree_trim_to_ = 0, trims_by_search_ = 0;
  bool informed_ = false;
  void updateInformed();  // the ellipse from the status as it stands (informed_ on)
  Impl &impl() const;  // throws EngineError(GBP_E_BAD_HANDLE) before begin
  void carryShared(bool remap_a, bool remap_b, const int64_t n_before[2], SharedStats *shared);
  bool graftTree(int k, const State &s, double radius, GraftStats &stats, SharedStats *shared,
                 bool test_edges);
};

// ---- implementation of the grid_map adapter (fast_terrain_map.cpp:31-91) -------
// Written against grid_map::GridMap's public API (getSize, getStartIndex,
// getPosition(Index, Position&), at(layer, Index), exists(layer)); a template
// so this header needs no grid_map build (not in this image; untested here).
template <class GridMap>
void FastTerrainMap::loadDataFromGridMap(const GridMap &map) {
  using Index = typename std::decay<decltype(map.getStartIndex())>::type;
  using Position = typename std::decay<decltype(map.getPosition())>::type;
  const int x_size = map.getSize()(0);
  const int y_size = map.getSize()(1);
  std::vector<double> x(x_size), y(y_size), z((size_t)x_size * y_size);
  const bool slopes = map.exists("dx");
  std::vector<double> dx, dy, dz;
  if (slopes) {
    dx.resize(z.size());
    dy.resize(z.size());
    dz.resize(z.size());
  }
  for (int i = 0; i < x_size; i++) {
    Index index((x_size - 1) - i, 0);
    Position position;
    map.getPosition(index, position);
    x[i] = position.x();
  }
  for (int i = 0; i < y_size; i++) {
    Index index(0, (y_size - 1) - i);
    Position position;
    map.getPosition(index, position);
    y[i] = position.y();
  }
  for (int i = 0; i < x_size; i++)
    for (int j = 0; j < y_size; j++) {
      Index index((x_size - 1) - i, (y_size - 1) - j);
      const size_t k = (size_t)i * y_size + j;
      z[k] = (double)map.at("elevation", index);
      if (slopes) {
        dx[k] = (double)map.at("dx", index);
        dy[k] = (double)map.at("dy", index);
        dz[k] = (double)map.at("dz", index);
      }
    }
  loadDataFlat(x_size, y_size, x.data(), y.data(), z.data(), slopes ? dx.data() : nullptr,
               slopes ? dy.data() : nullptr, slopes ? dz.data() : nullptr);
}

template <class GridMap>
bool FastTerrainMap::updateFromGridMap(const GridMap &map) {
  using Index = typename std::decay<decltype(map.getStartIndex())>::type;
  using Position = typename std::decay<decltype(map.getPosition())>::type;
  const int x_size = map.getSize()(0);
  const int y_size = map.getSize()(1);
  const bool slopes = map.exists("dx");
  bool same = handle_ && owned_ && x_size == x_size_ && y_size == y_size_ && slopes == slopes_ &&
              x_data_.size() == (size_t)x_size && y_data_.size() == (size_t)y_size;
  for (int i = 0; same && i < x_size; i++) {
    Index index((x_size - 1) - i, 0);
    Position position;
    map.getPosition(index, position);
    const double v = position.x();
    same = std::memcmp(&v, &x_data_[i], sizeof v) == 0;
  }
  for (int i = 0; same && i < y_size; i++) {
    Index index(0, (y_size - 1) - i);
    Position position;
    map.getPosition(index, position);
    const double v = position.y();
    same = std::memcmp(&v, &y_data_[i], sizeof v) == 0;
  }
  if (!same) {
    loadDataFromGridMap(map);
    return false;
  }
  std::vector<double> z((size_t)x_size * y_size), dx, dy, dz;
  if (slopes) {
    dx.resize(z.size());
    dy.resize(z.size());
    dz.resize(z.size());
  }
  for (int i = 0; i < x_size; i++)
    for (int j = 0; j < y_size; j++) {
      Index index((x_size - 1) - i, (y_size - 1) - j);
      const size_t k = (size_t)i * y_size + j;
      z[k] = (double)map.at("elevation", index);
      if (slopes) {
        dx[k] = (double)map.at("dx", index);
        dy[k] = (double)map.at("dy", index);
        dz[k] = (double)map.at("dz", index);
      }
    }
  updateDataFlat(0, 0, x_size, y_size, z.data(), slopes ? dx.data() : nullptr,
                 slopes ? dy.data() : nullptr, slopes ? dz.data() : nullptr);
  return true;
}

template <class GridMap>
bool FastTerrainMap::moveFromGridMap(const GridMap &map) {
  using Index = typename std::decay<decltype(map.getStartIndex())>::type;
  using Position = typename std::decay<decltype(map.getPosition())>::type;
  const int x_size = map.getSize()(0);
  const int y_size = map.getSize()(1);
  const bool slopes = map.exists("dx");
  bool same = handle_ && owned_ && x_size == x_size_ && y_size == y_size_ && slopes == slopes_ &&
              x_data_.size() == (size_t)x_size && y_data_.size() == (size_t)y_size;
  std::vector<double> x, y;
  int sx = 0, sy = 0;
  if (same) {
    x.resize(x_size);
    y.resize(y_size);
    for (int i = 0; i < x_size; i++) {
      Index index((x_size - 1) - i, 0);
      Position position;
      map.getPosition(index, position);
      x[i] = position.x();
    }
    for (int i = 0; i < y_size; i++) {
      Index index(0, (y_size - 1) - i);
      Position position;
      map.getPosition(index, position);
      y[i] = position.y();
    }
    same = gbp_coord_shift(x_data_.data(), x.data(), x_size, 1.0 / 1024, &sx) &&
           gbp_coord_shift(y_data_.data(), y.data(), y_size, 1.0 / 1024, &sy);
  }
  if (!same) {
    loadDataFromGridMap(map);
    return false;
  }
  std::vector<double> z((size_t)x_size * y_size), dx, dy, dz;
  if (slopes) {
    dx.resize(z.size());
    dy.resize(z.size());
    dz.resize(z.size());
  }
  for (int i = 0; i < x_size; i++)
    for (int j = 0; j < y_size; j++) {
      Index index((x_size - 1) - i, (y_size - 1) - j);
      const size_t k = (size_t)i * y_size + j;
      z[k] = (double)map.at("elevation", index);
      if (slopes) {
        dx[k] = (double)map.at("dx", index);
        dy[k] = (double)map.at("dy", index);
        dz[k] = (double)map.at("dz", index);
      }
    }
  moveDataFlat(sx, sy, x.data(), y.data(), z.data(), slopes ? dx.data() : nullptr,
               slopes ? dy.data() : nullptr, slopes ? dz.data() : nullptr);
  return true;
}

}  // namespace gbp_amd

// ---- flat C entry point of the batched planner (Python / bench) -------------
extern "C" {
typedef struct {
  int device, nx, ny;
  const double *x, *y, *z, *dx, *dy, *dz;  // x-major, dx/dy/dz may be NULL
  double start[8], goal[8];
  int batch;            // targets per half-iteration (1 = sequential runRRTConnect)
  double max_time;      // seconds
  uint64_t seed;
  int post_process;     // nonzero: run postProcessPath on the found path; 2: with its
                        // connect decisions as one table launch (set_post_process_device)
  int algorithm;        // 0 rrt-connect (first solution), 1 rrt-star-connect (anytime
                        // until max_time), 2 rrt-connect with the reference's anytime
                        // restarts (best post-processed path after max_time_opt),
                        // 3 rrt-connect with the search resident on the device
                        // (same trees and path as 0), 4 = 2 on the device-resident search,
                        // 5 = 1 with the search resident on the device (same trees)
  double max_time_opt;  // algorithm 2: keep restarting until a solution exists and this
                        // many seconds have passed (buildRRTConnect's max_time_opt)
  gbp_sampling sampling;  // direction-biased sampling (RRTClass::set_*_direction_sampling,
                          // params.yaml:21-27); all zero = off, the reference default
  int64_t fragile_eps_fm; // FRAGILE margin in 1e-15 units (GBP_OPT_FRAGILE_EPS); 0 = default
  int adaptive;           // state_action_pair_check_adaptive_step_size_flag (params.yaml:16)
  int nn_stats;           // GBP_OPT_NN_STATS: count the search's fp64 re-checks (diagnostics)
  int64_t max_halves;     // algorithms 0, 1, 3: stop after this many half-iterations
                          // (0 = no limit): a run that can be replayed exactly
  int64_t tree_capacity;  // rows of the tree_* buffers (0 = the trees are not returned)
  double *tree_v[2];      // algorithms 0, 1, 3: the final trees Ta / Tb — states [cap][8],
  double *tree_a[2];      //   the action reaching each vertex [cap][10] (root: zeros),
  int32_t *tree_parent[2];  // parents (root -1) and g values; rows past the result's
  double *tree_g[2];      //   vertices_a / vertices_b are not written
  int (*stop_poll)(void *ctx, int local_stop, int found);  // algorithm 3: see BatchStats
  void *stop_ctx;         //   (NULL: each run stops on its own)
  // algorithm 3: warm start (BatchStats::warm_*): init_n[k] vertices of tree k
  // (0 = the root given by start / goal), states [n][8], actions [n][10] and
  // parents [n] (root -1, parents before children); the first half-iteration
  // and the first extend index of the continuation
  int64_t init_n[2];
  const double *init_v[2];
  const double *init_a[2];
  const int32_t *init_parent[2];
  int64_t first_half;
  int64_t extend_base;
  int stage_timing;       // algorithms 3 / 5: time every half-iteration's stage groups
                          // (gbp_plan_stage_timing; diagnostics, adds events per half)
} gbp_plan_params;

typedef struct {
  int found;
  double time_to_first;  // wall seconds, build start -> first goal
  double total_time;
  int64_t iterations, targets, extends, attempts_checked, connects, vertices_a, vertices_b;
  int n_states;          // path states written (<= capacity)
  double path_length, path_cost, path_duration;
  int64_t rewires, solutions;  // RRT*: edges rewired, tree connections found
  double extent_a[4], extent_b[4];  // x_min, x_max, y_min, y_max of each tree's vertices
  int64_t fragile_resolved;    // decisions re-decided on the host with glibc (GBP_F_RESOLVED)
  int64_t depth_capped;        // connects stopped at GBP_CONNECT_MAX_DEPTH
  int64_t status_reads;        // algorithm 3: host synchronisations of the device loop
  int64_t halts[4];            // algorithm 3/4/5: FRAGILE halts in the targets / extend /
                               // connect / RRT* insertion stage of the device loop
  int64_t nn_rechecks, nn_scans;  // algorithm 3 with nn_stats: the matrix-core search's
                                  // fp64 half-chunk re-checks and segment scans
  double reported_length, reported_yaw;  // the planner's path_length_ / path_yaw_ (what
                                         // getStatistics reports; after postProcessPath
                                         // with its quirk, rrt_connect.cpp:202-215)
  int32_t meet_a, meet_b;      // algorithms 0 / 3: the vertices of Ta / Tb the first REACHED
                               // connect joined; algorithm 1: the best pair
  int64_t halves;              // half-iterations run
  int64_t polls;               // algorithm 3 with stop_poll: polls made
  int32_t stopped_by_peer;     // ... and 1 if another rank's solution ended this search
  double stage_us[7];          // with stage_timing: summed per-half microseconds
                               // (gbp_plan_stage_times: half, stages 0-3, 6, 7, 4-5,
                               // stage 6 before / in its pair checks)
  int64_t stage_halves;        //   over this many timed halves
} gbp_plan_result;

/* plans from start to goal; path_states[capacity][8] / path_actions[capacity][10]
 * (may be NULL).  Returns GBP_OK or a negative status. */
int gbp_plan_rrt_connect(const gbp_plan_params *p, gbp_plan_result *r, double *path_states,
                         double *path_actions, int capacity);

/* terrainArraysFromCSV (host only, no device): the FastTerrainMap arrays of
 * the reference's CSV -> grid_map -> FastTerrainMap path for the CSVs in dir.
 * Call with z == NULL to get nx / ny; then x[nx], y[ny], z/dx/dy/dz[nx][ny]
 * (x-major; any of dx/dy/dz may be NULL) are filled when capacity >= nx * ny.
 * Returns GBP_OK, GBP_E_SHAPE (capacity too small) or GBP_E_INVALID_ARG
 * (unreadable / non-square map). */
int gbp_terrain_arrays_from_csv(const char *dir, int *nx, int *ny, double *x, double *y,
                                double *z, double *dx, double *dy, double *dz, int64_t capacity);

/* RRTConnectClass::attemptConnect (rrt_connect.cpp:20-91) for n independent
 * (s_existing, s) pairs on an engine terrain handle, lock-step batched.
 * t_s[i] <= 0 (or t_s NULL) => poseDistance(s, s_existing) / V_NOM (:89).
 * s_new[n][8] / a_new[n][10] are in/out like the reference's references:
 * written only where the reference writes them.  result[i] = TRAPPED /
 * ADVANCED / REACHED. */
int gbp_attempt_connect_batch(gbp_terrain *t, int64_t n, const double *s_existing,
                              const double *s, const double *t_s, int direction, int adaptive,
                              int32_t *result, double *s_new, double *a_new);
}
