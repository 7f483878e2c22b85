/*
 * ref_gridmap_shim.cpp -- ORACLE SUPPORT (test infrastructure): C entry points around the REFERENCE's
 * own grid_map_core (GridMap, GridMapMath, SubmapGeometry, BufferRegion, the GridMap / Submap / Line /
 * Circle iterators), move_control's MapUpdater::lineOnMap and RrtPlanner::makePlan, compiled from the
 * sources where they lie (never copied) by oracle/Makefile's `ref` target into oracle/_ref/libref_gridmap.so.
 * Eigen, ROS and tf are stood in for by oracle/ref_shim/include (see Eigen/Core there for what the pin
 * rests on).  This file only calls the reference: it builds a grid_map::GridMap from an og_geom and
 * layers, walks the reference's iterators into index arrays, and runs the reference's own functions.
 *
 * Build-time interventions, both for the harness's sake and neither touching arithmetic:
 *  - -include rna_ref_rand.h (rrt_planner.cpp only) counts the planner's rand() calls and ends a run that
 *    exceeds a budget by throwing, because extendTree's while(true) never ends on a map with no free
 *    cell in reach; every value still comes from this libc's rand().
 *  - coefficient access out of range is counted by the Eigen stand-in (rna_ref_eigen_range_errors);
 *    every entry point returns RNA_REF_RANGE_ERROR when it happened.
 * Used by tests/ and tests/golden/gen_gridmap_ref_recorded.py only.
 */
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "grid_map_core/grid_map_core.hpp"

#include "move_control/map_updater.h"
#define private public /* the tree's size, for the node count */
#include "move_control/rrt_planner.h"
#undef private

#include "../rna_oracle.h"

extern "C" {
int rna_ref_eigen_range_errors = 0;
}

namespace {

const int RNA_REF_RANGE_ERROR = -2;
const int RNA_REF_GEOMETRY_ERROR = -3;

struct SampleBudgetExceeded {};
long g_rand_calls = 0;
long g_rand_budget = 0;

using grid_map::GridMap;
using grid_map::Index;
using grid_map::Length;
using grid_map::Position;
using grid_map::Size;

// a GridMap with the og_geom's geometry (setGeometry, then the circular buffer's start index) and, if given,
// column-major float layers named l0, l1, ...
bool make_map(const og_geom* g, GridMap& map, int n_layers = 0, float* const* layers = nullptr) {
  map.setGeometry(Length(g->len[0], g->len[1]), g->res, Position(g->pos[0], g->pos[1]));
  if (map.getSize()(0) != g->size[0] || map.getSize()(1) != g->size[1] || map.getLength()(0) != g->len[0] ||
      map.getLength()(1) != g->len[1])
    return false;
  map.setStartIndex(Index(g->start[0], g->start[1]));
  for (int k = 0; k < n_layers; ++k) {
    grid_map::Matrix m(g->size[0], g->size[1]);
    std::memcpy(m.data(), layers[k], sizeof(float) * (size_t)m.size());
    map.add("l" + std::to_string(k), m);
  }
  return true;
}

void layers_out(const GridMap& map, int n_layers, float* const* layers) {
  for (int k = 0; k < n_layers; ++k) {
    const grid_map::Matrix& m = map.get("l" + std::to_string(k));
    std::memcpy(layers[k], m.data(), sizeof(float) * (size_t)m.size());
  }
}

void put_geom(const GridMap& map, og_geom* out) {
  out->len[0] = map.getLength()(0);
  out->len[1] = map.getLength()(1);
  out->pos[0] = map.getPosition()(0);
  out->pos[1] = map.getPosition()(1);
  out->res = map.getResolution();
  out->size[0] = map.getSize()(0);
  out->size[1] = map.getSize()(1);
  out->start[0] = map.getStartIndex()(0);
  out->start[1] = map.getStartIndex()(1);
}

template <typename It>
int walk(It& it, int* cells, int cap) {
  int n = 0;
  for (; !it.isPastEnd(); ++it, ++n)
    if (n < cap) {
      cells[2 * n] = (*it)(0);
      cells[2 * n + 1] = (*it)(1);
    }
  return n;
}

// MapUpdater with nothing but the reference's own lineOnMap / markCell / clearCell in use
class RayUpdater : public move_control::MapUpdater {
 public:
  RayUpdater(ros::NodeHandle& nh, tf::TransformListener& tf, GridMap& map)
      : move_control::MapUpdater(nh, tf, map, "l0") {}
  void updateMap(double&, double&, double&, double&) override {}
  void addMonitorTopic(const std::string&) override {}
  void ray(const og_ray& r) {
    RangeSample s;
    s.start = Position(r.sx, r.sy);
    s.end = Position(r.ex, r.ey);
    s.ifClearEnd = r.clear_end != 0;
    lineOnMap(s);
  }
};

}  // namespace

extern "C" int rna_ref_rand() {
  if (++g_rand_calls > g_rand_budget) throw SampleBudgetExceeded();
  return rand();
}

extern "C" {

/* grid_map::getIndexFromPosition / getPositionFromIndex / getSubmapInformation on the og_geom's raw fields
 * (no GridMap, so any length / size pair of the gtests can be given).  Return the reference's bool. */
int refgm_index_from_position(const og_geom* g, const double pos[2], int idx[2]) {
  Index i;
  bool ok = grid_map::getIndexFromPosition(i, Position(pos[0], pos[1]), Length(g->len[0], g->len[1]),
                                           Position(g->pos[0], g->pos[1]), g->res, Size(g->size[0], g->size[1]),
                                           Index(g->start[0], g->start[1]));
  if (ok) { idx[0] = i(0); idx[1] = i(1); }
  return ok;
}

int refgm_position_from_index(const og_geom* g, const int idx[2], double pos[2]) {
  Position p;
  bool ok = grid_map::getPositionFromIndex(p, Index(idx[0], idx[1]), Length(g->len[0], g->len[1]),
                                           Position(g->pos[0], g->pos[1]), g->res, Size(g->size[0], g->size[1]),
                                           Index(g->start[0], g->start[1]));
  if (ok) { pos[0] = p(0); pos[1] = p(1); }
  return ok;
}

int refgm_submap_information(const og_geom* g, const double req_pos[2], const double req_len[2], og_submap_info* o) {
  Index tl, req;
  Size size;
  Position pos;
  Length len;
  bool ok = grid_map::getSubmapInformation(tl, size, pos, len, req, Position(req_pos[0], req_pos[1]),
                                           Length(req_len[0], req_len[1]), Length(g->len[0], g->len[1]),
                                           Position(g->pos[0], g->pos[1]), g->res, Size(g->size[0], g->size[1]),
                                           Index(g->start[0], g->start[1]));
  for (int a = 0; a < 2; ++a) {
    o->top_left[a] = tl(a);
    o->size[a] = size(a);
    o->pos[a] = pos(a);
    o->len[a] = len(a);
    o->requested_index[a] = req(a);
  }
  return ok;
}

/* grid_map::LineIterator(map, start, end) walked in order; (i, j) pairs, returns the number of cells */
int refgm_line_cells(const og_geom* g, const double start[2], const double end[2], int* cells, int cap) {
  rna_ref_eigen_range_errors = 0;
  GridMap map;
  if (!make_map(g, map)) return RNA_REF_GEOMETRY_ERROR;
  // When the line misses the map the constructor initialises nothing (its counters stay indeterminate);
  // built in zeroed storage it is past its end at once, which is what LineIteratorTest expects of that case.
  alignas(grid_map::LineIterator) unsigned char storage[sizeof(grid_map::LineIterator)];
  std::memset(storage, 0, sizeof(storage));
  grid_map::LineIterator* it = new (storage) grid_map::LineIterator(map, Position(start[0], start[1]), Position(end[0], end[1]));
  int n = walk(*it, cells, cap);
  it->~LineIterator();
  return rna_ref_eigen_range_errors ? RNA_REF_RANGE_ERROR : n;
}

/* grid_map::CircleIterator(map, center, radius) */
int refgm_circle_cells(const og_geom* g, const double center[2], double radius, int* cells, int cap) {
  rna_ref_eigen_range_errors = 0;
  GridMap map;
  if (!make_map(g, map)) return RNA_REF_GEOMETRY_ERROR;
  grid_map::CircleIterator it(map, Position(center[0], center[1]), radius);
  int n = walk(it, cells, cap);
  return rna_ref_eigen_range_errors ? RNA_REF_RANGE_ERROR : n;
}

/* grid_map::SubmapIterator(map, tl, size): buffer index then submap index, 4 ints per cell */
int refgm_submap_cells(const og_geom* g, const int tl[2], const int size[2], int* out, int cap) {
  rna_ref_eigen_range_errors = 0;
  GridMap map;
  if (!make_map(g, map)) return RNA_REF_GEOMETRY_ERROR;
  grid_map::SubmapIterator it(map, Index(tl[0], tl[1]), Size(size[0], size[1]));
  int n = 0;
  for (; !it.isPastEnd(); ++it, ++n)
    if (n < cap) {
      out[4 * n] = (*it)(0);
      out[4 * n + 1] = (*it)(1);
      out[4 * n + 2] = it.getSubmapIndex()(0);
      out[4 * n + 3] = it.getSubmapIndex()(1);
    }
  return rna_ref_eigen_range_errors ? RNA_REF_RANGE_ERROR : n;
}

/* GridMap::getSubmap(pos, len, indexInSubmap, isSuccess) of a one-layer map.  Returns isSuccess (0 / 1);
 * sub_geom, the submap's layer (column-major, sub_cap floats at most) and the requested index are written
 * on success. */
int refgm_get_submap(const og_geom* g, float* layer, const double pos[2], const double len[2], og_geom* sub_geom,
                     float* sub_out, int sub_cap, int requested_index[2]) {
  rna_ref_eigen_range_errors = 0;
  GridMap map;
  if (!make_map(g, map, 1, &layer)) return RNA_REF_GEOMETRY_ERROR;
  bool ok = false;
  Index idx;
  GridMap sub = map.getSubmap(Position(pos[0], pos[1]), Length(len[0], len[1]), idx, ok);
  if (rna_ref_eigen_range_errors) return RNA_REF_RANGE_ERROR;
  if (!ok) return 0;
  put_geom(sub, sub_geom);
  const grid_map::Matrix& m = sub.get("l0");
  if (m.size() > sub_cap) return RNA_REF_RANGE_ERROR;
  std::memcpy(sub_out, m.data(), sizeof(float) * (size_t)m.size());
  requested_index[0] = idx(0);
  requested_index[1] = idx(1);
  return 1;
}

/* GridMap::move(pos, newRegions) on n_layers column-major layers (modified in place); g is updated to the
 * moved geometry.  Returns the number of new regions (cap 4, quadrant codes as og_region), *moved = the result. */
int refgm_move(og_geom* g, float** layers, int n_layers, const double new_pos[2], og_region* regions, int* moved) {
  rna_ref_eigen_range_errors = 0;
  GridMap map;
  if (!make_map(g, map, n_layers, layers)) return RNA_REF_GEOMETRY_ERROR;
  std::vector<grid_map::BufferRegion> nr;
  *moved = map.move(Position(new_pos[0], new_pos[1]), nr) ? 1 : 0;
  if (rna_ref_eigen_range_errors || nr.size() > 4) return RNA_REF_RANGE_ERROR;
  for (size_t k = 0; k < nr.size(); ++k) {
    regions[k].index[0] = nr[k].getStartIndex()(0);
    regions[k].index[1] = nr[k].getStartIndex()(1);
    regions[k].size[0] = nr[k].getSize()(0);
    regions[k].size[1] = nr[k].getSize()(1);
    regions[k].quadrant = (int)nr[k].getQuadrant();
  }
  layers_out(map, n_layers, layers);
  put_geom(map, g);
  return (int)nr.size();
}

/* MapUpdater::lineOnMap for each ray in order, on one column-major layer (modified in place) */
int refgm_himm_update(const og_geom* g, float* layer, const og_ray* rays, int n) {
  rna_ref_eigen_range_errors = 0;
  GridMap map;
  if (!make_map(g, map, 1, &layer)) return RNA_REF_GEOMETRY_ERROR;
  ros::NodeHandle nh;
  tf::TransformListener tf;
  RayUpdater up(nh, tf, map);
  for (int r = 0; r < n; ++r) up.ray(rays[r]);
  if (rna_ref_eigen_range_errors) return RNA_REF_RANGE_ERROR;
  layers_out(map, 1, &layer);
  return 0;
}

/* srand(seed); RrtPlanner(map, start, target, close_tol).makePlan(path) on a map whose "master" layer is
 * `master`.  res: status 1 / 0 = makePlan's result, -1 = more than max_rand rand() calls (the reference would
 * not stop); path_len (goal -> start), tree_size; samples is not observable in the reference and set to -1. */
int refgm_rrt_plan(const og_geom* g, const float* master, const double start[2], const double target[2],
                   double close_tol, unsigned seed, long max_rand, double* path_xy, int path_cap, og_rrt_result* res) {
  rna_ref_eigen_range_errors = 0;
  GridMap map;
  if (!make_map(g, map)) return RNA_REF_GEOMETRY_ERROR;
  grid_map::Matrix m(g->size[0], g->size[1]);
  std::memcpy(m.data(), master, sizeof(float) * (size_t)m.size());
  map.add("master", m);
  Position s(start[0], start[1]), t(target[0], target[1]);
  move_control::RrtPlanner planner(map, s, t, close_tol);
  std::vector<Position> path;
  g_rand_calls = 0;
  g_rand_budget = max_rand;
  srand(seed);
  res->samples = -1;
  try {
    res->status = planner.makePlan(path) ? 1 : 0;
  } catch (const SampleBudgetExceeded&) {
    res->status = -1;
    res->path_len = 0;
    res->tree_size = (int)planner.rrtTree_.size();
    return rna_ref_eigen_range_errors ? RNA_REF_RANGE_ERROR : 0;
  }
  res->tree_size = (int)planner.rrtTree_.size();
  res->path_len = (int)path.size();
  for (size_t k = 0; k < path.size() && (int)k < path_cap; ++k) {
    path_xy[2 * k] = path[k](0);
    path_xy[2 * k + 1] = path[k](1);
  }
  return rna_ref_eigen_range_errors ? RNA_REF_RANGE_ERROR : 0;
}

}  // extern "C"
