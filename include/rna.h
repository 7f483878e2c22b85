/*
 * rna.h -- C ABI of the MI355X-native occupancy-grid planning engine (librna.so).
 *
 * The reference (jmloveyj/ros_navigation) has no FFI layer: its replan hot path sits behind plain
 * C++ class methods called by the node mains.  Every entry point below replaces one of those call
 * sites; the C++ mirror classes in ros_navigation_amd/host/ (same names and argument meaning as
 * the reference) and the ctypes binding in ros_navigation_amd/capi.py are thin shims over it.
 * Citations: mc/ = move_control/, gmc/ = grid_map-master/grid_map_core/ in the reference tree.
 *
 * Conventions: every call returns 0 (RNA_OK) or a negative rna_status; no exceptions cross the
 * boundary; buffers are caller-owned; calls on one engine are serialised by the caller (one HIP
 * stream per engine).  Grids are column-major float32, linear index = i + j*rows, exactly the
 * Eigen::MatrixXf storage of grid_map::GridMap (gmc/include/grid_map_core/TypeDefs.hpp:16).
 * "_device" variants take device pointers (inputs/outputs already resident in HBM) and are
 * asynchronous on the engine's stream; the plain variants take host pointers and return after the
 * results are back in host memory.
 */
#ifndef RNA_H
#define RNA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: rna_laser_scan carries the end pose (80 bytes), rna_astar_result.expanded / .rounds changed meaning (cells written,
 *    tile jobs per wavefront), statuses 4 / 5, profile slot astar_reset, default bucket width 96000.  A host checks
 *    rna_abi_version() == RNA_ABI_VERSION after loading the library (capi.py and move_control_amd.hpp do). */
/* 3: rna_synchronize_map, rna_hw_queue_advice (round 4); no existing signature changed.
 * 4: rna_scan_to_rays_tf[_device], rna_range_to_rays_tf (sensors with a full tf transform; round 4); no existing signature changed.
 * 5: rna_astar_job_counters (round 6); the default bucket width of the grid search is 128000, a pipeline may have up to 20 stages,
 *    rna_astar_result.rounds counts every job again (also the ones that find nothing); no existing signature changed. */
/* 6: robot radius of the grid A* (rna_astar_set_robot_radius / _get_robot_radius, rna_astar_download_blocked),
 *    rna_if_blocked_batch[_device], profile slot footprint; no existing signature changed.
 * 6, later: goal field entry points added (rna_goal_field_*, rna_goal_field_info), nothing changed -- no signature, no layout,
 *    no profile slot --, so the version stays 6.
 * 6, later still: clearance field and clearance cost (rna_clearance_*, rna_goal_field_set / _get_clearance_cost) added in the
 *    same way.  Likewise the shortcut, the frontiers, the view gain and scan matching (rna_scan_match*). */
#define RNA_ABI_VERSION 6

typedef enum {
  RNA_OK = 0,
  RNA_EINVAL = -1,     /* bad argument */
  RNA_ENOMEM = -2,     /* device/host allocation failed */
  RNA_EHIP = -3,       /* HIP runtime error (rna_last_error has the text) */
  RNA_ECAPACITY = -4,  /* a device work queue overflowed; retry with a larger capacity */
  RNA_ESTATE = -5,     /* call order (e.g. vfh step before vfh init) */
  RNA_ENODEVICE = -6   /* no usable gfx950 device */
} rna_status;

typedef struct rna_engine rna_engine;

/* grid_map::GridMap geometry (gmc/include/grid_map_core/GridMap.hpp:493-516) */
typedef struct {
  double length[2];      /* length_   */
  double position[2];    /* position_ */
  double resolution;     /* resolution_ */
  int32_t size[2];       /* size_: rows = Index(0), cols = Index(1) */
  int32_t start_index[2];/* startIndex_ (circular buffer) */
} rna_geometry;

/* layers of MapProvider's GridMap (mc/src/map_provider.cpp:17-19, map_updater.h:12-13) */
typedef enum { RNA_LAYER_MASTER = 0, RNA_LAYER_LASER = 1, RNA_LAYER_RANGE = 2, RNA_NUM_LAYERS = 3 } rna_layer;

/* ---- engine / GridMap container -------------------------------------------------------------- */
/* GridMap::GridMap + setGeometry (gmc/src/GridMap.cpp:27-70): size = round(length/res), all layers
 * NaN.  MapProvider::initMap (mc/src/map_provider.cpp:145-149). */
int rna_create(rna_engine** out, double length_x, double length_y, double resolution,
               double position_x, double position_y, int device_id);
void rna_destroy(rna_engine* e);
const char* rna_last_error(const rna_engine* e);
int rna_abi_version(void);
int rna_get_geometry(const rna_engine* e, rna_geometry* out);
/* GridMap::operator[] / get (gmc/src/GridMap.cpp:125-151): whole-layer copies to/from the host */
int rna_layer_upload(rna_engine* e, int layer, const float* host, size_t n_cells);
int rna_layer_download(rna_engine* e, int layer, float* host, size_t n_cells);
int rna_layer_fill(rna_engine* e, int layer, float value);
/* device pointer of a layer (rows*cols float32, column-major) for zero-copy producers/consumers */
void* rna_layer_device_ptr(rna_engine* e, int layer);
/* hipStream_t of the engine's MAP stream: map updates, compose, pack / unpack, uploads and the host-pointer calls run
 * on it.  It is not the only stream: with a pipeline depth > 1 the A* searches run on the stages' own streams and
 * rna_vfh_step_batch_device on an internal side stream, so work a caller chains on rna_stream() is ordered with the
 * map, NOT with the outputs of those two calls -- they are valid after rna_synchronize() (or, for VFH+, after
 * rna_synchronize_map()). */
void* rna_stream(rna_engine* e);
/* everything the engine has in flight: the map stream, the VFH+ side stream, every A* pipeline stage, and the second
 * passes over searches that ran out of pages (issued here if they are still due) */
int rna_synchronize(rna_engine* e);
/* the map stream and the VFH+ side stream only: searches in flight keep running (a tiled host's per-pass exchange,
 * a consumer of the VFH+ commands).  Does not make A* outputs valid. */
int rna_synchronize_map(rna_engine* e);
/* GridMap::getIndex / getPosition / isInside (gmc/src/GridMap.cpp:227-240) -- host-side math */
int rna_get_index(const rna_engine* e, double x, double y, int32_t index[2]);   /* 1 inside, 0 outside */
int rna_get_position(const rna_engine* e, int32_t i, int32_t j, double position[2]);

/* The same math over a geometry alone -- no engine, no GPU (host iterators of the C++ mirror, callers that only
 * need indices).  1 inside / in range, 0 outside, < 0 = rna_status. */
int rna_geometry_index(const rna_geometry* g, double x, double y, int32_t index[2]);
int rna_geometry_position(const rna_geometry* g, int32_t i, int32_t j, double position[2]);
/* grid_map_core's iterators as cell lists ((i, j) buffer-index pairs in visiting order; return value = length of
 * the walk, only the first cap cells are written): LineIterator (gmc/src/iterators/LineIterator.cpp:16-150; the
 * cells a HIMM ray clears), CircleIterator (CircleIterator.cpp:16-93; the blocked-disc scan of GlobalPlanner::
 * ifBlocked), SubmapIterator (SubmapIterator.cpp:28-83). */
int rna_line_cells(const rna_geometry* g, double sx, double sy, double ex, double ey, int32_t* cells, int cap);
int rna_circle_cells(const rna_geometry* g, double cx, double cy, double radius, int32_t* cells, int cap);
int rna_submap_cells(const rna_geometry* g, const int32_t top_left[2], const int32_t size[2], int32_t* cells, int cap);
/* GridMap copy-assignment (`map = map_`, MapProvider::getMap, mc/src/map_provider.cpp:120-125): a new engine with
 * the same geometry, start index and layer contents; the caller destroys it. */
int rna_clone(rna_engine* src, rna_engine** out);

/* ---- HIMM map update ------------------------------------------------------------------------- */
/* RangeSample (mc/include/move_control/map_updater.h:28-32) */
typedef struct {
  double sx, sy;        /* start */
  double ex, ey;        /* end   */
  int32_t clear_end;    /* ifClearEnd */
  int32_t _pad;
} rna_ray;
/* LaserMapUpdater::updateMap / RangeMapUpdater::updateMap -> MapUpdater::lineOnMap for every
 * sample in order (mc/src/laser_map_updater.cpp:7-21, map_updater.h:38-71): order-faithful result. */
int rna_himm_update(rna_engine* e, int layer, const rna_ray* rays_host, int n);
int rna_himm_update_device(rna_engine* e, int layer, const rna_ray* rays_device, int n);
/* MapProvider::composeMasterMapFromLayerdMap (mc/src/map_provider.cpp:216-223): master = laser.
 * mode 0: only the 64x64 tiles the HIMM batches touched since the last compose (fused path);
 * mode 1: whole-layer copy exactly as the reference does every cycle. */
int rna_compose_master(rna_engine* e, int mode);
/* MapProvider::updateMap (mc/src/map_provider.cpp:190-205): laser HIMM batch, then compose(mode) */
int rna_update_map(rna_engine* e, const rna_ray* rays_host, int n, int compose_mode);
int rna_update_map_device(rna_engine* e, const rna_ray* rays_device, int n, int compose_mode);
/* Tiled single map (SURVEY.md 8e mode 2, BASELINE config 5): every GPU holds a full-size layer but
 * owns one window of it.  rna_himm_set_window restricts every later HIMM batch to the cells
 * [i0, i0+ni) x [j0, j0+nj) (buffer indices): lines are still clipped and walked on the whole map's
 * geometry (LineIterator.cpp:60-150), so inside the window the result is bit-identical to the
 * untiled update.  ni <= 0 or nj <= 0 restores the whole map. */
int rna_himm_set_window(rna_engine* e, int i0, int j0, int ni, int nj);
/* Rectangular block of a layer <-> dense column-major device buffer (ni*nj floats, i fastest):
 * halo strips and owner tiles exchanged between GPUs.  Both return after the copy has finished. */
int rna_layer_pack_region(rna_engine* e, int layer, int i0, int ni, int j0, int nj, float* dense_device);
int rna_layer_unpack_region(rna_engine* e, int layer, int i0, int ni, int j0, int nj, const float* dense_device);
/* Incremental hand-over of the tiled mode.  rna_last_dirty_tiles: one byte per 64 x 64 tile (index tj*tiles_i + ti,
 * tiles_i = ceil(rows/64)) = the tiles the last rna_compose_master consumed, i.e. what the last HIMM batch changed on
 * this GPU.  rna_layer_pack_tiles / rna_layers_unpack_tiles move the listed tiles, clipped to the window
 * [i0,i0+ni) x [j0,j0+nj), through a dense device buffer of n slots of 4096 floats; unpack writes layer_a and (if
 * >= 0) layer_b and flags the tiles for the next rna_compose_master(e, 0), which refreshes their A* neighbour masks
 * (+ring) instead of rebuilding all of them.  rna_layer_unpack_region_tracked is rna_layer_unpack_region with the
 * same per-tile bookkeeping.  Precondition of the tracked calls: the laser layer is complete on this GPU (every
 * owner's changes have been unpacked into laser AND master), so that composing a flagged tile is harmless. */
int rna_last_dirty_tiles(rna_engine* e, uint8_t* flags_host, size_t n_tiles);
int rna_layer_pack_tiles(rna_engine* e, int layer, const int32_t* tiles_host, int n, int i0, int ni, int j0, int nj,
                         float* dense_device);
int rna_layers_unpack_tiles(rna_engine* e, int layer_a, int layer_b, const int32_t* tiles_host, int n, int i0, int ni,
                            int j0, int nj, const float* dense_device);
int rna_layer_unpack_region_tracked(rna_engine* e, int layer, int i0, int ni, int j0, int nj, const float* dense_device);
/* The same with the tile lists resident on the device (a C/C++ host that drives RCCL itself, include/rna_rccl.h):
 * rna_last_dirty_tiles_device compacts the flagged tiles that intersect the window into list_device (room for every
 * tile of the map) and their number into *count_device; the pack / unpack forms take device lists.  Asynchronous on
 * the engine's stream. */
int rna_last_dirty_tiles_device(rna_engine* e, int i0, int ni, int j0, int nj, int32_t* list_device, int* count_device);
int rna_layer_pack_tiles_device(rna_engine* e, int layer, const int32_t* tiles_device, int n, int i0, int ni, int j0, int nj,
                                float* dense_device);
int rna_layers_unpack_tiles_device(rna_engine* e, int layer_a, int layer_b, const int32_t* tiles_device, int n, int i0, int ni,
                                   int j0, int nj, const float* dense_device);
/* GridMap::move (gmc/src/GridMap.cpp:346-412): recentre the circular buffer, dropped cells -> NaN */
int rna_move(rna_engine* e, double position_x, double position_y, int* moved);

/* MapProvider::getSubMap -> GridMap::getSubmap (mc/src/map_provider.cpp:93-100, gmc/src/GridMap.cpp:287-339,
 * getSubmapInformation gmc/src/GridMapMath.cpp:246-296): the requested window is clamped to the map, and the
 * submap's cells are gathered across the circular-buffer seam (the reference's <= 4 quadrant block copies) into
 * out (column-major, info->size[0]*info->size[1] floats, startIndex (0,0)).  Callers: Steerer (1.5 m window,
 * mc/src/steerer.cpp:158; fused into rna_vfh_step_batch here) and Nav::makePlan's planning window
 * (mc/src/nav_node.cpp:141).  Returns 1 = success, 0 = the reference's isSuccess == false, < 0 = rna_status
 * (RNA_ECAPACITY when the submap has more than cap_cells cells; info is filled in that case too). */
typedef struct {
  double length[2];      /* submap length_ (size * resolution) */
  double position[2];    /* submap position_ (centre) */
  int32_t size[2];
  int32_t top_left[2];   /* buffer index of the submap's first cell in the parent map */
} rna_submap_info;
int rna_get_submap(rna_engine* e, int layer, double position_x, double position_y, double length_x, double length_y,
                   float* out_host, size_t cap_cells, rna_submap_info* info);
int rna_get_submap_device(rna_engine* e, int layer, double position_x, double position_y, double length_x,
                          double length_y, float* out_device, size_t cap_cells, rna_submap_info* info);
/* The same as a GridMap of its own, which is what GridMap::getSubmap returns: a NEW engine (same device) with the
 * submap's geometry and all three layers, ready for rna_rrt_batch / rna_astar_batch on the planning window -- the
 * flow of Nav::makePlan (mc/src/nav_node.cpp:136-152: getSubMap, then RrtPlanner on the submap).  Returns 1 and the
 * engine in *out (caller destroys it), 0 when the reference's isSuccess is false, < 0 = rna_status. */
int rna_create_submap(rna_engine* parent, double position_x, double position_y, double length_x, double length_y,
                      rna_engine** out);

/* ---- VFH+ local avoidance -------------------------------------------------------------------- */
/* VFH constructor arguments + SetRobotRadius (mc/include/move_control/vfh.h:185-203,235;
 * defaults of Steerer::initVfh, mc/src/steerer.cpp:69-121) */
typedef struct {
  double cell_size;
  int32_t window_diameter;
  int32_t sector_angle;
  double safety_dist_0ms, safety_dist_1ms;
  int32_t max_speed, max_speed_narrow_opening, max_speed_wide_opening;
  int32_t max_acceleration, min_turnrate, max_turnrate_0ms, max_turnrate_1ms;
  double min_turn_radius_safety_factor;
  double free_space_cutoff_0ms, obs_cutoff_0ms, free_space_cutoff_1ms, obs_cutoff_1ms;
  double weight_desired_dir, weight_current_dir;
  double robot_radius;
} rna_vfh_params;
void rna_vfh_default_params(rna_vfh_params* p);
/* One robot pose + the per-step arguments of VFH::Update_VFH (mc/include/move_control/vfh.h:216-222)
 * as Steerer::update derives them (mc/src/steerer.cpp:221-263); dt replaces gettimeofday(). */
typedef struct {
  double x, y, yaw;            /* MapProvider::getRobotPos(pos, orient) */
  double dt;                   /* seconds since this robot's previous step */
  int32_t current_speed;       /* mm/s */
  float goal_direction;        /* deg, 90 = straight ahead */
  float goal_distance;         /* mm */
  float goal_tolerance;        /* mm */
} rna_pose;
typedef struct {
  int32_t chosen_speed;        /* mm/s  */
  int32_t chosen_turnrate;     /* deg/s */
  float picked_angle;          /* VFH::GetPickedAngle() */
  int32_t emergency;           /* 1 when something was inside the safety distance */
} rna_vfh_out;
/* VFH::VFH + SetRobotRadius + Init (mc/src/vfh.cpp:53-110,237-416) for `n_robots` independent,
 * stateful VFH instances (Last_Binary_Hist, Last_Picked_Angle, last_chosen_speed, ...).
 * Accepted: window_diameter 2..64, even or odd; sector_angle 3..360 with rint(360 / sector_angle) == 360 / sector_angle in
 * integers (3, 4, 5, 6, 7, 8, 9, 10, 12, 15, 16, ... but not 11, 13, 14, 100 or 200), which keeps the histogram between 1
 * and 128 sectors, and not 144..179 (two sectors that do not close the circle: the reference's valley borders wrap at 360
 * there, in a sector that can open); max_speed 1..100000. Anything else is refused with RNA_EINVAL and the instances of the last
 * successful call stay as they are.  Two inputs the reference leaves undefined are defined: the centre cell of an odd
 * window, for which vfh.cpp:1018 reads laser_ranges[-2], is never occupied; a current speed above max_speed, which
 * indexes Min_Turning_Radius past its end, takes the per-speed quantities of the masked histogram at max_speed. */
int rna_vfh_init(rna_engine* e, const rna_vfh_params* p, int n_robots);
int rna_vfh_reset(rna_engine* e);          /* re-Init every instance's state */
int rna_vfh_hist_size(const rna_engine* e);
/* Steerer::getRangesFromSubmap + VFH::Update_VFH for robots [0, n) (mc/src/steerer.cpp:147-191,
 * 260-263; mc/src/vfh.cpp:480-605).  origin_hist / hist: n x hist_size float32 (may be NULL):
 * VFH::OriginHist and VFH::Hist after the step. */
int rna_vfh_step_batch(rna_engine* e, const rna_pose* poses_host, int n, rna_vfh_out* out_host,
                       float* origin_hist_host, float* hist_host);
/* (_device: with a pipeline depth > 1 the step runs on an internal side stream behind the map stream -- its outputs are
 * valid after rna_synchronize_map() / rna_synchronize(), not for work merely enqueued on rna_stream() after the call) */
int rna_vfh_step_batch_device(rna_engine* e, const rna_pose* poses_device, int n, rna_vfh_out* out_device,
                              float* origin_hist_device, float* hist_device);
/* VFH::Update_VFH fed with caller-provided range scans (double[361][2] per robot, as the reference
 * signature) instead of the map -- the drop-in for code that owns its own scan (cd/src/vfh_node.cpp). */
int rna_vfh_update_batch(rna_engine* e, const double* ranges_host /* n*361*2 */, const rna_pose* poses_host,
                         int n, rna_vfh_out* out_host, float* origin_hist_host, float* hist_host);

/* ---- global planning: grid A* ------------------------------------------------------------------ */
/* The reference's AStarPlanner::makePlan (mc/src/astar_planner.cpp:63-96) searches a 9-vertex
 * waypoint graph; BASELINE.json asks for a grid A* over the GridMap, whose contract is defined in
 * DESIGN.md ("Grid A* contract") and restated by oracle/astar.c.  Cells are buffer linear indices
 * (i + j*rows, what GridMap::getIndex hands out); on a map that GridMap::move has recentred the
 * search runs in map space (unwrapped indices) and paths cross the circular-buffer seam. */
typedef struct { int32_t start, goal; } rna_astar_query;
typedef struct {
  int32_t status;      /* 0 found, 1 no path, 2 invalid query, 3 path longer than max_path_len,
                          4 path cost beyond the field's 30-bit g range (>= 1.07e9), 5 TRANSIENT: the query's share of search
                          pages was used up (pages are only limited after rna_astar_set_page_cap or when HBM is short) and it
                          waits for its second pass on a full-size retry slot -- visible only in a device result buffer read
                          before rna_synchronize(); never final (a goal that cannot be reached floods its component, is
                          searched again and answers 1) */
  int32_t path_len;    /* cells, start..goal inclusive */
  int32_t cost;        /* 1000/1414 integer cost of the path */
  int32_t expanded;    /* cells the device wrote (64 per row of a tile a job changed; >= the oracle's settled count) */
  int32_t rounds;      /* tile jobs per wavefront of the query's workgroup: every job, also the ones that find nothing better in their
                          halo, and every sticky turn (rounds 1-2: barrier-separated rounds of jobs) */
  int32_t buckets;     /* f-buckets visited */
} rna_astar_result;
/* max_queries: queries searched concurrently (one g-field each; larger batches are processed in
 * chunks); queue_capacity: ignored (the cell queues of the frontier kernel removed in round 3; the tile kernel's open
 * list has a fixed size in LDS and parks what does not fit); bucket_width: the f-range (cost units, >= 2828) inside
 * which free wavefronts take tiles by key before the search advances (default 128000; 96000 until round 5); 0 = keep/default.
 * Maps of more than 65 536 tiles of 64 x 16 cells (8192 x 8192 cells) are refused with RNA_EINVAL. */
int rna_astar_configure(rna_engine* e, int max_queries, int queue_capacity, int bucket_width);
/* Pipelined batches: with depth d > 1 consecutive rna_astar_batch_device calls run their searches on d
 * rotating internal streams (each with its own search fields), so the tail of one batch overlaps
 * the next batch and the next map update.  Outputs of a call are valid after rna_synchronize() -- not after a
 * bare hipDeviceSynchronize(): searches that ran out of their share of pages are searched again by a second launch
 * the host issues when it sees their count, at the latest inside rna_synchronize().  The call returns after
 * enqueueing; while every stage is busy it blocks until one is free.  The caller must give calls that may be in
 * flight together distinct output buffers.  Default 4; up to 20 (16 until round 5).
 * Hardware queues: every stage's stream wants a hardware queue of its own, and the HIP runtime multiplexes all of a
 * process's streams over GPU_MAX_HW_QUEUES (default 4) of them, read from the environment at its first call.  librna.so
 * sets GPU_MAX_HW_QUEUES=8 when it is loaded and the variable is unset (RNA_KEEP_HW_QUEUES=1 turns that off); when the
 * value in force is too small for `depth` the call still succeeds -- searches then share queues and overlap less --
 * and rna_last_error() holds the one-line advice of rna_hw_queue_advice(). */
int rna_astar_set_pipeline_depth(rna_engine* e, int depth);
/* Host-only (no engine, no GPU): 0 and an empty string when GPU_MAX_HW_QUEUES -- the value librna.so found (or set) WHEN IT
 * WAS LOADED, which is what the HIP runtime latches at its first call; later changes of the environment do not count --
 * leaves the stages of `pipeline_depth` a hardware queue each (depth <= 2, or >= 8 queues); 1 and one line of advice in
 * buf when it is too small; 2 and one line when the library set the variable itself but the process had already opened
 * the GPU by then (the setting probably came too late: export it before the first HIP call, e.g. before importing torch). */
int rna_hw_queue_advice(int pipeline_depth, char* buf, size_t cap);
/* The tile kernel keeps a search's distance field in 4 KiB pages (64 x 16 cells) handed out on first touch.  By
 * default every query may take one page per tile of the map (it can never run out; HBM is only touched where a
 * search goes; half a map's worth when the pipeline stages would not fit HBM otherwise).  A smaller share per query makes room for more queries / pipeline stages in flight; a search that
 * needs more is searched again on one of 8 full-size retry slots per stage (eight at a time, as many passes as it
 * takes): status 5 does not reach the caller.  0 = default. */
int rna_astar_set_page_cap(rna_engine* e, int pages_per_query);
/* What the first batch (or rna_astar_configure after a map is loaded) actually allocated: pipeline stages, pages per
 * query and concurrent queries may have been reduced to fit 75 % of the free HBM.  Any pointer may be NULL; all three
 * are 0 before the allocation. */
int rna_astar_effective_config(const rna_engine* e, int* pipeline_depth, int* pages_per_query, int* max_queries);
int rna_astar_batch(rna_engine* e, const rna_astar_query* queries_host, int n, int32_t* paths_host,
                    int max_path_len, rna_astar_result* results_host);
int rna_astar_batch_device(rna_engine* e, const rna_astar_query* queries_device, int n, int32_t* paths_device,
                           int max_path_len, rna_astar_result* results_device);
/* E of DESIGN.md's roofline: for each query of the LAST batch (n <= max_queries, i.e. one chunk) the
 * number of cells with g + h <= f*, counted from the g fields still resident in HBM.  Equals the CPU
 * oracle's settled count; measurement/test utility, not part of the timed path.  -1 for a query whose field is gone
 * (it outgrew its share of pages and was searched again in a second pass whose retry slot has been reused since). */
int rna_astar_settled_counts(rna_engine* e, int32_t* counts_host, int n);
/* What the grid-A* search kernels counted since the engine's search state was allocated (or since the last call with
 * reset != 0), summed over all searches of all batches; waits for the batches in flight.  counters_host[8]:
 *   [0] searches, [1] tiles that got a page (a search's "touched tiles"), [2] tile jobs -- every job, sticky turns included --,
 *   [3] of them jobs that found nothing better in their halo and left before the sweeps, [4] sticky turns (a wavefront kept a
 *   tile that was woken while its job ran), [5] rows of 64 cells written, [6] f-buckets, [7] buckets that were run again because the open list ran out of nodes.
 * Measurement utility (bench.py's roofline.work_inflation: jobs per touched tile and the no-op share, observed in the timed
 * run itself); the kernel's cost is seven atomic adds per SEARCH.  No reference counterpart (the reference has no grid search:
 * move_control/src/astar_planner.cpp:63-96 is the waypoint graph). */
int rna_astar_job_counters(rna_engine* e, uint64_t* counters_host, int reset);
/* per-cell traversable-neighbour mask derived from the master layer (rows*cols uint8) */
int rna_astar_download_nbr_mask(rna_engine* e, uint8_t* host, size_t n_cells);
/* Robot radius r (metres) of the grid A*: the footprint GlobalPlanner::ifBlocked checks with its 0.3 m disc
 * (mc/include/move_control/map_global_planner.h:39-54, "the radius should be configured from ROS::Parameter footPrint").
 * r == 0 (the default): a cell is blocked iff its own master value is finite and > 0, as before.  r > 0: a cell c is
 * blocked iff ifBlocked(getPosition(c)) with radius r is true -- some cell that CircleIterator(map, centre of c, r)
 * visits (gmc/src/iterators/CircleIterator.cpp:16-93) holds a finite master value > 0; NaN does not block, cells
 * outside the map are not visited.  The neighbour masks, costs and statuses follow from that blocked set by the rules
 * of DESIGN.md's grid A* contract; a start or goal in the inflated region answers as a blocked one.  Valid:
 * 0 <= r and r / resolution <= 63, anything else is RNA_EINVAL.  Batches already issued keep the masks they were
 * issued with; the next batch (or rna_astar_download_nbr_mask) sees the new radius.  rna_clone and rna_create_submap
 * copy it.  The blocked set is a function of the master layer AND of the geometry, start index included: where the box
 * of a disc ends exactly on the map's far edge (radii of k + 1/2 cells) the iterator's corner index equals the size, which
 * the reference wraps to 0 on a moved buffer and leaves out of range on an unmoved one, so the same map in map order
 * can block a few cells of the rows next to that edge on a moved buffer that it leaves free on an unmoved one.  Both
 * answers are the reference's, and the engine gives the one of its own start index. */
int rna_astar_set_robot_radius(rna_engine* e, double radius);
int rna_astar_get_robot_radius(const rna_engine* e, double* radius);
/* the blocked set the search uses (rows*cols uint8 in buffer order, 1 = blocked), refreshed first as
 * rna_astar_download_nbr_mask is: with r == 0 the master layer's finite-and-> 0 cells */
int rna_astar_download_blocked(rna_engine* e, uint8_t* host, size_t n_cells);
/* GlobalPlanner::ifBlocked (map_global_planner.h:39-54, CircleIterator.cpp:16-93) at n arbitrary positions (xy: n x 2
 * doubles) with a chosen radius (finite, >= 0; the reference's is 0.3) on the master layer: out[k] = 1 blocked, 0 free.
 * A check of a tailored or followed plan (mc/src/nav_node.cpp:192-204) or of poses from a caller's own sampler.
 * Corners of the disc's bounding box within rounding of the map's far edge are handled as oracle/gridmath.c
 * og_circle_cells and oracle/rrt.c og_if_blocked define them.  The _device form is asynchronous on the engine stream. */
int rna_if_blocked_batch(rna_engine* e, const double* xy_host, int n, double radius, uint8_t* out_host);
int rna_if_blocked_batch_device(rna_engine* e, const double* xy_device, int n, double radius, uint8_t* out_device);

/* ---- global planning: goal distance field (one sweep serves every start) ------------------------ */
/* What navfn / global_planner offer: ONE wavefront expansion from the goal gives the cost-to-goal of every cell, and a plan
 * from any start is a walk downhill -- for a goal that stays put while robots move (Nav::loopPlan replans to the same goal,
 * mc/src/nav_node.cpp:103-154) or is shared by a fleet.  Same contract as the batch search (DESIGN.md "Grid A* contract",
 * oracle/astar.c): the engine's current neighbour masks (what rna_astar_download_nbr_mask returns: robot radius included,
 * map space on a moved map), costs 1000 / 1414.
 *   field[c]  least cost of a path between cell c and the goal, int32, indexed by BUFFER linear index; field[goal] = 0;
 *             RNA_GOAL_FIELD_UNREACHED for blocked cells and cells of other components; cells whose distance is at or
 *             beyond the search's 30-bit limit (>= 2^30, status 4) read RNA_GOAL_FIELD_FAR; every distance below it is exact.
 *   next[c]   the canonical step from c towards the goal: neighbour number 0-7 in the contract's fixed order
 *             (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1) (map space) -- the first neighbour n that c's mask allows
 *             with field[n] + w == field[c] --, 8 = c is the goal, 254 = far, 255 = unreached.  The flow field a fleet steers by.
 *   paths     from start s: s, next(s), ..., goal.  Cell for cell the REVERSE of what the batch search answers for the query
 *             (start = goal, goal = s), cost = field[s].  rna_astar_result: status 0 found (s == goal: path_len 1, cost 0),
 *             1 field[s] unreached (blocked start, other component, blocked goal), 2 s out of range, 3 path longer than
 *             max_path_len (path_len = true length), 4 far; expanded = rounds = buckets = 0.
 * A field is a SNAPSHOT: map updates, rna_move or a new robot radius after the build change neither the field nor the paths
 * drawn from it; info.stale turns 1 once a call that can change the masks has run (any HIMM batch, compose, upload, fill,
 * unpack, rna_layer_device_ptr, move or radius call -- conservative: also a call that changes nothing, such as rna_move to
 * the current position, the radius it already has, HIMM on the range layer; stale is never 0 after a change and may be 1
 * after none), and the next rna_goal_field_build refreshes it.
 * Memory (5 B per cell) is allocated at the first build; rna_clone / rna_create_submap do not copy a field. */
#define RNA_GOAL_FIELD_UNREACHED 0x7fffffff
#define RNA_GOAL_FIELD_FAR       0x7ffffffe
typedef struct {
  int32_t goal;        /* buffer linear index the field is rooted at; -1 = no field built yet */
  int32_t status;      /* 0 built, 2 the goal cell is blocked (every cell unreached) */
  int32_t reached;     /* cells with a finite distance (the goal included) */
  int32_t max_cost;    /* largest finite distance */
  int32_t rounds;      /* relaxation rounds launched */
  int32_t tile_jobs;   /* tile relaxations run (work inflation = tile_jobs / tiles_reached) */
  int32_t tiles_reached;   /* 64 x 64 map-space tiles holding a reached cell */
  int32_t stale;       /* 1 = something that can change the masks ran since the build */
} rna_goal_field_info;
/* Builds the field of `goal` on the map stream and returns when it is complete (RNA_ECAPACITY: the relaxation exceeded its
 * proven round bound or 30 s -- a defect, reported instead of a hang).  Batches in flight on the pipeline stages are not disturbed. */
int rna_goal_field_build(rna_engine* e, int32_t goal, rna_goal_field_info* info_host /* may be NULL */);
int rna_goal_field_info_get(const rna_engine* e, rna_goal_field_info* out);   /* RNA_OK also before a build (goal -1) */
/* either pointer may be NULL (not both); RNA_ESTATE before a build */
int rna_goal_field_download(rna_engine* e, int32_t* field_host, uint8_t* next_host, size_t n_cells);
void* rna_goal_field_device_ptr(rna_engine* e);   /* int32 per cell, buffer order; NULL before a build */
/* paths: n x max_path_len cells (row k: the path of starts[k], start first); the _device form is asynchronous on rna_stream() */
int rna_goal_field_paths(rna_engine* e, const int32_t* starts_host, int n, int32_t* paths_host, int max_path_len,
                         rna_astar_result* results_host);
int rna_goal_field_paths_device(rna_engine* e, const int32_t* starts_device, int n, int32_t* paths_device, int max_path_len,
                                rna_astar_result* results_device);

/* ---- global planning: goal distance field with many sources, start costs and owner labels -------- */
/* The field above with more than one seed: every robot drives to the cheapest of K docks or frontier cells (one build for the
 * fleet), or -- the sources being the robots -- every cell learns which robot reaches it first and at what cost: the
 * travel-cost Voronoi partition of the map.  A start cost per source is that robot's head start against it (the 12 s of work
 * it still has).  Integers only: every output has exactly one right value.
 *   sources   cells goals[0 .. n), buffer linear indices, and start costs seed[0 .. n), int32, 0 <= seed[k] < 2^30; a NULL
 *             seed means all 0.  1 <= n <= cells; duplicates are allowed.  A source whose cell is in the search's blocked set
 *             (what rna_astar_download_blocked returns: robot radius included, masks refreshed first) is skipped and counted.
 *   field     the least fixpoint of
 *                 field[c] = min( min over unblocked sources k with goals[k] == c of seed[k],
 *                                 pen[c] + min over the neighbours n that c's mask allows of field[n] + w(n, c) )
 *             w = 1000 / 1414; pen = the clearance cost when a table is set (rna_goal_field_set_clearance_cost), else 0.  A
 *             source's own cell pays no pen on its seed term (the single goal's "the goal's own cost is not counted").  The
 *             30-bit rule is unchanged: a sum >= 2^30 is RNA_GOAL_FIELD_FAR, and FAR propagates as itself.  Edge weights are
 *             positive integers: the fixpoint is unique.
 *   terminal  cell c is a terminal iff some unblocked source k has goals[k] == c and seed[k] == field[c]; a tie with an
 *             equally cheap arrival through a neighbour goes to the terminal.  next[c] = 8 on terminals; everywhere else the
 *             canonical rule: the first neighbour in the contract's order with field[n] + w + pen[c] == field[c].  A source
 *             that a cheaper source undercuts is an ordinary cell.  254 / 255 as above.
 *   owner[c]  int32 per cell, BUFFER order: the smallest k with goals[k] == t and seed[k] == field[t], t the terminal the walk
 *             along next from c ends at; -1 on cells whose field is unreached or FAR.  The field strictly decreases along
 *             next, so the walks form a forest and owner is unique.
 *   paths     rna_goal_field_paths[_device] work unchanged on such a field: they walk to next == 8, cost = field[start]; a start
 *             that is a terminal gives path_len 1 and cost = its seed; the last cell of a found path is goals[owner[start]].
 * One source with start cost 0 gives byte for byte what rna_goal_field_build(goal) gives: field, next, reached, max_cost,
 * tiles_reached.  info.goal = goals[0]; info.status = 2 iff every source is blocked (every cell is then unreached, the owners
 * all -1).  Both forms return when the field -- and with RNA_GOAL_FIELD_OWNERS the labels -- is complete.  RNA_EINVAL: n < 1 or
 * n > cells, NULL goals, unknown flag bits, a goal outside [0, cells), a seed outside [0, 2^30); the _device form cannot see
 * its arrays before it enqueues: its seeding kernel skips and counts the bad entries, the host reads the count with the first
 * rounds and the call then fails with RNA_EINVAL.  A failed build leaves no field (goal == -1).  RNA_ECAPACITY as above, and for
 * an owner pass beyond its ceil(log2 cells) + 1 rounds (a defect, reported instead of a hang).
 * The owner calls return RNA_ESTATE (the pointer is NULL) when no field is built or the field was built without the flag.
 * Owner memory is 4 B per cell, allocated at the first build that asks for it and released with the field; rna_clone /
 * rna_create_submap copy nothing of it.  stale, the snapshot rule and the coexistence with pipelined batches are the single
 * goal's.  No reference counterpart. */
#define RNA_GOAL_FIELD_OWNERS 1
typedef struct {
  int32_t sources;          /* n of the build; 1 for a field built by rna_goal_field_build */
  int32_t blocked_sources;  /* skipped: their cell is in the blocked set */
  int32_t terminals;        /* cells with next == 8 */
  int32_t owners;           /* 1 = the owner labels were built */
  int32_t owner_rounds;     /* global rounds of the owner pass */
  int32_t reserved[3];      /* 0 */
} rna_goal_field_sources_info;
int rna_goal_field_build_multi(rna_engine* e, const int32_t* goals_host, const int32_t* seed_host /* NULL = 0 */, int n,
                               unsigned flags, rna_goal_field_info* info_host /* may be NULL */);
int rna_goal_field_build_multi_device(rna_engine* e, const int32_t* goals_device, const int32_t* seed_device, int n,
                                      unsigned flags, rna_goal_field_info* info_host);
int rna_goal_field_sources_info_get(const rna_engine* e, rna_goal_field_sources_info* out);   /* RNA_OK before a build: all 0 */
int rna_goal_field_owners_download(rna_engine* e, int32_t* owners_host, size_t n_cells);
void* rna_goal_field_owners_device_ptr(rna_engine* e);
int rna_goal_field_owners_at(rna_engine* e, const int32_t* cells_host, int n, int32_t* owners_host);   /* -1 for a cell out of range */

/* ---- global planning: clearance field and clearance cost (a costmap's inflation gradient) ------- */
/* The robot radius above is a hard limit: it closes a narrow door outright and leaves every cell just outside the disc as
 * cheap as the middle of the corridor.  What costmap_2d's inflation layer adds to navfn / global_planner is the gradient:
 * cells near obstacles stay passable but cost more, so plans keep their distance where there is room and still squeeze
 * through where there is none.  Two pieces:
 *   clr[c]   uint16, indexed by BUFFER linear index: the exact squared Euclidean distance in cells, di^2 + dj^2 (map space,
 *            unwrapped indices on a moved map), from c to the nearest cell of the search's blocked set -- the set
 *            rna_astar_download_blocked returns: robot radius included, masks refreshed first in the same way.  Blocked
 *            cells read 0; cells outside the map are no obstacles (CircleIterator does not visit them either).  The
 *            transform is capped at max_cells cells, 1 <= max_cells <= 63 (the footprint's bound): a cell with no blocked
 *            cell at d^2 <= max_cells^2 reads RNA_CLEARANCE_NONE.  Integers only: every value is exact.
 *   cost     a table cost_by_cells[0 .. n), 2 <= n <= 64, cap R = n - 1: entry k (1 .. R) is the cost in A* cost units of
 *            BEING ON a free cell with k^2 <= clr < (k + 1)^2; entry 0 is ignored; cells with clr > R^2 (or
 *            RNA_CLEARANCE_NONE) cost 0.  With a table set, rna_goal_field_build first makes sure a clearance field of that R
 *            exists for the current masks (it builds one if there is none, if it is stale or if it has another R), then
 *            computes the least fixpoint of
 *                field[goal] = 0,   field[c] = pen[c] + min over the neighbours n that c's mask allows of field[n] + w(n, c)
 *            (the goal's own cost is not counted).  next[c] is the first neighbour in the contract's order with
 *            field[n] + w + pen[c] == field[c]; paths follow next as before and result.cost = field[start].  A sum at or
 *            beyond 2^30 is RNA_GOAL_FIELD_FAR as before.  The batch search (rna_astar_batch) does not use the table.
 * A full rebuild per request; 2 B per cell, allocated at the first build.  `stale` follows the goal field's rule: any call
 * that can change the masks sets it.  rna_clone / rna_create_submap copy the table, not the fields.  Setting or clearing
 * the table marks an existing goal field stale (not the clearance field: the masks did not change).  No reference
 * counterpart: the reference plans on its waypoint graph and checks clearance with the one 0.3 m disc only. */
#define RNA_CLEARANCE_NONE 0xFFFF
/* on the map stream; returns when the field is complete.  RNA_EINVAL for max_cells outside 1..63 */
int rna_clearance_build(rna_engine* e, int max_cells);
int rna_clearance_download(rna_engine* e, uint16_t* host, size_t n_cells);   /* RNA_ESTATE before a build */
void* rna_clearance_device_ptr(rna_engine* e);   /* uint16 per cell, buffer order; NULL before a build */
int rna_clearance_info_get(const rna_engine* e, int* max_cells, int* stale);   /* 0, 0 before a build */
/* n == 0 (cost_by_cells may be NULL) = off, the default: every goal-field call behaves as without this section.
 * RNA_EINVAL for any other n outside 2..64.  Host only: takes effect at the next rna_goal_field_build. */
int rna_goal_field_set_clearance_cost(rna_engine* e, const uint16_t* cost_by_cells, int n);
/* returns n (0 = off, < 0 = rna_status) and writes the first min(n, cap) entries */
int rna_goal_field_get_clearance_cost(const rna_engine* e, uint16_t* out, int cap);

/* ---- global planning: line-of-sight shortcutting of cell paths ----------------------------------- */
/* Every planner above answers with an 8-connected staircase of cells.  What navfn / global_planner users do after the
 * search: reduce the plan to the few way points where it has to turn, every straight leg between two of them checked
 * against the map.  Integers only (DESIGN.md "Grid A* contract" has the full text):
 *   line(a, b)  the cells of the reference's LineIterator(map, Index start, Index end) between two cells in map space
 *               (unwrapped indices on a moved map): rna_line_cells_index.
 *   los(a, b)   every consecutive pair c_t -> c_t+1 of line(a, b) is a move the engine's current neighbour masks allow
 *               (bit of that move set in nbr[c_t], what rna_astar_download_nbr_mask returns): a leg is itself a path the
 *               grid-A* contract allows -- robot radius, diagonal corner rule and map space come with the masks.
 *   shortcut    of a path p[0 .. L): emit p[0]; a = 0; while a < L - 1: k = a + 1; while k + 1 < L and (max_span == 0 or
 *               k + 1 - a <= max_span) and ok(a, k + 1): k += 1; emit p[k]; a = k.  ok(a, m) = los(p[a], p[m]); with
 *               RNA_SHORTCUT_KEEP_CLEARANCE additionally min clr over line(p[a], p[m]) >= min clr over p[a .. m] (clr = the
 *               engine's clearance field, RNA_CLEARANCE_NONE the largest value): a leg never brings the robot closer to an
 *               obstacle than the piece of plan it replaces.  Visibility along a path is not monotone: the result is
 *               defined by the FIRST failing candidate, not by the farthest visible cell.  The original step
 *               p[a] -> p[a + 1] is always accepted, so the way points never drop below the input path.
 * Input is what rna_astar_batch[_device] / rna_goal_field_paths[_device] leave: rows of max_path_len buffer linear indices
 * plus the result records (status, path_len); output is rows of max_waypoints buffer linear indices plus one
 * rna_shortcut_result per path.  The call refreshes the masks first as rna_astar_download_nbr_mask does and uses the
 * engine's CURRENT geometry.  The _device form is asynchronous on rna_stream(): it chains behind
 * rna_goal_field_paths_device and behind rna_astar_batch_device without the host seeing a path -- the searches run on the
 * pipeline stages' own streams, so the call makes rna_stream() wait for every search still in flight (work enqueued on
 * rna_stream() after it waits with it).  Only searches that ran out of a page share set with rna_astar_set_page_cap get
 * their second pass from the host: with a page cap, call rna_synchronize() first (a row still at status 5 answers status 1).
 * The host form returns way-point rows with 0 in every slot behind the last way point (whole rows of 0 for status 1 / 2);
 * the _device form writes the way points only and leaves the other slots as the caller's buffer had them.
 * A workgroup's LDS is 4 B x max_path_len -- the row stride, not the longest path -- so a compute unit works on
 * 160 KiB / (4 x max_path_len) paths at a time: give rows no longer than the plans need.
 * Cost: an anchor on an open map sees the whole rest of its path, about L^2 / 2 mask bytes per path without max_span and
 * L * max_span with it -- that is what max_span is for.
 * RNA_EINVAL: n < 0, max_path_len < 1, max_waypoints < 2, max_span < 0 or == 1 (a span of 1 would be the identity: ask for
 * 0 = unlimited or >= 2), unknown flag bits, NULL buffers with n > 0.  RNA_ECAPACITY: max_path_len > RNA_SHORTCUT_MAX_PATH_LEN
 * (a path is staged in the LDS of one compute unit) or a map of more than 65 536 cells along an axis.  RNA_ESTATE:
 * RNA_SHORTCUT_KEEP_CLEARANCE without a built, non-stale clearance field (rna_clearance_build; the call builds nothing). */
typedef struct {
  int32_t status;        /* 0 ok; 1 no input path (input status != 0 or path_len > max_path_len); 2 invalid input path (a cell
                            out of range, or two consecutive cells that are not king-move neighbours in map space);
                            3 more way points than max_waypoints (n_waypoints = true count, the first max_waypoints written) */
  int32_t n_waypoints;   /* start and goal included; a one-cell path gives 1 */
  int32_t blocked_steps; /* original steps p[t] -> p[t + 1] the current masks do not allow: > 0 = an obstacle has landed on
                            the plan since it was computed (the replan trigger) */
  int32_t longest_span;  /* cells of the longest leg (index distance in the input path) */
} rna_shortcut_result;
#define RNA_SHORTCUT_KEEP_CLEARANCE 1
#define RNA_SHORTCUT_MAX_PATH_LEN 40960
int rna_shortcut_paths(rna_engine* e, const int32_t* paths_host, const rna_astar_result* results_host, int n, int max_path_len,
                       int max_span, unsigned flags, int32_t* waypoints_host, int max_waypoints, rna_shortcut_result* out_host);
int rna_shortcut_paths_device(rna_engine* e, const int32_t* paths_device, const rna_astar_result* results_device, int n,
                              int max_path_len, int max_span, unsigned flags, int32_t* waypoints_device, int max_waypoints,
                              rna_shortcut_result* out_device);
/* LineIterator(map, Index start, Index end) (gmc/src/iterators/LineIterator.cpp:25-28, 60-70, 106-150) as a cell list, host
 * only: raw indices (no geometry, no wrapping), max(|d0|, |d1|) + 1 cells, (i, j) pairs; returns the length of the walk
 * (only the first `cap` cells are written).  The closed form the shortcut kernel evaluates.  RNA_EINVAL for NULL arguments,
 * cap < 0 or a coordinate of magnitude 2^30 or more. */
int rna_line_cells_index(const int32_t start[2], const int32_t end[2], int32_t* cells, int cap);

/* ---- global planning: exploration frontiers (the goal source of a robot that maps while it drives) -- */
/* MapUpdater leaves NaN in every cell no ray has crossed and the engine keeps it; a frontier is where the known free space
 * ends.  Everything in map space (unwrapped indices on a moved map, no adjacency across the map edge), integers and bit
 * tests only: every output has exactly one right value.
 *   unknown(c)   the master value of c is NaN (cells outside the map are not unknown)
 *   free(c)      the master value of c is not NaN and c is not in the search's blocked set -- the set
 *                rna_astar_download_blocked returns: robot radius included, masks refreshed first in the same way
 *   frontier(c)  free(c) and at least one of c's four edge neighbours inside the map is unknown
 *   cluster      an 8-connected component of frontier cells; its label is the smallest BUFFER linear index among its cells
 *   labels[c]    int32 per cell, indexed by BUFFER linear index: the cluster's label on frontier cells, -1 elsewhere
 * One rna_frontier per cluster of at least min_size cells, sorted by label.  With RNA_FRONTIER_RANK, cost is the minimum
 * over the cluster's cells of the engine's goal-field value (compared as the raw int32: RNA_GOAL_FIELD_FAR and _UNREACHED
 * order themselves) and nearest the cell that has it, ties to the smallest buffer index: build the field at the robot's cell
 * and cost is the travel cost to the cluster, rna_goal_field_paths from nearest, reversed, the plan to it.  That needs a
 * built, non-stale goal field (RNA_ESTATE otherwise; the call builds nothing).  Without the flag cost =
 * RNA_GOAL_FIELD_UNREACHED and nearest = label.  Clusters below min_size get no record; they keep their labels.
 * A SNAPSHOT like the goal field: later map changes set info.stale (the clearance field's rule) and change nothing else.
 * Memory: 8 B per cell plus 96 B per cluster, allocated at the first build and released in rna_destroy; rna_clone /
 * rna_create_submap copy nothing of it.  No reference counterpart: the reference's only goal source is a click in rviz. */
typedef struct {
  int32_t label;         /* smallest buffer linear index of the cluster's cells */
  int32_t size;          /* cells */
  int32_t min_i, max_i, min_j, max_j;   /* bounding box, map space */
  int32_t nearest, cost; /* see RNA_FRONTIER_RANK */
  int64_t sum_i, sum_j;  /* map space: centroid = sum / size */
} rna_frontier;
typedef struct {
  int32_t cells;         /* frontier cells */
  int32_t clusters_all;  /* clusters before the size filter */
  int32_t clusters;      /* clusters after the size filter */
  int32_t largest;       /* size of the largest cluster */
  int32_t min_size;      /* the value the build was called with */
  int32_t ranked;        /* 1 = built with RNA_FRONTIER_RANK */
  int32_t stale;         /* 1 = something that can change the masks ran since the build */
  int32_t reserved;      /* 0 */
} rna_frontier_info;
#define RNA_FRONTIER_RANK 1
/* On the map stream; returns when complete.  out_host may be NULL iff cap == 0 (count only: RNA_OK).  With cap > 0 and more
 * clusters than cap: RNA_ECAPACITY, info filled with the true counts, out_host untouched, the labels valid.  RNA_EINVAL:
 * min_size < 1, cap < 0, unknown flag bits, NULL out_host with cap > 0.  RNA_ECAPACITY also for a map of 2^31 cells or more
 * and for a kernel that exceeded the stated bound of a loop (a defect, reported instead of a hang). */
int rna_frontiers_build(rna_engine* e, int min_size, unsigned flags, rna_frontier* out_host, int cap,
                        rna_frontier_info* info_host /* may be NULL */);
int rna_frontiers_info_get(const rna_engine* e, rna_frontier_info* out);   /* RNA_OK before a build too (all zero) */
int rna_frontiers_download(rna_engine* e, int32_t* labels_host, size_t n_cells);   /* RNA_ESTATE before a build */
void* rna_frontiers_device_ptr(rna_engine* e);   /* int32 per cell, buffer order; NULL before a build */

/* ---- global planning: information gain of view points (what a robot would learn at a frontier) ---- */
/* The frontiers say where the known free space ends and the goal field what it costs to get there; this says what a sensor
 * of range R cells would see from a candidate cell: exploration planners choose by utility, gain against travel cost.  Ray
 * casting over the master layer, in map space (unwrapped indices on a moved map), integers and bit tests only: every output
 * has exactly one right value.
 *   unknown(c)   the master value of c is NaN
 *   occupied(c)  the master value of c is not NaN and > 0 (GlobalPlanner::ifBlocked's predicate on the RAW layer, not the
 *                search's blocked set: the robot radius does not stop a sensor ray)
 *   opaque(c)    occupied(c); with RNA_VIEW_UNKNOWN_OPAQUE occupied(c) or unknown(c) -- the pessimistic gain: only what is
 *                certainly visible
 *   ring of v    for the view cell v = (vi, vj) and the radius R, 1 <= R <= RNA_VIEW_MAX_RADIUS: the 8R index pairs
 *                (vi + a, vj + b) with max(|a|, |b|) = R -- raw map-space indices, they may lie outside the map
 *   ray to e     c_0 = v, c_1 .. c_R = the cells of LineIterator(map, Index v, Index e) as rna_line_cells_index(v, e) returns
 *                them.  The walk goes t = 1, 2, ...: it stops before c_t when c_t is outside the map or (c_t - v) has
 *                a^2 + b^2 > R^2; otherwise c_t is seen, and if opaque(c_t) the walk stops after it
 *   seen(v)      {v} and the seen cells of all 8R rays: a set, so it depends neither on an order nor on which thread walks
 *                which ray
 * One record per view point: unknown = |seen and unknown| (the gain), visible = |seen|, occupied = |seen and occupied| (the
 * surface seen).  status 0 = evaluated: every view cell inside the map that is not occupied, an unknown one included;
 * 1 = cell index outside [0, rows * cols); 2 = the view cell is occupied; 1 and 2 give three zeros.  View cells are buffer
 * linear indices, like every other cell the ABI takes.  The call uses the engine's current geometry and the master layer as
 * rna_layer_download would see it at that point of the call sequence (on the map stream, behind the map updates enqueued so
 * far).  Not a snapshot: nothing is kept, there is no stale flag.  The _device form is asynchronous on rna_stream().
 * RNA_EINVAL: n < 0, radius_cells < 1, unknown flag bits, NULL buffers with n > 0; RNA_ECAPACITY: radius_cells >
 * RNA_VIEW_MAX_RADIUS (the window's three bitmaps, 24 480 B at 127, live in the LDS of one workgroup); n == 0 is RNA_OK.
 * The record is a struct TAG (the entry point has its name): write `struct rna_view_gain`.
 * No reference counterpart: the reference's only goal source is a click in rviz. */
struct rna_view_gain {
  int32_t status;        /* 0 evaluated; 1 cell out of range; 2 the view cell is occupied */
  int32_t unknown;       /* seen cells that are unknown: the gain */
  int32_t visible;       /* seen cells, the view cell included */
  int32_t occupied;      /* seen cells that are occupied */
};
#define RNA_VIEW_UNKNOWN_OPAQUE 1
#define RNA_VIEW_MAX_RADIUS 127
int rna_view_gain(rna_engine* e, const int32_t* cells_host, int n, int radius_cells, unsigned flags, struct rna_view_gain* out_host);
int rna_view_gain_device(rna_engine* e, const int32_t* cells_device, int n, int radius_cells, unsigned flags,
                         struct rna_view_gain* out_device);

/* ---- pose source: scan matching (correct a pose by correlating a scan with the map) ---------- */
/* The map is built from whatever sensor pose the caller passes to rna_scan_to_rays; in the reference that is tf's odom ->
 * base_link, never corrected, and HIMM writes every wall twice once odometry has drifted.  This is the correlative
 * scan-to-map matcher that sits at that seam: before a scan is fused, search a small window of poses round the guess for
 * the one at which the scan's end points fall on the map's occupied cells.  An exhaustive search over rotations x
 * (2T + 1)^2 cell shifts x points, stated over integers: every output has exactly one right value.
 * Everything is in INDEX space (index i grows as x falls, as GridMap::getIndex), cells are map-space cells (unwrapped on a
 * moved map), and the master layer is read as rna_layer_download would see it at that point of the call sequence.
 *   occupied(c)  c is inside the map and its master value is not NaN and > 0 (GlobalPlanner::ifBlocked's predicate on the
 *                RAW layer: no robot radius)
 *   bit_l(c)     l = 0 .. L - 1: some occupied cell lies within Chebyshev distance l of c.  Defined on all of Z^2: a cell
 *                outside the map next to an occupied edge cell has bit_1.  w(c) = sum over l of bit_l(c), an integer
 *                likelihood ramp: L on a wall, L - 1 next to it, ...  1 <= L <= RNA_SCAN_MATCH_MAX_LEVELS
 *   points       (px, py), an int32 pair in Q6 (1/64 of a cell), sensor frame, already in index orientation.  A point is
 *                USED iff |px|, |py| <= 32767 and px^2 + py^2 <= (64 R)^2, R = range_cells, 1 <= R <=
 *                RNA_SCAN_MATCH_MAX_RANGE: no rotation enters, n_used is one number per query
 *   rotation r   a pair (c, s) of int32 in Q14 supplied by the caller, n_rot of them per query (1 <= n_rot <=
 *                RNA_SCAN_MATCH_MAX_ROT), those of query q from rot[2 * q * n_rot]:
 *                  qx = (c * px - s * py + 8192) >> 14,  qy = (s * px + c * py + 8192) >> 14   (arithmetic shifts)
 *                With |c|, |s| <= 16384 everything fits int32; beyond that the products wrap (no score is promised).
 *   guess        `cell` = the buffer linear index of the cell that holds the sensor, (gi, gj) its map-space index; sub[2] =
 *                the sensor's offset from that cell's centre in Q6, in [-32, 31].  The cell a point falls in is
 *                  a = gi + ((qx + sub[0] + 32) >> 6),  b = gj + ((qy + sub[1] + 32) >> 6)
 *                For a pair of magnitude 16384 (lrint(16384 cos), lrint(16384 sin)) and sub in range, |a - gi|, |b - gj| <=
 *                R.  A used point with |a - gi| or |b - gj| > R + 1 (another pair, another sub) adds nothing to the scores
 *                of that rotation; it still counts in n_used.
 *   score        score(r, da, db) = sum over the used points of w((a + da, b + db)), |da|, |db| <= T = max_shift,
 *                0 <= T <= RNA_SCAN_MATCH_MAX_SHIFT
 *   best         compared in this order: greatest score; smallest da^2 + db^2; smallest |r - r_c|, r_c = n_rot / 2;
 *                smallest r; smallest db; smallest da.  A total order: one value whatever the arrival order.
 * One record per query: status 0 = matched, score = the best's, rot = its r, shift = its (da, db), n_used, score_guess =
 * score(r_c, 0, 0), score_max = n_used * L.  status 1 = `cell` outside [0, rows * cols); status 2 = no used point; both
 * give rot = r_c, zero shift, zero scores and n_used.  `volume`, when not NULL, receives every score as
 * [n][n_rot][2T + 1 (db)][2T + 1 (da)] int32 (zeros for status 1 and 2): what a caller fits a covariance to.
 * n_points <= RNA_SCAN_MATCH_MAX_POINTS per query; points_offset counts points (pairs) of the concatenated array of
 * n_points_total points.  A query whose points leave that array: RNA_EINVAL from the host form, status 2 in the _device form.
 * RNA_EINVAL: NULL engine, n < 0, n_rot, range_cells or levels < 1, max_shift < 0, NULL buffers with n > 0 (volume may be
 * NULL), in the _device form records that are not 8-byte aligned; RNA_ECAPACITY (with error text): range_cells, max_shift,
 * levels or n_rot beyond its define, or n * n_rot >= 2^24 (one workgroup each, one launch); n == 0 with valid arguments is
 * RNA_OK.  Argument checks come before anything reads the
 * engine.  The _device form is asynchronous on rna_stream(): three enqueues, nothing is read back; the records hold
 * intermediate values until the last has run.  Nothing is kept: no snapshot, no device memory.
 * The record is a struct TAG (the entry point has its name): write `struct rna_scan_match`.
 * No reference counterpart: MapProvider never corrects the pose (gmapping is a commented-out line of a launch file). */
struct rna_scan_match {
  int32_t status;        /* 0 matched; 1 cell out of range; 2 no used point */
  int32_t score;         /* the best score */
  int32_t rot;           /* its rotation slot r */
  int32_t shift[2];      /* its (da, db), cells in index space */
  int32_t n_used;        /* used points */
  int32_t score_guess;   /* score(r_c, 0, 0): what the guess itself scores */
  int32_t score_max;     /* n_used * levels: every point on an occupied cell */
};
typedef struct {
  int32_t cell;          /* buffer linear index of the cell that holds the sensor */
  int32_t sub[2];        /* offset of the sensor from that cell's centre, Q6, [-32, 31] */
  int32_t points_offset; /* first point of this query in the concatenated points array */
  int32_t n_points;
} rna_scan_match_query;
#define RNA_SCAN_MATCH_MAX_RANGE 127
#define RNA_SCAN_MATCH_MAX_SHIFT 16
#define RNA_SCAN_MATCH_MAX_LEVELS 4
#define RNA_SCAN_MATCH_MAX_ROT 128
#define RNA_SCAN_MATCH_MAX_POINTS 8192
int rna_scan_match(rna_engine* e, const rna_scan_match_query* queries_host, int n, const int32_t* points_host, size_t n_points_total,
                   const int32_t* rot_host, int n_rot, int range_cells, int max_shift, int levels,
                   struct rna_scan_match* out_host, int32_t* volume_host /* may be NULL */);
int rna_scan_match_device(rna_engine* e, const rna_scan_match_query* queries_device, int n, const int32_t* points_device,
                          size_t n_points_total, const int32_t* rot_device, int n_rot, int range_cells, int max_shift, int levels,
                          struct rna_scan_match* out_device, int32_t* volume_device /* may be NULL */);
/* Two host-only helpers, like rna_geometry_index: no engine, no GPU.
 * rna_scan_match_prepare turns a scan's end points (sensor frame, metres, x y pairs) and a pose guess into one query:
 *   points_q6[2k], [2k + 1] = lrint(-p / resolution * 64) (the sign is the index orientation; flipping both axes commutes
 *                with a rotation), values beyond +-2^30 and NaN become 2^30 (never a used point);
 *   rot_q14[2r], [2r + 1] = lrint(16384 * cos / sin(yaw + (r - r_c) * yaw_step)), r_c = n_rot / 2;
 *   q->cell from (x, y) by the math of rna_geometry_index, q->sub = lrint(-(position - cell centre) / resolution * 64)
 *                clamped to [-32, 31]; q->points_offset = 0, q->n_points = n_points.
 * Returns 1; 0 when (x, y) is outside the map, with q->cell = -1 and sub 0 (points and rotations are still written);
 * RNA_EINVAL for a bad geometry, NULL pointers, n_points < 0 or > RNA_SCAN_MATCH_MAX_POINTS, n_rot < 1 or >
 * RNA_SCAN_MATCH_MAX_ROT.
 * rna_scan_match_pose turns a record back into a pose: pose = (x - shift[0] * resolution, y - shift[1] * resolution,
 * yaw + (rot - r_c) * yaw_step) -- a shift of +1 in index space lowers the coordinate by one resolution.  A record with
 * status != 0 (rot = r_c, zero shift) returns the guess.  Returns RNA_OK or RNA_EINVAL. */
int rna_scan_match_prepare(const rna_geometry* g, const double* points_xy, int n_points, double x, double y, double yaw, double yaw_step,
                           int n_rot, rna_scan_match_query* q, int32_t* points_q6, int32_t* rot_q14);
int rna_scan_match_pose(const rna_geometry* g, double x, double y, double yaw, double yaw_step, int n_rot, const struct rna_scan_match* m,
                        double pose[3]);

/* ---- global planning: waypoint-graph A* (the reference's own AStarPlanner) ------------------- */
/* AStarPlanner::init + makePlan over a caller-supplied graph (astar_planner.cpp:63-145): start and
 * target positions are snapped to the closest vertex; path = start, vertex locations..., target.
 * 1 <= n_vertices <= 256, edge ends in [0, n_vertices), max_len >= 3; path_len[q] is the number of positions of the route
 * (0 = no route); a row of paths_xy is written only when path_len[q] <= max_len and is otherwise left as the caller had it.
 * A NEGATIVE EDGE WEIGHT IS REFUSED (RNA_EINVAL, nothing is launched).  Boost refuses it too: astar_bfs_visitor::examine_edge
 * throws negative_edge.  On an undirected edge it is a negative cycle: relax() lowers the distance of either end in turn and
 * re-opens both, until float absorption stops it -- 2^24 + 2 pops, each with one relaxation and one re-opening, in the CPU
 * restatement (oracle/astar.c, counted by tests/test_graph_astar_host.py) for two vertices joined by an edge of weight -1 and
 * a goal that is not connected: that would be one lane's work.  -0.0 and NaN pass: a NaN weight never relaxes, here and in
 * Boost alike.  RNA_EINVAL as well for any other argument out of the ranges above; n = 0 is RNA_OK. */
int rna_graph_astar_batch(rna_engine* e, int n_vertices, const double* vertex_xy, int n_edges,
                          const int32_t* edge_uv, const float* edge_weight /* NULL = 0 as the reference */,
                          const double* start_target_xy /* n*4 */, int n, double* paths_xy /* n*max_len*2 */,
                          int max_len, int32_t* path_len);

/* ---- global planning: RRT (mc/src/rrt_planner.cpp) -------------------------------------------- */
typedef struct {
  double start[2], target[2];
  double close_tolerance;      /* RrtPlanner ctor default 0.2 */
  uint32_t seed;               /* srand(seed) of this query's private glibc-compatible rand() */
  int32_t max_samples;         /* bound for extendTree's while(true) */
} rna_rrt_query;
typedef struct { int32_t status, path_len, tree_size, samples; } rna_rrt_result;
/* RrtPlanner::makePlan for n queries on the master layer, one workgroup a query, each with its own rand() stream.
 *   status     1  reached: the last node is within close_tolerance of the target or, for a target outside the map, of the
 *                 map's border (ifFinishPlan);
 *              0  the tree is full at its 2000 nodes (rrt_planner.cpp:6) without having reached; the path is the one from the
 *                 last node, as makePlan returns it;
 *             -1  the budget of max_samples draws of extendTree ran out: no path, path_len 0.  max_samples <= 0 is -1 at
 *                 once, with tree_size 1 and samples 0 (unless the start itself finishes the plan: status 1, path_len 1).
 *   tree_size  nodes in the tree, the start included; samples: draws of extendTree, blocked ones included.
 *   Way points run goal -> start, as backtraceTree leaves them: row q of paths_xy (max_path_len x 2 doubles) holds the last
 *   node first and the query's start last.
 *   path_len is the FULL length of the path even when it exceeds max_path_len; only the first max_path_len way points
 *   (the goal side) are then written.  A tree never holds more than 2000 nodes, so max_path_len = 2000 cuts nothing.
 *   What the call does not write -- a row behind min(path_len, max_path_len) way points, the whole row of a query with
 *   status -1 -- comes back as the caller had it, in both forms (the host form uploads the caller's rows first).
 *   findNearNode's `shortest = 9999.0` is kept: a sample 9999 m or more from every node extends node 0, the start.
 * RNA_EINVAL for max_path_len <= 0, n < 0 or a null pointer with n > 0, before anything is launched; n = 0 is RNA_OK and
 * touches nothing.  Starts are expected inside the map; close_tolerance and the positions finite.  The _device form is
 * asynchronous on the engine stream. */
int rna_rrt_batch(rna_engine* e, const rna_rrt_query* queries_host, int n, double* paths_xy_host,
                  int max_path_len, rna_rrt_result* results_host);
int rna_rrt_batch_device(rna_engine* e, const rna_rrt_query* queries_device, int n, double* paths_xy_device,
                         int max_path_len, rna_rrt_result* results_device);

/* ---- laser ingestion ------------------------------------------------------------------------- */
/* One sensor_msgs/LaserScan plus the planar sensor poses tf reports for it: at header.stamp, and at the end time
 * laser_geometry's high-fidelity projection asks for, stamp + (beams - 1) * time_increment, where `beams` counts the
 * beams of the scan that is projected -- the decimated one when angle_increment < 0.017 (rna_scan_projected_beams).
 * Every beam is transformed with the pose interpolated for its index (position linearly, yaw along the shortest arc),
 * as transformLaserScanToPointCloud does with tf's start / end transforms.  End pose == start pose: a pose that is
 * constant over the scan.
 * The arithmetic, all in double, each operation rounded on its own (tests/_scan_reference.py replays it): beam i of n projected
 * beams has ratio = i * (1 / (n - 1)), 0 for n = 1; its point is (float)(range * cos(a)), (float)(range * sin(a)) with
 * a = angle_min + i * angle_increment (the decimated scan's increment); dyaw = fmod(yaw_end - yaw, 2 pi), less 2 pi if above
 * pi, then plus 2 pi if below -pi; yaw_i = yaw + ratio * dyaw; t = (1 - ratio) * start + ratio * end per coordinate; end point
 * (float)((cos(yaw_i) * px - sin(yaw_i) * py) + tx), (float)((sin(yaw_i) * px + cos(yaw_i) * py) + ty).  A scan of no range
 * gives no ray. */
typedef struct {
  float angle_min, angle_max, angle_increment, range_min, range_max;
  int32_t n_ranges;
  int64_t ranges_offset;   /* first range of this scan in the concatenated ranges array */
  double x, y, yaw;        /* sensor pose in the map frame at header.stamp (also the origin of every ray) */
  double x_end, y_end, yaw_end;   /* sensor pose at the end time */
} rna_laser_scan;
/* number of beams of the scan LaserMapUpdater hands to the projector (simplifyLaserScan, mc/src/laser_map_updater.cpp:
 * 118-143, when angle_increment < 0.017; else n_ranges): the end time above is stamp + (this - 1) * time_increment */
int rna_scan_projected_beams(int n_ranges, float angle_increment);
/* LaserMapUpdater::bufferIncomingMsg (mc/src/laser_map_updater.cpp:37-75): simplifyLaserScan
 * (:118-143), laser_geometry's projection + tf transform of every valid beam (:78-99), ray origin
 * (:101-116) -> RangeSamples in scan order, beam order.  n_rays receives the number of rays produced;
 * RNA_ECAPACITY if it exceeds max_rays (the first max_rays rays are still written).  The device
 * variant leaves the count in device memory; max_beams_per_scan >= every scan's n_ranges (<= 8192). */
int rna_scan_to_rays(rna_engine* e, const rna_laser_scan* scans_host, int n_scans, const float* ranges_host,
                     size_t n_ranges_total, rna_ray* rays_host, int max_rays, int* n_rays);
int rna_scan_to_rays_device(rna_engine* e, const rna_laser_scan* scans_device, int n_scans, const float* ranges_device,
                            int max_beams_per_scan, rna_ray* rays_device, int max_rays, int* n_rays_device);

/* The same with the sensor's FULL pose (a tilted or rolled mount, a sensor above the base): what tf's lookupTransform
 * (map frame <- header.frame_id) returns at the two times, translation and rotation quaternion (x, y, z, w) as
 * StampedTransform::getOrigin / getRotation give them.  Every beam's point (x, y, 0 in the sensor frame, float32) goes
 * through the transform interpolated for its index -- translation by tf::Vector3::setInterpolate3, rotation by
 * tf::Quaternion::slerp (shortest arc) -- and the map keeps x and y of the result, as LaserMapUpdater reads only the
 * cloud's x and y fields (mc/src/laser_map_updater.cpp:53-60, 78-99).  The ray origin is the start translation's x, y
 * (tf::transformPoint of the frame's origin, :101-116).  For a planar pose (rotation about z) the result equals
 * rna_scan_to_rays' up to the rounding of the two formulations. */
typedef struct {
  float angle_min, angle_max, angle_increment, range_min, range_max;
  int32_t n_ranges;
  int64_t ranges_offset;   /* first range of this scan in the concatenated ranges array */
  double t[3], q[4];       /* sensor frame in the map frame at header.stamp: translation, quaternion x y z w */
  double t_end[3], q_end[4];   /* ... at the end time (see rna_laser_scan) */
} rna_laser_scan_tf;
int rna_scan_to_rays_tf(rna_engine* e, const rna_laser_scan_tf* scans_host, int n_scans, const float* ranges_host,
                        size_t n_ranges_total, rna_ray* rays_host, int max_rays, int* n_rays);
int rna_scan_to_rays_tf_device(rna_engine* e, const rna_laser_scan_tf* scans_device, int n_scans, const float* ranges_device,
                               int max_beams_per_scan, rna_ray* rays_device, int max_rays, int* n_rays_device);

/* One sensor_msgs/Range reading (sonar) plus the planar sensor pose tf reports for its stamp. */
typedef struct {
  float range, max_range;  /* msg->range, msg->max_range */
  double x, y, yaw;        /* sensor pose in the map frame */
} rna_range_reading;
/* RangeMapUpdater::bufferIncomingMsg (mc/src/range_map_updater.cpp:38-76), host only: one RangeSample per reading,
 * start = T(0,0,0), end = T(range,0,0) (tf::transformPoint in double), ifClearEnd = !(range < max_range).  The rays
 * go to rna_himm_update(e, RNA_LAYER_RANGE, ...) -- the "range" MapUpdater of MapProvider's factory
 * (mc/src/map_provider.cpp:12-15,262-266); master is composed from the laser layer only (:216-223). */
int rna_range_to_rays(const rna_range_reading* readings, int n, rna_ray* rays);
/* The same with the sensor's full pose (translation + quaternion x y z w, as above): start = T * (0, 0, 0),
 * end = T * (range, 0, 0), x and y kept. */
typedef struct {
  float range, max_range;
  double t[3], q[4];
} rna_range_reading_tf;
int rna_range_to_rays_tf(const rna_range_reading_tf* readings, int n, rna_ray* rays);

/* ---- message formats either side of the path ------------------------------------------------- */
/* GridMapRosConverter::toOccupancyGrid (grid_map-master/grid_map_ros/src/GridMapRosConverter.cpp:251-287)
 * as MapProvider::publishMap calls it with (0, 255) (mc/src/map_provider.cpp:113-118,206-213):
 * out[nCells-1-(ui + uj*rows)] = NaN or negative -> -1, else (int8)(clamp((v-min)/(max-min), 0, 1)*100),
 * (ui, uj) the unwrapped index -- info.width = rows, info.height = cols, origin = position - length/2
 * (rna_get_geometry).  out holds rows*cols int8. */
int rna_to_occupancy_grid(rna_engine* e, int layer, float data_min, float data_max, int8_t* out_host);
int rna_to_occupancy_grid_device(rna_engine* e, int layer, float data_min, float data_max, int8_t* out_device);
/* GridMapRosConverter::fromOccupancyGrid, data part (:238-246): layer(i) = data[n-1-i], -1 -> NaN.  The
 * geometry part (:208-236) is rna_create(resolution*size, resolution, origin + length/2). */
int rna_from_occupancy_grid(rna_engine* e, int layer, const int8_t* data_host);
/* Steerer::pubHist -> move_control/Histogram.msg (mc/src/steerer.cpp:201-220) for the first n VFH
 * instances: num_bin = hist_size/2 per robot; x_data[num_bin] (shared), y_data / y_bin_data
 * [n][num_bin] = (uint16)(int)OriginHist / Hist; thresholds = {yLowThreshold, yHighThreshold}. */
int rna_vfh_hist_msg_batch(rna_engine* e, int n, uint16_t* x_data_host, uint16_t* y_data_host,
                           uint16_t* y_bin_data_host, uint16_t thresholds[2]);
/* Nav::taileredPlan (mc/src/nav_node.cpp:192-204): walk the plan backwards keeping every stride-th
 * index and the last one (host only; out_xy holds up to n positions).  The stride is blind to the map; the map-aware
 * alternative is rna_shortcut_paths above: the way points where the plan has to turn, every leg checked against the masks. */
int rna_tailor_plan(const double* plan_xy, int n, unsigned stride, double* out_xy, int* n_out);
/* Steerer::acceptPlan + the plan-following head of Steerer::update (mc/src/steerer.cpp:27-33,222-256), host only:
 * *plan_index is Steerer::planIndex_ (acceptPlan sets it to 1); way points closer than 250 mm are skipped, then
 * goal distance (mm, float hypot), goal direction (deg, RAD2DEG(normalize_angle_positive(atan2f(dy,dx) - yaw + M_PI/2)))
 * and current_speed = (int)(linear_velocity * 1000.0) are written to *pose together with x, y, yaw, dt -- ready for
 * rna_vfh_step_batch.  Returns 1 while the plan is being followed, 0 when it is finished (ifPlanReady_ = false;
 * also for a plan of fewer than 2 points, where the reference reads plan_[1] out of bounds), < 0 on bad arguments. */
int rna_follow_plan(const double* plan_xy, int n, int32_t* plan_index, double x, double y, double yaw,
                    double linear_velocity, double dt, rna_pose* pose);

/* ---- measurement ------------------------------------------------------------------------------ */
typedef enum {
  RNA_K_HIMM_PREP = 0, RNA_K_HIMM_RASTER, RNA_K_HIMM_APPLY, RNA_K_COMPOSE, RNA_K_NBRMASK,
  RNA_K_VFH_STEP, RNA_K_ASTAR_SEARCH, RNA_K_ASTAR_INIT, RNA_K_RRT, RNA_K_OCCUPANCY, RNA_K_ASTAR_RESET,
  RNA_K_FOOTPRINT, RNA_K_COUNT
} rna_kernel_id;
/* when enabled, every launch of the kernels above is bracketed by hipEvents on the stream it runs on (the engine
 * stream; astar_search: the pipeline stage's own stream; astar_init / astar_reset / vfh_step: the side stream) */
/* on: 0 off, 1 every slot, 2 only astar_search / astar_reset (an event record is a packet of its own on the stream:
 * bracketing the ten slots of the engine stream costs its chain of short kernels about 1 ms per replan pass) */
int rna_profile_enable(rna_engine* e, int on);
int rna_profile_reset(rna_engine* e);
int rna_profile_get(rna_engine* e, int kernel_id, double* total_ms, int64_t* launches);
const char* rna_kernel_name(int kernel_id);

#ifdef __cplusplus
}
#endif
#endif /* RNA_H */
