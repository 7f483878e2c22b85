// engine.hpp -- internal state of one rna_engine (librna.so).  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/rna.h"
#include "gridmath.hpp"
#include "map_state.hpp"

// control words of the goal field and of the frontiers, the VFH+ kernels' argument: each private to its file (defined in its unnamed namespace)
namespace {
struct GfCtl;
struct FrCtl;
struct VfhK;
}  // namespace

namespace rna {

constexpr int TILE = 64;  // dirty-tracking / mask tile edge (cells)

struct HimmSlot { int cell; int head; int len; int offset; };

struct HimmScratch {
  int cap_rays = 0;
  int n_slots = 0;
  rna_ray* rays_dev = nullptr;   // staging for host-pointer calls
  int4* desc = nullptr;          // clipped start/end indices per ray
  int* ncells = nullptr;         // Bresenham cell count per ray (0 = no cells)
  int* next = nullptr;           // chain of marks per cell
  HimmSlot* slots = nullptr;     // open-addressing hash cell -> marks
  int* seqs = nullptr;           // sorted ray sequence numbers of marks, grouped per cell
  unsigned* before = nullptr;    // clears that land before mark k
  unsigned* after = nullptr;     // clears after the last mark of the cell
  int* total = nullptr;          // allocation cursor into seqs
  unsigned* mark_bitmap = nullptr;  // 1 bit per cell: cell holds >= 1 mark in the current batch
  int* pairs = nullptr;          // (tile, ray) pairs grouped by tile: the rays each 64 x 64 tile has to rasterise
  size_t pairs_cap = 0;          // ints allocated for them
  bool pairs_checked = false;    // pairs_cap is below the worst case: every batch's pair count is read back before it is used
  int* pairs_total_host = nullptr;   // pinned: the count of the batch being launched (pairs_checked only)
  int* tile_bins = nullptr;      // per-tile pair counts, offsets, fill cursors and the rasteriser's job list: one block, laid out by HimmBins (himm.hip)
  int win[4] = {0, 0, 0, 0};     // owner window [i0, i1) x [j0, j1) in buffer indices; i1 == 0: whole map
};

struct VfhDevice {
  bool ready = false;
  rna_vfh_params p{};
  int n_robots = 0, H = 0;
  char *tables = nullptr, *state = nullptr;   // the two device blocks, laid out by VfhLayout (vfh_tables.hpp)
  float *hist = nullptr, *origin = nullptr;   // [n_robots][H] of the state block (msgs.hip reads them)
  VfhK* k = nullptr;                          // the kernels' argument, filled once by rna_vfh_init (host memory, vfh.hip)
  rna_pose* poses_dev = nullptr; rna_vfh_out* out_dev = nullptr; double* ranges_dev = nullptr;   // staging of the host forms, allocated at their first call
};

// One pipeline stage of the grid A* (astar.hip owns it; astar_tile.hip lays out its blocks and launches on its stream).
struct AstarStage {
  unsigned* pool = nullptr;        // page pool: the pages, then their edge-column copies (astar_tile.hip, TsaStage)
  int32_t* rev = nullptr;          // reversed-path staging per query
  char* block = nullptr;           // starts zeroed: ticket and counters | page counts | launch order | mask snapshot | tile -> page | page -> tile
  unsigned* retry_pool = nullptr;  // only when page_cap < tiles of the map: TSA_RETRY slots with a page per tile, and their block,
  char* retry_block = nullptr;     // for the second pass over searches that outgrew their pages (astar_tile.hip)
  hipStream_t stream = nullptr;    // pipelined only (depth > 1); one stream: the engine stream
  hipEvent_t done = nullptr;       // the search of the stage's last batch (and its second passes so far) has finished
  hipEvent_t snap_done = nullptr;  // the mask snapshot of the stage's batch (taken on the side stream) has been taken
  bool snap_pending = false;
  bool busy = false;               // `done` is recorded and the host has not seen it complete yet
  unsigned long long seq = 0;      // launch number of the stage's last batch (0: never used)
  // Searches that outgrew their share of pages are counted by the kernel and the count is copied to pinned host memory behind the search;
  // their second pass is launched when the host sees it (a launch per batch "in case" cost every stage 0.2 - 4 ms: its workgroups wait for CU slots)
  int* retry_flag = nullptr;       // the stage's word of AstarDevice::retry_flag (null: the stage has no retry slots)
  bool retry_armed = false;
  int last_retried = 0;            // searches of the stage's last batch that went through the second pass
  size_t last_lds = 0;
  alignas(8) unsigned char last_launch[384] = {};   // TsaLaunch of the stage's last batch
};
// One entry of the launch ring: ticket, launch order and mask snapshot of one batch (AstarDevice::ring_mem + index * ring_stride).
struct AstarRingEntry {
  hipEvent_t free = nullptr;       // the search that read this entry last has finished
  bool used = false;
};

struct AstarDevice {
  int max_queries = 0;
  int bucket_width = 128000;        // f-range of one bucket (128 cells; round 6, on the bench: 72 / 96 / 128 / 160 / 200 / 256 k -> 159.8 / 160.8 / 162.2 / 159.7 / 158.5 / 159.3 k cycles/s, profiles/r06_sweep_bucket_width.txt); inside it free wavefronts take the tile with the lowest key (astar_tile.hip)
  // Pipelined batches: `depth` independent stages, each with its own HIP stream, so the tail of batch k (few long
  // queries) overlaps the head of batch k+1.
#ifndef RNA_ASTAR_MAX_DEPTH
#define RNA_ASTAR_MAX_DEPTH 20   // (developer builds may raise it: scripts/r06_depth_hwq.sh)
#endif
  // From 22 stages on the rate falls by a fifth, with GPU_MAX_HW_QUEUES = 8 and = 24 alike (profiles/r04_sweep_depth_16_22_engine_max_24.txt,
  // r06_sweep_depth_hw_queues.txt): the process then holds 25 queues (the stages' streams, the engine stream, the side stream, the null stream).
  static constexpr int MAX_DEPTH = RNA_ASTAR_MAX_DEPTH;
  int depth = 4;
  AstarStage stage[MAX_DEPTH];
  bool live() const { return stage[0].pool != nullptr; }   // the configuration is allocated
  int rev_cap = 16800;             // g < 2^24 at >= 1000 per step bounds a path to 16 777 cells
  int page_cap = 0;                // 4 KiB pages per query (0 = one per tile: a search can never run out)
  int page_cap_request = 0;        // rna_astar_set_page_cap
  // Pipelined launches: the mask snapshot, the launch order and the ticket of a batch live in an entry of a ring, not in
  // the stage -- they are written on the engine's side stream (CUs the searches cannot take) as soon as the map is
  // composed, before any stage has to be free; the search itself goes to a stage that IS free (the host waits for one).
  static constexpr int MAX_RING = 2 * MAX_DEPTH;
  int ring_n = 0;
  char* ring_mem = nullptr;
  size_t ring_stride = 0;
  AstarRingEntry ring[MAX_RING];
  hipEvent_t ev_init = nullptr;          // the engine stream has reached the launch: the masks are what the batch shall see
  hipEvent_t ev_prep = nullptr;          // snapshot + launch order of the batch being launched are in place
  int* retry_flag = nullptr;             // pinned host memory, an int per possible stage: copied from the stage's device counter behind each search
  unsigned long long launches = 0;
  int last_slot = 0;
  rna_astar_query* queries_dev = nullptr;
  rna_astar_result* results_dev = nullptr;
  int32_t* paths_dev = nullptr;
  int paths_cap = 0;               // max_queries * max_path_len currently allocated
  const rna_astar_query* last_queries = nullptr;   // device pointers of the last launched chunk
  const rna_astar_result* last_results = nullptr;
  int last_n = 0;
};

// The disc of GlobalPlanner::ifBlocked with radius r as a stencil of cell offsets (footprint.hip): every offset (di, dj),
// |di|, |dj| <= R = ceil(r / res), is sure-in, sure-out or a tie by the nominal distance (di^2 + dj^2) res^2 against r^2
// with a margin that bounds the rounding of the reference's f64 cell-centre arithmetic for coordinates up to `mag`.
// Row dj's sure-in offsets are di in [-w[|dj|], w[|dj|]] (w = -1: none); ties are evaluated per cell in f64.
struct FootprintPlan {
  double r = 0.0, res = 0.0, mag = 0.0;   // radius, resolution and coordinate magnitude the plan was made for
  int R = 0;                              // stencil half-extent (cells)
  int K = 0;                              // largest |di| (= |dj|) of an offset that is not sure-out (<= R)
  int band = 0;                           // cells closer than this to the map edge (map space) check their bounding box
  int n_ties = 0;
  int w[64] = {};
};

// A module's device control words and their pinned host copy.
template <typename T>
struct CtlPair {
  T* dev = nullptr;
  T* host = nullptr;
  int alloc(rna_engine* e);     // RNA_ENOMEM when either is refused
  void release();
  int read(rna_engine* e);      // the launch check of the kernels enqueued so far, then the words as they leave them: returns with the engine stream idle
};

// The goal distance field (goal_field.hip): a snapshot of cost-to-goal and canonical steps, built on request.
struct GoalField {
  int32_t* field = nullptr;        // [ncell] buffer order: exact distance, RNA_GOAL_FIELD_UNREACHED / _FAR
  uint8_t* next = nullptr;         // [ncell] neighbour number 0-7 of the canonical step, 8 = goal, 254 = far, 255 = unreached
  int* keys = nullptr;             // [2][tiles]: pending key per map-space tile, this round's and the next one's
  uint8_t* touched = nullptr;      // [tiles]: the tile has been relaxed during this build
  CtlPair<GfCtl> ctl;              // control words
  int rows = 0, cols = 0, s0 = 0, s1 = 0;   // geometry the field was built with (paths are walked in its map space)
  unsigned long long epoch = 0;    // rna_engine::map.epoch at the build
  rna_goal_field_info info{-1, 0, 0, 0, 0, 0, 0, 0};
  // many sources (rna_goal_field_build_multi): the last build's source counts, and the owner labels when it asked for them
  rna_goal_field_sources_info sources{0, 0, 0, 0, 0, {0, 0, 0}};
  int32_t* owner = nullptr;        // [ncell] buffer order, allocated at the first build with RNA_GOAL_FIELD_OWNERS: index of the
                                   // source the walk along next ends at, -1 unreached / far
  // clearance cost (rna_goal_field_set_clearance_cost): cost_n == 0 = off, the field is the plain 1000 / 1414 one
  uint16_t cost_tab[64] = {};      // entry k: cost of a free cell with k^2 <= clearance < (k + 1)^2 (entry 0 unused)
  int cost_n = 0;                  // entries (2..64): the clearance cap is cost_n - 1 cells
  bool cost_changed = false;       // the table was set or cleared since the build: the field reports itself stale
  uint16_t* pen = nullptr;         // device: the cost by SQUARED clearance, (cost_n - 1)^2 + 1 entries
  bool pen_current = false;        // pen holds the present table
};

// The clearance field (clearance.hip): squared distance of every cell to the nearest blocked cell, built on request.
struct Clearance {
  uint16_t* clr = nullptr;         // [ncell] buffer order: di^2 + dj^2, 0 on blocked cells, RNA_CLEARANCE_NONE beyond the cap
  int R = 0;                       // cap in cells of the field that is there (0 = none)
  unsigned long long epoch = 0;    // rna_engine::map.epoch at the build
};

// Exploration frontiers (frontier.hip): labels of the 8-connected clusters of frontier cells and their records, built on request.
struct Frontiers {
  int32_t* labels = nullptr;       // [ncell] buffer order: the cluster's smallest buffer index on frontier cells, -1 elsewhere
  int32_t* slot = nullptr;         // [ncell] written at root cells only: the root's entry of rec
  rna_frontier* rec = nullptr;     // [rec_cap] one accumulator per cluster, in arrival order
  rna_frontier* out = nullptr;     // [rec_cap] the records that passed the size filter
  int rec_cap = 0;
  CtlPair<FrCtl> ctl;              // control words
  bool built = false;
  unsigned long long epoch = 0;    // rna_engine::map.epoch at the build
  rna_frontier_info info{0, 0, 0, 0, 0, 0, 0, 0};
};

struct ProfSlot {
  double total_ms = 0;
  int64_t launches = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;  // recorded, not yet read back
};

}  // namespace rna

struct rna_engine {
  rna::Geom geom{};
  int device = 0;
  int cu_count = 256;              // compute units of the device (MI355X: 256 = 8 XCDs x 32)
  hipStream_t stream = nullptr;
  // Side work: the pipelined replan loop runs the VFH+ step and the mask snapshot + launch order of a search batch on
  // a stream of their own, so that neither sits in the engine stream's chain of map-update kernels.  Both only READ
  // the map (master layer / neighbour masks); whatever may WRITE what they read joins them first (RNA_ENTER).
  hipStream_t vfh_stream = nullptr;
  hipEvent_t ev_vfh_go = nullptr, ev_vfh_done = nullptr;
  bool vfh_pending = false;
  size_t ncell = 0;
  float* layer[RNA_NUM_LAYERS] = {nullptr, nullptr, nullptr};
  int tiles_i = 0, tiles_j = 0;
  unsigned* dirty_tiles = nullptr;   // one BYTE per TILE x TILE tile: laser changed since last compose
  unsigned* last_dirty = nullptr;    // the flags the last compose consumed (tiled mode: what this GPU has to hand on)
  int32_t* tile_list = nullptr;      // staging for rna_layer_pack_tiles / rna_layers_unpack_tiles
  int tile_list_cap = 0;
  rna::MapState map;                 // what the next compose or search has to redo, and the epoch (map_state.hpp)
  uint8_t* nbr = nullptr;            // A* neighbour masks derived from master
  // Robot radius of the grid A* (rna_astar_set_robot_radius, footprint.hip): 0 = point robot (the masks come from
  // nbr_mask_tiles_kernel / compose_nbr_tiles_kernel exactly as before); > 0 = the masks are built from the blocked set
  // of GlobalPlanner::ifBlocked with this radius by footprint_tiles_kernel.
  double robot_r = 0.0;
  unsigned long long* fp_bits = nullptr;       // r > 0: blocked set, 64 x 64 bits per MAP-space tile (word = row j, bit = i)
  rna::FootprintPlan fp{};           // r > 0: the disc stencil, classified for the geometry's coordinate magnitude
  int2* fp_ties = nullptr;           // r > 0: the tie offsets of fp (device)
  int fp_ties_cap = 0;
  rna::GoalField gfield;
  rna::Clearance clearance;
  rna::Frontiers frontiers;
  bool shortcut_lds_raised = false;   // shortcut.hip: the kernels' dynamic-LDS limit has been raised to 160 KiB on this engine's device
  rna::HimmScratch himm;
  rna::VfhDevice vfh;
  rna::AstarDevice astar;
  int profiling = 0;                // 0 off, 1 every kernel slot, 2 only the slots of the A* pipeline stages' own streams
  rna::ProfSlot prof[RNA_K_COUNT];
  std::vector<hipEvent_t> free_events;   // recycled hipEvents of the profiler
  size_t pending_events = 0;
  std::string err;
};

namespace rna {

inline int fail(rna_engine* e, int code, const std::string& msg) {
  if (e) e->err = msg;
  return code;
}

#define RNA_HIP(e, call)                                                                      \
  do {                                                                                        \
    hipError_t _st = (call);                                                                  \
    if (_st != hipSuccess)                                                                    \
      return ::rna::fail((e), RNA_EHIP, std::string(#call) + ": " + hipGetErrorString(_st)); \
  } while (0)

// Profiling (rna_profile_enable): every launch of a tracked kernel is bracketed by two hipEvents
// recorded on the engine stream WITHOUT a host sync; rna_profile_get() drains them.  The timed loop
// of bench.py therefore measures kernels live at negligible cost.
int profile_flush(rna_engine* e);

struct KernelTimer {
  rna_engine* e;
  int id;
  hipEvent_t a = nullptr, b = nullptr;
  static hipEvent_t take(rna_engine* e) {
    hipEvent_t ev = nullptr;
    if (!e->free_events.empty()) { ev = e->free_events.back(); e->free_events.pop_back(); }
    else if (hipEventCreate(&ev) != hipSuccess) ev = nullptr;
    return ev;
  }
  hipStream_t st;
  KernelTimer(rna_engine* eng, int kid, hipStream_t stream = nullptr) : e(eng), id(kid), st(stream ? stream : eng->stream) {
    if (!wanted()) return;
    if (e->pending_events > 16384) (void)profile_flush(e);
    a = take(e);
    b = take(e);
    if (a) (void)hipEventRecord(a, st);
  }
  // mode 2: only the search and the launch-order kernel (stage / side stream).  An event record is a barrier packet of its own: on the
  // engine stream, whose chain of short kernels gates the next batch, the brackets of ten kernel slots cost ~1 ms per pass
  bool wanted() const { return e->profiling == 1 || (e->profiling == 2 && (id == RNA_K_ASTAR_SEARCH || id == RNA_K_ASTAR_RESET)); }
  ~KernelTimer() {
    if (!wanted() || !a || !b) return;
    (void)hipEventRecord(b, st);
    e->prof[id].pending.emplace_back(a, b);
    e->pending_events += 2;
  }
};

// A refused hipMalloc is RNA_ENOMEM, and its HIP error is consumed: left behind, it would be what the thread's next launch
// check (hipGetLastError) reports.
template <typename T>
inline int dev_alloc(rna_engine* e, T** p, size_t n) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (n == 0) return RNA_OK;
  hipError_t st = hipMalloc((void**)p, n * sizeof(T));
  if (st != hipSuccess) {
    *p = nullptr;
    (void)hipGetLastError();
    return fail(e, RNA_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(st));
  }
  return RNA_OK;
}

template <typename T>
inline void dev_free(T** p) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
}

// The device temporaries of ONE C-ABI call (`who`, for the messages) that takes host pointers, on the engine stream: in()
// uploads, out() registers a download, scratch() only allocates; the caller launches on e->stream and returns finish().
// The first failure latches: later in / out / scratch calls enqueue nothing and return nullptr, and finish() reports it
// -- RNA_ENOMEM for a refused allocation (as dev_alloc, its HIP error consumed), RNA_EHIP for anything else -- with e->err
// set.  Plain hipMalloc / hipFree per call, freed by the destructor once the stream has drained (kernels and copies in
// flight read and write the buffers).
class Staging {
 public:
  Staging(rna_engine* e, const char* who) : e_(e), who_(who) {}
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  ~Staging() {
    if (!bufs_.empty() && !drained_) (void)hipStreamSynchronize(e_->stream);
    for (void* p : bufs_) (void)hipFree(p);
  }
  bool ok() const { return rc_ == RNA_OK; }
  // n == 0 still yields a valid pointer (the kernels' device forms reject NULL)
  template <typename T>
  T* scratch(size_t n) {
    if (!ok()) return nullptr;
    void* p = nullptr;
    if (!hip(hipMalloc(&p, (n ? n : 1) * sizeof(T)), "hipMalloc", RNA_ENOMEM)) {
      (void)hipGetLastError();
      return nullptr;
    }
    bufs_.push_back(p);
    return static_cast<T*>(p);
  }
  template <typename T>
  T* in(const T* host, size_t n) {
    T* d = scratch<T>(n);
    // (pageable host memory: the copy has left the caller's array when the call returns)
    if (d && n) hip(hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, e_->stream), "upload");
    return ok() ? d : nullptr;
  }
  // finish() copies the n elements to host; zero: the buffer is cleared on the stream first
  template <typename T>
  T* out(T* host, size_t n, bool zero = false) {
    T* d = scratch<T>(n);
    if (d && n && zero) hip(hipMemsetAsync(d, 0, n * sizeof(T), e_->stream), "clear");
    if (!ok()) return nullptr;
    if (n) downloads_.push_back(Download{host, d, n * sizeof(T)});
    return d;
  }
  // in() and out() on one buffer: what the kernel does not write comes back as the caller had it
  template <typename T>
  T* inout(T* host, size_t n) {
    T* d = in(host, n);
    if (d && n) downloads_.push_back(Download{host, d, n * sizeof(T)});
    return d;
  }
  // The launch check, the registered downloads, the stream synchronisation.  A call that staged nothing (the _device form
  // of an entry point that has both) stops after the launch check: it has no temporaries to outlive.
  int finish() {
    if (ok()) hip(hipGetLastError(), "launch");
    if (bufs_.empty()) return rc_;
    for (const Download& d : downloads_)
      if (ok()) hip(hipMemcpyAsync(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost, e_->stream), "download");
    if (ok()) {
      hip(hipStreamSynchronize(e_->stream), "synchronize");
      drained_ = ok();
    }
    return rc_;
  }

 private:
  struct Download { void* host; const void* dev; size_t bytes; };
  bool hip(hipError_t st, const char* what, int code = RNA_EHIP) {
    if (st != hipSuccess && ok()) rc_ = fail(e_, code, std::string(who_) + ": " + what + ": " + hipGetErrorString(st));
    return st == hipSuccess;
  }
  rna_engine* e_;
  const char* who_;
  int rc_ = RNA_OK;
  bool drained_ = false;
  std::vector<void*> bufs_;
  std::vector<Download> downloads_;
};

template <typename T>
int CtlPair<T>::alloc(rna_engine* e) {
  const int rc = dev_alloc(e, &dev, 1);
  if (rc != RNA_OK) return rc;
  if (hipHostMalloc((void**)&host, sizeof(T)) == hipSuccess) return RNA_OK;
  host = nullptr;
  (void)hipGetLastError();
  return fail(e, RNA_ENOMEM, "hipHostMalloc failed");
}
template <typename T>
void CtlPair<T>::release() {
  dev_free(&dev);
  if (host) { (void)hipHostFree(host); host = nullptr; }
}
template <typename T>
int CtlPair<T>::read(rna_engine* e) {
  RNA_HIP(e, hipGetLastError());
  RNA_HIP(e, hipMemcpyAsync(host, dev, sizeof(T), hipMemcpyDeviceToHost, e->stream));
  RNA_HIP(e, hipStreamSynchronize(e->stream));
  return RNA_OK;
}

// the engine stream waits for the side work in flight (see rna_engine::vfh_stream); cheap when there is none
int side_join(rna_engine* e);
// the side stream (created on first use)
int side_stream(rna_engine* e, hipStream_t* out);
// grid A*: second pass over the searches of finished batches that ran out of pages (astar.hip)
int astar_settle(rna_engine* e);
// entry of a C-ABI call that enqueues on the engine stream: select the device, join the side work.  Calls that cannot
// disturb it (the ray batch of the laser layer, the searches, the VFH+ step itself, getters) use RNA_ENTER_NOJOIN.
#define RNA_ENTER(e)                                        \
  do {                                                      \
    RNA_HIP(e, hipSetDevice((e)->device));                  \
    const int rc_join_ = rna::side_join(e);                 \
    if (rc_join_ != RNA_OK) return rc_join_;                \
  } while (0)
#define RNA_ENTER_NOJOIN(e) RNA_HIP(e, hipSetDevice((e)->device))

// module entry points used across translation units
int himm_release(rna_engine* e);
int vfh_release(rna_engine* e);
int astar_release(rna_engine* e);
int map_prepare_nbr(rna_engine* e);   // make e->nbr consistent with the master layer
// robot radius > 0 (footprint.hip): blocked set + neighbour masks of every tile (all != 0) or of the tiles that are dirty
// or touch a dirty tile (unmoved map), on the engine stream -- the r > 0 replacement of nbr_mask_tiles_kernel
int footprint_refresh(rna_engine* e, int all);
int footprint_release(rna_engine* e);
int goal_field_release(rna_engine* e);
// clearance field of the current masks capped at R cells, enqueued on the engine stream (clearance.hip)
int clearance_refresh(rna_engine* e, int R);
int clearance_release(rna_engine* e);
int frontiers_release(rna_engine* e);
int sync_all(rna_engine* e);          // main stream + every A* side stream
// tile-synchronous A* (astar_tile.hip)
bool tsa_supported(const rna_engine* e);
int tsa_tiles(const rna_engine* e);                                   // 64 x 16 tiles of the map
constexpr int TSA_RETRY = 8;                                          // full-size retry slots per stage
// sizes at e->astar's max_queries and page_cap: a stage's page pool and its block (must start zeroed), the same of its retry slots, a ring entry
size_t tsa_pool_bytes(int max_queries, int cap);
size_t tsa_stage_bytes(const rna_engine* e);
size_t tsa_retry_pool_bytes(const rna_engine* e);
size_t tsa_retry_bytes(const rna_engine* e);
size_t tsa_ring_bytes(const rna_engine* e);
int tsa_stage_prepare(rna_engine* e, int d);                          // fresh stage: page 0 of every slot "unreached"
int tsa_retry_prepare(rna_engine* e, int d);
// A batch on stage d, three launches on the streams the caller hands in (astar.hip orders them with its events): the mask
// snapshot and the launch order go into ring entry `ring`, or into the stage's own block if ring < 0; the search reads them there.
int tsa_snapshot(rna_engine* e, int d, int ring, hipStream_t st);
int tsa_order(rna_engine* e, int d, int ring, hipStream_t st, const rna_astar_query* q_dev, int n);
int tsa_search(rna_engine* e, int d, int ring, hipStream_t st, const rna_astar_query* q_dev, int n, int32_t* paths_dev, int max_len,
               rna_astar_result* res_dev);
int* tsa_retry_count(const rna_engine* e, int d);   // device int: searches of the stage's batch that ended with status 5
int tsa_retry_launch(rna_engine* e, int d, hipStream_t st, int count);   // second pass over `count` listed searches
int tsa_settled(rna_engine* e, int d, const rna_astar_query* q, const rna_astar_result* r, int n, int32_t* d_counts);
int tsa_counters_read(rna_engine* e, unsigned long long* out, bool reset);   // sums the job counters of every stage view into out[16]

}  // namespace rna
