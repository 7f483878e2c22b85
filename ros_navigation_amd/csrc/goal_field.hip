// goal_field.hip -- the goal distance field of the grid A*: one sweep from the goal serves every start.
// What navfn / global_planner offer on a ROS stack and the reference's replan loop would use (Nav::loopPlan replans to
// the same clicked goal while the robot moves, mc/src/nav_node.cpp:103-154): the exact 1000 / 1414 integer cost-to-goal
// of every cell under the grid A* contract (oracle/astar.c), and plans from any start as a walk downhill.
//
// The field is the least fixpoint of field[c] = min over the neighbours n that c's mask allows of field[n] + w(n, c) with
// field[goal] = 0.  It is unique, so any relaxation order gives the same bits; the kernels below only decide how much
// work is redone:
//   gf_init_kernel / gf_seed_kernel   every cell unreached, every source its start cost (the goal 0), the sources' tiles and
//                       their rings pending
//   gf_round_kernel     one launch = one round: a workgroup per 64 x 64 MAP-space tile; a pending tile loads its field with
//                       a one-cell halo and its masks into LDS, relaxes there until nothing changes, stores what fell and
//                       posts the smallest improved value of each of its eight borders as the neighbour tile's pending key
//                       FOR THE NEXT LAUNCH.  No workgroup waits for another: whatever a tile reads of a neighbour that is
//                       being written in the same launch is a valid upper bound, and the neighbour's post makes the tile
//                       run again after the launch boundary.  Tiles whose key lies `width` above the smallest pending key
//                       are put off (the search kernel's f-buckets one level up); width 0 = every pending tile every round.
//   gf_terminal_kernel  per source: the source whose start cost IS its cell's field value marks the cell a terminal
//   gf_finalize_kernel  per reached tile: the canonical step of every cell (`next`, the oracle's backtrace rule run over a
//                       field rooted at the goal), reached cells, largest distance, terminals
//   gf_paths_kernel     one wavefront per start: follows `next` tile by tile through LDS, writes the path start first
// Clearance cost (rna_goal_field_set_clearance_cost): with a table set the fixpoint is field[c] = pen[c] + min(field[n] + w),
// pen[c] the table's cost for c's clearance (clearance.hip) -- a non-negative integer per cell, so the least fixpoint is
// still unique and the same relaxation finds it.  gf_round_kernel<true> / gf_finalize_kernel<true> are that build; the
// <false> instantiations are the table-free kernels: no penalty load, no extra LDS, the same sweeps as before the table existed.
// Termination is the host's: it enqueues rounds in chunks, reads the pending count back and stops at zero (rna_goal_field_build).
// A field is a snapshot: the kernels read the live masks only during the build; paths follow the stored `next` bytes.
// Many sources (rna_goal_field_build_multi): the same least fixpoint with a virtual super-source that reaches source k at
// its start cost seed[k]; the round kernel does not know the difference.  A source cell that a cheaper arrival undercuts is an
// ordinary cell; the others are the terminals (next == 8) the downhill walks end at.
// Owner labels (RNA_GOAL_FIELD_OWNERS): which source the walk along `next` from a cell ends at.  `next` is a forest (the field
// strictly decreases along it), so this is pointer jumping, in two levels:
//   gf_owner_tile_kernel   per relaxed tile: the successors inside the tile in LDS, doubled until every cell points at the
//                       cell of its walk that is a terminal or leaves the tile; stores the terminal's source or the first cell
//                       outside the tile (the EXIT, encoded below -1)
//   gf_owner_jump_kernel   global rounds: an unresolved cell takes its exit's word -- the owner when the exit is resolved, the
//                       exit's exit otherwise: chains halve per round.  Only cells on a tile's border can be exits, so the
//                       rounds run over those; one last launch over every cell resolves the interior.
#include "engine.hpp"
#include "map_tiles_dev.hpp"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <vector>

using namespace rna;

namespace {

constexpr int GF_INF = RNA_GOAL_FIELD_UNREACHED;
constexpr int GF_FAR = RNA_GOAL_FIELD_FAR;
constexpr unsigned GF_LIMIT = 1u << 30;   // the search's own 30-bit g range (rna.h, status 4)
constexpr int GF_W = TILE + 2;            // a tile with its halo: cells per row / rows
constexpr int GF_S = GF_W + 1;            // LDS row stride (odd: lanes along i AND lanes along j hit distinct banks)
constexpr uint8_t GF_NEXT_GOAL = 8, GF_NEXT_FAR = 254, GF_NEXT_NONE = 255;
constexpr unsigned GF_DEFAULT_WIDTH = 256000;   // see gf_width(): four tiles' worth of cost; 0 / 128 k / 256 k / 512 k measured
constexpr int GF_CHUNK = 32;              // rounds enqueued between two looks at the pending count
constexpr int GF_OWNER_SLOTS = 36;        // jump rounds of the owner pass: ceil(log2 cells) + 1 <= 32 (cells <= 2e9)
constexpr int GF_OWNER_CHUNK = 8;         // jump rounds enqueued between two looks at the unresolved count
constexpr int GF_PS = TILE + 1;           // clearance cost of the tile's cells in LDS, uint16: row stride (odd, in halfwords: lanes
                                          // along j fall into distinct banks as lanes along i do)

// Rotating per-round control words: round r reads slot (r + 2) % 3 (what round r - 1 posted), posts into slot r % 3 and
// clears slot (r + 1) % 3 for round r + 1.
struct GfRound {
  int pending;    // posts for the next round (wakes + put-off tiles); 0 = the field is complete
  int min_key;    // smallest key among them
  int pad[2];
};
struct GfCtl {
  GfRound round[3];
  int status;          // 0, or 2: the goal cell is blocked
  int rounds;          // rounds that found something pending
  int tile_jobs;       // tile relaxations run
  int reached, max_cost, tiles_reached;
  int passes, max_passes;   // relaxation passes over a tile in LDS: all jobs, the longest job (RNA_GOAL_FIELD_STATS)
  int goal0;           // goals[0] as the seed kernel read it (the device form's info.goal)
  int blocked_sources; // sources skipped: their cell is in the blocked set
  int invalid_sources; // sources with a cell outside the map or a start cost outside [0, 2^30): the build fails
  int terminals;       // cells with next == 8
  int own_unres[GF_OWNER_SLOTS];   // owner pass: cells a jump round left unresolved, per round
};

// A source as the seed and the terminal kernel see it: 0 usable, 1 blocked, 2 invalid.  goals == nullptr: the one source
// goal0 with start cost 0 (rna_goal_field_build).
__device__ __forceinline__ int gf_source(const int32_t* __restrict__ goals, const int32_t* __restrict__ seed, int k, int goal0, int rows,
                                         int cols, int tiles_i, int s0, int s1, const float* __restrict__ master,
                                         const unsigned long long* __restrict__ bits, int& g, int& s, int& i, int& j) {
  g = goals ? goals[k] : goal0;
  s = seed ? seed[k] : 0;
  if (g < 0 || (long long)g >= (long long)rows * cols || (unsigned)s >= GF_LIMIT) return 2;
  map_cell_of(g, rows, cols, s0, s1, i, j);
  return (bits ? fp_bit(bits, tiles_i, cols, i, j) : cell_blocked(master[g])) ? 1 : 0;
}

// owner words: >= 0 the source, -1 no owner (unreached, far), <= -2 unresolved: the walk goes on at buffer cell -(word + 2)
__device__ __forceinline__ int gf_exit_word(int cell) { return -cell - 2; }

// fn + w with the 30-bit rule: a sum at or beyond 2^30 is FAR, FAR stays FAR, unreached stays unreached
__device__ __forceinline__ int gf_add(int fn, int w) {
  const unsigned s = (unsigned)fn + (unsigned)w;
  return s < GF_LIMIT ? (int)s : (fn == GF_INF ? GF_INF : GF_FAR);
}

// the tile's field with a one-cell halo (outside the map: unreached) -> F[GF_W rows of stride GF_S]
__device__ __forceinline__ void gf_load_field(int* F, const int32_t* __restrict__ field, int i0, int j0, int rows, int cols, int s0,
                                              int s1) {
  for (int k = threadIdx.x; k < GF_W * GF_W; k += blockDim.x) {
    const int ii = k % GF_W, jj = k / GF_W;
    const int i = i0 - 1 + ii, j = j0 - 1 + jj;
    int v = GF_INF;
    if (i >= 0 && j >= 0 && i < rows && j < cols) v = field[buffer_lin(i, j, rows, cols, s0, s1)];
    F[jj * GF_S + ii] = v;
  }
}

// the tile's masks twice: M[lj][li] for the sweeps with lanes along i, MT[li][lj] for the sweeps with lanes along j
__device__ __forceinline__ void gf_load_masks(uint8_t* M, uint8_t* MT, const uint8_t* __restrict__ nbr, int i0, int j0, int rows, int cols,
                                              int s0, int s1) {
  for (int k = threadIdx.x; k < TILE * TILE; k += blockDim.x) {
    const int li = k & (TILE - 1), lj = k >> 6;
    const int i = i0 + li, j = j0 + lj;
    const uint8_t m = (i < rows && j < cols) ? nbr[buffer_lin(i, j, rows, cols, s0, s1)] : (uint8_t)0;
    M[k] = m;
    MT[li * TILE + lj] = m;
  }
}

// one relaxation of tile cell (li, lj), mask m, against its neighbours among DIRS (bit k = neighbour k); 1 when the cell fell.
// The loads are unconditional (the halo makes every address valid): one LDS round trip per step, not one per neighbour.
// pen: the cell's clearance cost, paid on entering it (0 without a table).
template <unsigned DIRS>
__device__ __forceinline__ int gf_relax(int* F, unsigned m, int li, int lj, int pen) {
  m &= DIRS;
  if (!m) return 0;
  int* c = &F[(lj + 1) * GF_S + li + 1];
  const int cur = *c;
  const int v0 = (DIRS & 1u) ? c[-GF_S - 1] : 0, v1 = (DIRS & 2u) ? c[-GF_S] : 0, v2 = (DIRS & 4u) ? c[-GF_S + 1] : 0;
  const int v3 = (DIRS & 8u) ? c[-1] : 0, v4 = (DIRS & 16u) ? c[1] : 0;
  const int v5 = (DIRS & 32u) ? c[GF_S - 1] : 0, v6 = (DIRS & 64u) ? c[GF_S] : 0, v7 = (DIRS & 128u) ? c[GF_S + 1] : 0;
  int best = cur;
  if (DIRS & 1u) best = min(best, (m & 1u) ? gf_add(v0, 1414 + pen) : GF_INF);
  if (DIRS & 2u) best = min(best, (m & 2u) ? gf_add(v1, 1000 + pen) : GF_INF);
  if (DIRS & 4u) best = min(best, (m & 4u) ? gf_add(v2, 1414 + pen) : GF_INF);
  if (DIRS & 8u) best = min(best, (m & 8u) ? gf_add(v3, 1000 + pen) : GF_INF);
  if (DIRS & 16u) best = min(best, (m & 16u) ? gf_add(v4, 1000 + pen) : GF_INF);
  if (DIRS & 32u) best = min(best, (m & 32u) ? gf_add(v5, 1414 + pen) : GF_INF);
  if (DIRS & 64u) best = min(best, (m & 64u) ? gf_add(v6, 1000 + pen) : GF_INF);
  if (DIRS & 128u) best = min(best, (m & 128u) ? gf_add(v7, 1414 + pen) : GF_INF);
  if (best < cur) { *c = best; return 1; }
  return 0;
}

// the clearance cost of a cell: the table by squared clearance, 0 beyond its last entry (RNA_CLEARANCE_NONE included)
__device__ __forceinline__ int gf_pen(const uint16_t* __restrict__ clr, const uint16_t* __restrict__ pen_tab, int pen_r2, size_t b) {
  const int c = clr[b];
  return c <= pen_r2 ? (int)pen_tab[c] : 0;
}

}  // namespace

__global__ void gf_init_kernel(int32_t* __restrict__ field, uint8_t* __restrict__ next, size_t ncell, int* __restrict__ keys,
                               uint8_t* __restrict__ touched, int ntile, GfCtl* __restrict__ ctl, int32_t* __restrict__ owner) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < ncell; k += stride) {
    field[k] = GF_INF;
    next[k] = GF_NEXT_NONE;
    if (owner) owner[k] = -1;   // (also the largest unsigned: gf_terminal_kernel takes the smallest source with atomicMin)
  }
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < (size_t)ntile; k += stride) {
    keys[k] = GF_INF;
    keys[ntile + k] = GF_INF;
    touched[k] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // the control words; round 0 reads slot 2: the seed kernel posts there
    GfCtl c = {};
    c.round[0].min_key = c.round[1].min_key = c.round[2].min_key = GF_INF;
    c.goal0 = -1;
    *ctl = c;
  }
}

// One thread per source.  A source whose cell is blocked (robot radius: the footprint's blocked set, else the master layer's
// own predicate) or invalid is counted and skipped; every other one lowers field[goal] to its start cost and makes the goal's
// tile and its ring pending for round 0 with that key.  Everything is a minimum: the order of the sources does not matter.
__global__ void __launch_bounds__(256) gf_seed_kernel(int32_t* __restrict__ field, int* __restrict__ keys, GfCtl* __restrict__ ctl,
                                                      const int32_t* __restrict__ goals, const int32_t* __restrict__ seed, int n, int goal0,
                                                      int rows, int cols, int tiles_i, int s0, int s1, const float* __restrict__ master,
                                                      const unsigned long long* __restrict__ bits) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  int g, s, i, j;
  const int kind = gf_source(goals, seed, k, goal0, rows, cols, tiles_i, s0, s1, master, bits, g, s, i, j);
  if (k == 0) ctl->goal0 = g;
  if (kind == 2) { atomicAdd(&ctl->invalid_sources, 1); return; }
  if (kind == 1) { atomicAdd(&ctl->blocked_sources, 1); return; }
  // the start cost is stored here, not by a tile job, so no job would post it to a neighbour tile when the source lies on
  // its tile's border (and its neighbours inside the tile are blocked): the ring is made pending with the same key
  atomicMin(&field[g], s);
  const int tiles_j = (cols + TILE - 1) / TILE;
  for (int b = j / TILE - 1; b <= j / TILE + 1; ++b)
    for (int a = i / TILE - 1; a <= i / TILE + 1; ++a)
      if (a >= 0 && b >= 0 && a < tiles_i && b < tiles_j) atomicMin(&keys[b * tiles_i + a], s);
  atomicMin(&ctl->round[2].min_key, s);
  atomicAdd(&ctl->round[2].pending, 1);
}

// One thread per source, after the last round: source k is a terminal's source iff seed[k] == field[goals[k]] (a tie with an
// arrival through a neighbour goes to the terminal).  The mark is the cell's `next` byte, which nothing else has written since
// gf_init_kernel; gf_finalize_kernel keeps it.  With owner labels the cell also takes the smallest such k.
__global__ void __launch_bounds__(256) gf_terminal_kernel(const int32_t* __restrict__ field, uint8_t* __restrict__ next,
                                                          int32_t* __restrict__ owner, const int32_t* __restrict__ goals,
                                                          const int32_t* __restrict__ seed, int n, int goal0, int rows, int cols, int tiles_i,
                                                          int s0, int s1, const float* __restrict__ master,
                                                          const unsigned long long* __restrict__ bits) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  int g, s, i, j;
  if (gf_source(goals, seed, k, goal0, rows, cols, tiles_i, s0, s1, master, bits, g, s, i, j) != 0) return;
  if (field[g] != s) return;
  next[g] = GF_NEXT_GOAL;   // (every writer stores the same byte)
  if (owner) atomicMin(reinterpret_cast<unsigned*>(&owner[g]), (unsigned)k);
}

// One relaxation round (see the head of the file).  Grid = tiles of the map in MAP space, 256 threads.  A pass over the tile
// in LDS is four directional sweeps: lanes along i, wavefront w sweeping its band of rows 16 w .. 16 w + 15 down (relaxing
// against the row above and the own row) and up; then lanes along j, wavefront w sweeping its band of columns right and
// left.  A value travels a whole band per pass in each of the eight directions (with the j sweeps alone a straight run along i
// advanced two cells per pass: 107 ms per build at 4096^2 instead of the figure in DESIGN.md).  Inside a sweep a cell is
// written by its owner thread only, reads of cells another wavefront is writing see an earlier or a later valid bound; the
// two lane layouts are separated by barriers.  Passes repeat until one changes nothing.
// PEN: the clearance cost of the tile's cells (clr -> pen_tab, see gf_pen) sits in LDS next to the masks, one uint16 layout
// that both lane orders read without bank conflicts; without PEN the three last arguments are not read.
template <bool PEN>
__global__ void __launch_bounds__(256) gf_round_kernel(int32_t* __restrict__ field, const uint8_t* __restrict__ nbr, int* __restrict__ keys,
                                                       uint8_t* __restrict__ touched, GfCtl* __restrict__ ctl, int round, unsigned width,
                                                       int rows, int cols, int s0, int s1, const uint16_t* __restrict__ clr,
                                                       const uint16_t* __restrict__ pen_tab, int pen_r2) {
  __shared__ int F[GF_W * GF_S];
  __shared__ uint8_t M[TILE * TILE], MT[TILE * TILE];
  __shared__ uint16_t P[PEN ? TILE * GF_PS : 1];
  __shared__ int wake[8];
  const int tiles_i = gridDim.x, tiles_j = gridDim.y, ntile = tiles_i * tiles_j;
  const int ti = blockIdx.x, tj = blockIdx.y, t = tj * tiles_i + ti;
  const GfRound prev = ctl->round[(round + 2) % 3];
  GfRound* cur = &ctl->round[round % 3];
  if (t == 0 && threadIdx.x == 0) {
    GfRound* nx = &ctl->round[(round + 1) % 3];
    nx->pending = 0;
    nx->min_key = GF_INF;
    if (prev.pending) ctl->rounds += 1;
  }
  if (!prev.pending) return;
  int* key_cur = keys + (round & 1) * ntile;
  int* key_nxt = keys + ((round + 1) & 1) * ntile;
  const int key = key_cur[t];   // (posted by earlier launches only)
  if (key == GF_INF) return;
  __syncthreads();              // every thread has read the key before it is cleared
  if (threadIdx.x == 0) key_cur[t] = GF_INF;
  if (width && key > prev.min_key && (unsigned)key >= (unsigned)prev.min_key + width) {
    // put off: the tile stays pending with its key (the tile holding the smallest key always runs)
    if (threadIdx.x == 0) {
      atomicMin(&key_nxt[t], key);
      atomicMin(&cur->min_key, key);
      atomicAdd(&cur->pending, 1);
    }
    return;
  }
  const int i0 = ti * TILE, j0 = tj * TILE;
  gf_load_field(F, field, i0, j0, rows, cols, s0, s1);
  gf_load_masks(M, MT, nbr, i0, j0, rows, cols, s0, s1);
  if (PEN) {
    for (int k = threadIdx.x; k < TILE * TILE; k += blockDim.x) {
      const int pi = k & (TILE - 1), pj = k >> 6;
      const int i = i0 + pi, j = j0 + pj;
      P[pj * GF_PS + pi] = (i < rows && j < cols) ? (uint16_t)gf_pen(clr, pen_tab, pen_r2, buffer_lin(i, j, rows, cols, s0, s1)) : (uint16_t)0;
    }
  }
  if (threadIdx.x < 8) wake[threadIdx.x] = GF_INF;
  if (threadIdx.x == 0) {
    touched[t] = 1;
    atomicAdd(&ctl->tile_jobs, 1);
  }
  __syncthreads();
  const int li = threadIdx.x & 63, band = (threadIdx.x >> 6) * 16;
  int changed, passes = 0;
  do {
    changed = 0;
    ++passes;
#pragma unroll 1
    for (int s = 0; s < 16; ++s) changed |= gf_relax<0x1Fu>(F, M[(band + s) * TILE + li], li, band + s, PEN ? P[(band + s) * GF_PS + li] : 0);        // down: dj = -1, 0
#pragma unroll 1
    for (int s = 15; s >= 0; --s) changed |= gf_relax<0xF8u>(F, M[(band + s) * TILE + li], li, band + s, PEN ? P[(band + s) * GF_PS + li] : 0);      // up: dj = 1, 0
    __syncthreads();
    // (li is this thread's j here)
#pragma unroll 1
    for (int s = 0; s < 16; ++s) changed |= gf_relax<0x6Bu>(F, MT[(band + s) * TILE + li], band + s, li, PEN ? P[li * GF_PS + band + s] : 0);       // right: di = -1, 0
#pragma unroll 1
    for (int s = 15; s >= 0; --s) changed |= gf_relax<0xD6u>(F, MT[(band + s) * TILE + li], band + s, li, PEN ? P[li * GF_PS + band + s] : 0);     // left: di = 1, 0
  } while (__syncthreads_or(changed));
  if (threadIdx.x == 0) {
    atomicAdd(&ctl->passes, passes);
    atomicMax(&ctl->max_passes, passes);
  }
  // store what fell; the smallest improved value on each border is the neighbour tile's key
  int w[8] = {GF_INF, GF_INF, GF_INF, GF_INF, GF_INF, GF_INF, GF_INF, GF_INF};
  const int i = i0 + li;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int lj = band + s, j = j0 + lj;
    if (i >= rows || j >= cols) continue;
    const int v = F[(lj + 1) * GF_S + li + 1];
    int32_t* p = &field[buffer_lin(i, j, rows, cols, s0, s1)];
    if (v < *p) {
      *p = v;
      const bool up = li == 0, dn = li == TILE - 1, lf = lj == 0, rt = lj == TILE - 1;
      if (lf && up) w[0] = min(w[0], v);
      if (lf) w[1] = min(w[1], v);
      if (lf && dn) w[2] = min(w[2], v);
      if (up) w[3] = min(w[3], v);
      if (dn) w[4] = min(w[4], v);
      if (rt && up) w[5] = min(w[5], v);
      if (rt) w[6] = min(w[6], v);
      if (rt && dn) w[7] = min(w[7], v);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (w[k] != GF_INF) atomicMin(&wake[k], w[k]);
  __threadfence();
  __syncthreads();
  if (threadIdx.x < 8) {
    const int k = threadIdx.x, v = wake[k];
    const int a = ti + nbr_di(k), b = tj + nbr_dj(k);
    if (v != GF_INF && a >= 0 && b >= 0 && a < tiles_i && b < tiles_j) {
      atomicMin(&key_nxt[b * tiles_i + a], v);
      atomicMin(&cur->min_key, v);
      atomicAdd(&cur->pending, 1);
    }
  }
}

// The canonical step of every cell of a tile that was relaxed: the first neighbour k of the cell's mask (fixed order = lowest
// map-space linear index first) with field[n] + w == field[c] -- oracle/astar.c's backtrace rule over a field rooted at
// the goal; a cell gf_terminal_kernel marked (its `next` byte, read before it is written) is a terminal and keeps its 8.
// Also the build's totals.  PEN: field[n] + w + the cell's own clearance cost == field[c].
template <bool PEN>
__global__ void __launch_bounds__(256) gf_finalize_kernel(const int32_t* __restrict__ field, const uint8_t* __restrict__ nbr,
                                                          uint8_t* __restrict__ next, const uint8_t* __restrict__ touched,
                                                          GfCtl* __restrict__ ctl, int rows, int cols, int s0, int s1,
                                                          const uint16_t* __restrict__ clr, const uint16_t* __restrict__ pen_tab, int pen_r2) {
  __shared__ int F[GF_W * GF_S];
  __shared__ int tot[3];
  const int tiles_i = gridDim.x;
  const int ti = blockIdx.x, tj = blockIdx.y, t = tj * tiles_i + ti;
  if (!touched[t]) return;
  const int i0 = ti * TILE, j0 = tj * TILE;
  gf_load_field(F, field, i0, j0, rows, cols, s0, s1);
  if (threadIdx.x < 3) tot[threadIdx.x] = 0;
  __syncthreads();
  int n_reached = 0, v_max = 0, n_term = 0;
  for (int k = threadIdx.x; k < TILE * TILE; k += blockDim.x) {
    const int li = k & (TILE - 1), lj = k >> 6;
    const int i = i0 + li, j = j0 + lj;
    if (i >= rows || j >= cols) continue;
    const size_t b = buffer_lin(i, j, rows, cols, s0, s1);
    const int* c = &F[(lj + 1) * GF_S + li + 1];
    const int v = *c;
    uint8_t nx = GF_NEXT_NONE;
    if (v == GF_FAR) nx = GF_NEXT_FAR;
    else if ((unsigned)v < GF_LIMIT) {
      ++n_reached;
      v_max = max(v_max, v);
      if (next[b] == GF_NEXT_GOAL) { nx = GF_NEXT_GOAL; ++n_term; }
      else {
        const unsigned m = nbr[b];
        const int pen = PEN ? gf_pen(clr, pen_tab, pen_r2, b) : 0;
        const int off[8] = {-GF_S - 1, -GF_S, -GF_S + 1, -1, 1, GF_S - 1, GF_S, GF_S + 1};
        const int wt[8] = {1414, 1000, 1414, 1000, 1000, 1414, 1000, 1414};
#pragma unroll
        for (int q = 7; q >= 0; --q)
          if (((m >> q) & 1u) && (unsigned)c[off[q]] < GF_LIMIT && c[off[q]] + wt[q] + pen == v) nx = (uint8_t)q;
      }
    }
    next[b] = nx;
  }
  if (n_reached) {
    atomicAdd(&tot[0], n_reached);
    atomicMax(&tot[1], v_max);
    if (n_term) atomicAdd(&tot[2], n_term);
  }
  __syncthreads();
  if (threadIdx.x == 0 && tot[0]) {
    atomicAdd(&ctl->reached, tot[0]);
    atomicMax(&ctl->max_cost, tot[1]);
    atomicAdd(&ctl->tiles_reached, 1);
    if (tot[2]) atomicAdd(&ctl->terminals, tot[2]);
  }
}

// Owner labels, level 1.  Grid = tiles of the map in MAP space, 256 threads, a tile that was relaxed only (every other cell
// keeps the -1 of gf_init_kernel).  P: the local index (lj * 64 + li) of a cell's successor inside the tile, or the cell itself
// when its walk ends or leaves here: a terminal, a cell whose step leaves the tile, a cell without a step.  V: what such a
// root stands for -- the terminal's source (left in `owner` by gf_terminal_kernel), the exit, or -1.  Pointer doubling between
// two copies of P (a step reads one and writes the other): after s steps a pointer is 2^s successors ahead or at its root, a
// walk inside a tile has fewer than 4096 steps, so 12 steps reach every root.  A workgroup reads and writes the `owner` words of
// its own tile only.
__global__ void __launch_bounds__(256) gf_owner_tile_kernel(const uint8_t* __restrict__ next, int32_t* __restrict__ owner,
                                                            const uint8_t* __restrict__ touched, int rows, int cols, int s0, int s1) {
  __shared__ uint16_t P[2][TILE * TILE];
  __shared__ int V[TILE * TILE];
  const int ti = blockIdx.x, tj = blockIdx.y, t = tj * gridDim.x + ti;
  if (!touched[t]) return;
  const int i0 = ti * TILE, j0 = tj * TILE;
  for (int l = threadIdx.x; l < TILE * TILE; l += blockDim.x) {
    const int li = l & (TILE - 1), lj = l >> 6;
    const int i = i0 + li, j = j0 + lj;
    int p = l, v = -1;
    if (i < rows && j < cols) {
      const size_t b = buffer_lin(i, j, rows, cols, s0, s1);
      const int k = next[b];
      if (k == GF_NEXT_GOAL) v = owner[b];
      else if (k < 8) {
        const int ni = li + nbr_di(k), nj = lj + nbr_dj(k);
        if ((unsigned)ni < (unsigned)TILE && (unsigned)nj < (unsigned)TILE) p = nj * TILE + ni;
        else v = gf_exit_word(buffer_lin<int>(i0 + ni, j0 + nj, rows, cols, s0, s1));   // (a step never leaves the map)
      }
    }
    P[0][l] = (uint16_t)p;
    V[l] = v;
  }
  __syncthreads();
  int cur = 0;
  for (int s = 0; s < 12; ++s) {   // bound: see above
    int changed = 0;
    for (int l = threadIdx.x; l < TILE * TILE; l += blockDim.x) {
      const int p = P[cur][l], q = P[cur][p];
      P[cur ^ 1][l] = (uint16_t)q;
      changed |= q != p;
    }
    cur ^= 1;
    if (!__syncthreads_or(changed)) break;
  }
  for (int l = threadIdx.x; l < TILE * TILE; l += blockDim.x) {
    const int i = i0 + (l & (TILE - 1)), j = j0 + (l >> 6);
    if (i < rows && j < cols) owner[buffer_lin(i, j, rows, cols, s0, s1)] = V[P[cur][l]];
  }
}

// Owner labels, level 2: one launch = one round.  An unresolved cell (word <= -2) replaces its word by its exit's word: the
// owner when the exit is resolved, else the exit's own exit.  Every word a cell ever holds is either its walk's owner or a cell
// farther down its walk, whichever launch it was read in -- so the word of an exit that another workgroup is replacing in the
// same launch may be read before or after (one aligned 32-bit word, read and written whole): the result does not depend on
// it, only how far the cell gets in this round, and that is at least as far as with the words the launch started from.  With
// those a chain of d unresolved exits has floor(d / 2) left after a round; d < cells, so ceil(log2 cells) rounds resolve every
// exit.  An exit is the first cell outside a tile, hence on the border of its own tile: ALL == false runs over the border cells
// of the relaxed tiles (252 threads of the 256 have one), ALL == true over every cell once the borders are resolved -- then no
// word that is read is written in the same launch.  Round r counts what it leaves unresolved into own_unres[r] and does
// nothing once the round before it left nothing.
template <bool ALL>
__global__ void __launch_bounds__(256) gf_owner_jump_kernel(int32_t* __restrict__ owner, const uint8_t* __restrict__ touched,
                                                            GfCtl* __restrict__ ctl, int round, int rows, int cols, int s0, int s1) {
  const int ti = blockIdx.x, tj = blockIdx.y, t = tj * gridDim.x + ti;
  if (!touched[t]) return;
  if (!ALL && round > 0 && ctl->own_unres[round - 1] == 0) return;   // (written by earlier launches only)
  const int i0 = ti * TILE, j0 = tj * TILE;
  int left = 0;
  for (int l = threadIdx.x; l < (ALL ? TILE * TILE : 4 * TILE - 4); l += blockDim.x) {
    int li, lj;
    if (ALL) { li = l & (TILE - 1); lj = l >> 6; }
    else if (l < 2 * TILE) { li = l & (TILE - 1); lj = l < TILE ? 0 : TILE - 1; }
    else { li = l < 3 * TILE - 2 ? 0 : TILE - 1; lj = 1 + (l - 2 * TILE) % (TILE - 2); }
    const int i = i0 + li, j = j0 + lj;
    if (i >= rows || j >= cols) continue;
    int32_t* w = &owner[buffer_lin(i, j, rows, cols, s0, s1)];
    const int v = *w;   // (only this thread writes this word)
    if (v > -2) continue;
    const int x = __hip_atomic_load(&owner[-v - 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    left += x <= -2;
  }
  if (left) atomicAdd(&ctl->own_unres[round], left);
}

// One wavefront per start.  The walk is the same in every lane (uniform values): the lanes only share the loads of the
// 64 x 64 tile of `next` bytes the walk is in (LDS, 4 KiB), lane 0 stores the path.  (rows, cols, s0, s1) are the
// geometry the field was built with: cells are buffer linear indices, steps are taken in map space.
__global__ void __launch_bounds__(64) gf_paths_kernel(const int32_t* __restrict__ field, const uint8_t* __restrict__ next,
                                                      const int32_t* __restrict__ starts, int n, int32_t* __restrict__ paths, int max_len,
                                                      rna_astar_result* __restrict__ results, int rows, int cols, int s0, int s1) {
  __shared__ uint8_t T[TILE * TILE];
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q >= n) return;
  const long long ncell = (long long)rows * cols;
  const int s = starts[q];
  rna_astar_result r = {2, 0, GF_INF, 0, 0, 0};
  if (s >= 0 && s < ncell) {
    const int f = field[s];
    r.cost = f;
    if (f == GF_INF) r.status = 1;
    else if (f == GF_FAR) r.status = 4;
    else {
      int i, j;
      map_cell_of(s, rows, cols, s0, s1, i, j);
      int32_t* out = paths + (size_t)q * max_len;
      int len = 0;   // (cells <= 2e9, rna_create)
      bool done = false, broken = false;
      while (!done && !broken) {
        const int i0 = i & ~(TILE - 1), j0 = j & ~(TILE - 1);
        __syncthreads();   // the previous tile's walk is over
        for (int rr = 0; rr < TILE; ++rr) {
          const int ci = i0 + lane, cj = j0 + rr;
          T[rr * TILE + lane] = (ci < rows && cj < cols) ? next[buffer_lin(ci, cj, rows, cols, s0, s1)] : GF_NEXT_NONE;
        }
        __syncthreads();
        while ((i & ~(TILE - 1)) == i0 && (j & ~(TILE - 1)) == j0) {
          if (len < max_len && lane == 0) out[len] = buffer_lin<int>(i, j, rows, cols, s0, s1);
          ++len;
          const int k = __builtin_amdgcn_readfirstlane((int)T[(j - j0) * TILE + (i - i0)]);
          if (k == GF_NEXT_GOAL) { done = true; break; }
          if (k > 7 || len > ncell) { broken = true; break; }   // (cannot happen for a finalized field)
          i += nbr_di(k);
          j += nbr_dj(k);
          if ((unsigned)i >= (unsigned)rows || (unsigned)j >= (unsigned)cols) { broken = true; break; }
        }
      }
      if (broken) { r.status = 1; r.cost = GF_INF; }
      else {
        r.path_len = len;
        r.status = len > max_len ? 3 : 0;
      }
    }
  }
  if (lane == 0) results[q] = r;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace rna {

int goal_field_release(rna_engine* e) {
  GoalField& f = e->gfield;
  dev_free(&f.field);
  dev_free(&f.next);
  dev_free(&f.keys);
  dev_free(&f.touched);
  dev_free(&f.pen);
  dev_free(&f.owner);
  f.sources = rna_goal_field_sources_info{0, 0, 0, 0, 0, {0, 0, 0}};
  f.pen_current = false;
  f.ctl.release();
  f.info = rna_goal_field_info{-1, 0, 0, 0, 0, 0, 0, 0};
  return RNA_OK;
}

}  // namespace rna

namespace {

int gf_alloc(rna_engine* e) {
  GoalField& f = e->gfield;
  if (f.field) return RNA_OK;
  const size_t ntile = (size_t)e->tiles_i * e->tiles_j;
  int rc = dev_alloc(e, &f.field, e->ncell);
  if (rc == RNA_OK) rc = dev_alloc(e, &f.next, e->ncell);
  if (rc == RNA_OK) rc = dev_alloc(e, &f.keys, 2 * ntile);
  if (rc == RNA_OK) rc = dev_alloc(e, &f.touched, ntile);
  if (rc == RNA_OK) rc = f.ctl.alloc(e);
  if (rc != RNA_OK) {
    const std::string msg = e->err;
    goal_field_release(e);
    e->err = msg;
  }
  return rc;
}

// tile keys farther than this above the smallest pending key wait (cost units; 0 = plain rounds).  Developer knob
// RNA_GOAL_FIELD_WIDTH, read at every build; the default is the measured one (profiles/goal_field_rows.json).
unsigned gf_width() {
  const char* v = getenv("RNA_GOAL_FIELD_WIDTH");
  const long long n = v ? atoll(v) : -1;
  return n < 0 ? GF_DEFAULT_WIDTH : (unsigned)std::min<long long>(n, 1 << 30);
}

}  // namespace

namespace {

int gf_log2_ceil(size_t n) {
  int k = 0;
  while (((size_t)1 << k) < n) ++k;
  return k;
}

// The owner pass of a finalized field (see the head of the file), on the engine stream; returns when the labels are complete.
int gf_owners(rna_engine* e, int* rounds_out) {
  GoalField& f = e->gfield;
  GfCtl* const ctl = f.ctl.dev;
  const GfCtl* const host = f.ctl.host;
  const dim3 grid(e->tiles_i, e->tiles_j), block(256);
  int rc;
  hipLaunchKernelGGL(gf_owner_tile_kernel, grid, block, 0, e->stream, f.next, f.owner, f.touched, f.rows, f.cols, f.s0, f.s1);
  // border rounds in chunks until one leaves nothing unresolved: at most ceil(log2 cells) of them (gf_owner_jump_kernel)
  const int cap = std::max(1, gf_log2_ceil(e->ncell));
  int round = 0, clean = -1;
  while (clean < 0) {
    for (int k = 0; k < GF_OWNER_CHUNK && round < cap; ++k, ++round)
      hipLaunchKernelGGL(gf_owner_jump_kernel<false>, grid, block, 0, e->stream, f.owner, f.touched, ctl, round, f.rows, f.cols, f.s0, f.s1);
    if ((rc = f.ctl.read(e)) != RNA_OK) return rc;
    for (int r = 0; r < round && clean < 0; ++r)
      if (host->own_unres[r] == 0) clean = r;
    if (clean < 0 && round >= cap)
      return fail(e, RNA_ECAPACITY, "rna_goal_field_build_multi: the owner pass did not settle within its bound (" + std::to_string(round) +
                                        " rounds)");
  }
  // the gather: every cell, its count goes into the slot behind the border rounds
  const int slot = GF_OWNER_SLOTS - 1;
  hipLaunchKernelGGL(gf_owner_jump_kernel<true>, grid, block, 0, e->stream, f.owner, f.touched, ctl, slot, f.rows, f.cols, f.s0, f.s1);
  if ((rc = f.ctl.read(e)) != RNA_OK) return rc;
  if (host->own_unres[slot] != 0)
    return fail(e, RNA_ECAPACITY, "rna_goal_field_build_multi: the owner pass left " + std::to_string(host->own_unres[slot]) +
                                      " cells unresolved");
  *rounds_out = clean + 2;   // the border rounds up to the first clean one, and the gather
  return RNA_OK;
}

// The build behind both entry points.  goals / seed: DEVICE arrays of n sources (seed may be NULL = all 0), or goals == NULL:
// the one source goal0 with start cost 0.  checked: the host has validated the sources already.
int gf_build(rna_engine* e, const int32_t* goals, const int32_t* seed, int n, int32_t goal0, unsigned flags, rna_goal_field_info* info_host,
             const char* who) {
  int rc = map_prepare_nbr(e);
  if (rc != RNA_OK) return rc;
  if ((rc = gf_alloc(e)) != RNA_OK) return rc;
  GoalField& f = e->gfield;
  const bool owners = (flags & RNA_GOAL_FIELD_OWNERS) != 0;
  if (owners && !f.owner && (rc = dev_alloc(e, &f.owner, e->ncell)) != RNA_OK) return rc;
  // clearance cost: a clearance field of the table's cap for the current masks, and the table by squared clearance
  const bool pen = f.cost_n > 0;
  const int pen_r = f.cost_n - 1, pen_r2 = pen_r * pen_r;
  if (pen) {
    if (e->clearance.R != pen_r || e->clearance.epoch != e->map.epoch)
      if ((rc = clearance_refresh(e, pen_r)) != RNA_OK) return rc;
    if (!f.pen_current) {
      std::vector<uint16_t> tab((size_t)pen_r2 + 1, 0);
      for (int k = 1; k <= pen_r; ++k)
        for (int d2 = k * k; d2 < (k + 1) * (k + 1) && d2 <= pen_r2; ++d2) tab[d2] = f.cost_tab[k];
      // (no kernel in flight reads f.pen: a build returns when it is complete, paths do not use it)
      if ((rc = dev_alloc(e, &f.pen, tab.size())) != RNA_OK) return rc;
      RNA_HIP(e, hipMemcpy(f.pen, tab.data(), tab.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
      f.pen_current = true;
    }
  }
  const Geom& g = e->geom;
  const int rows = g.size[0], cols = g.size[1], s0 = g.start[0], s1 = g.start[1];
  const int ntile = e->tiles_i * e->tiles_j;
  // (no field while this one is being built, also when the build fails from here on; a failure above -- the clearance
  // refresh, the table upload -- leaves the previous field in place: its buffers have not been touched yet)
  f.info.goal = -1;
  f.sources = rna_goal_field_sources_info{0, 0, 0, 0, 0, {0, 0, 0}};
  GfCtl* const ctl = f.ctl.dev;
  const GfCtl* const host = f.ctl.host;
  const float* master = e->layer[RNA_LAYER_MASTER];
  const unsigned long long* bits = e->robot_r > 0.0 ? e->fp_bits : (const unsigned long long*)nullptr;
  const dim3 per_source((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(gf_init_kernel, dim3((unsigned)std::min<size_t>((e->ncell + 255) / 256, 8192)), dim3(256), 0, e->stream, f.field,
                     f.next, e->ncell, f.keys, f.touched, ntile, ctl, owners ? f.owner : (int32_t*)nullptr);
  hipLaunchKernelGGL(gf_seed_kernel, per_source, dim3(256), 0, e->stream, f.field, f.keys, ctl, goals, seed, n, goal0, rows, cols,
                     e->tiles_i, s0, s1, master, bits);
  RNA_HIP(e, hipGetLastError());
  // Rounds in chunks; the pending count decides between them.  Hard caps, from true bounds: a
  // shortest path crosses tile borders at most once per border cell, fewer than 128 x tiles times, and after k plain rounds
  // every cell whose path has <= k crossings is final; with a width the smallest pending key grows by >= 1000 a round and the
  // finite distances of a connected component lie within 1414 x its cells of its cheapest source: 1414 x cells over all of
  // them, and one round per source for the gaps between them.  More rounds than that, or 30 s, is a bug in the kernel: an
  // error, not a hang.
  const unsigned width = gf_width();
  const long long cap = (width ? (long long)(1.5 * (double)e->ncell) + 64 : 128ll * ntile + 64) + (n - 1);
  const auto t0 = std::chrono::steady_clock::now();
  long long round = 0;
  for (;;) {
    for (int k = 0; k < GF_CHUNK; ++k, ++round)
      hipLaunchKernelGGL(pen ? gf_round_kernel<true> : gf_round_kernel<false>, dim3(e->tiles_i, e->tiles_j), dim3(256), 0, e->stream,
                         f.field, e->nbr, f.keys, f.touched, ctl, (int)(round % 6), width, rows, cols, s0, s1,
                         pen ? e->clearance.clr : (const uint16_t*)nullptr, f.pen, pen_r2);
    if ((rc = f.ctl.read(e)) != RNA_OK) return rc;
    // (the device form's sources are seen here first: the seed kernel skipped the bad ones, the field is dropped)
    if (host->invalid_sources)
      return fail(e, RNA_EINVAL, std::string(who) + ": " + std::to_string(host->invalid_sources) +
                                     " sources with a cell outside the map or a start cost outside [0, 2^30)");
    if (host->round[(round + 2) % 3].pending == 0) break;
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (round > cap || secs > 30.0)
      return fail(e, RNA_ECAPACITY, std::string(who) + ": the relaxation did not settle within its bound (" + std::to_string(round) +
                                        " rounds, " + std::to_string(secs) + " s)");
  }
  hipLaunchKernelGGL(gf_terminal_kernel, per_source, dim3(256), 0, e->stream, f.field, f.next, owners ? f.owner : (int32_t*)nullptr, goals,
                     seed, n, goal0, rows, cols, e->tiles_i, s0, s1, master, bits);
  hipLaunchKernelGGL(pen ? gf_finalize_kernel<true> : gf_finalize_kernel<false>, dim3(e->tiles_i, e->tiles_j), dim3(256), 0, e->stream,
                     f.field, e->nbr, f.next, f.touched, ctl, rows, cols, s0, s1, pen ? e->clearance.clr : (const uint16_t*)nullptr,
                     f.pen, pen_r2);
  if ((rc = f.ctl.read(e)) != RNA_OK) return rc;
  f.rows = rows; f.cols = cols; f.s0 = s0; f.s1 = s1;
  f.epoch = e->map.epoch;
  f.cost_changed = false;
  if (getenv("RNA_GOAL_FIELD_STATS"))   // developer knob
    fprintf(stderr, "[goal field] width %u: %d rounds, %d tile jobs on %d tiles, %d passes (longest job %d)\n", width, host->rounds,
            host->tile_jobs, host->tiles_reached, host->passes, host->max_passes);
  // (the pass below overwrites the pinned copy)
  const rna_goal_field_info info = {host->goal0, host->blocked_sources == n ? 2 : 0, host->reached, host->max_cost, host->rounds,
                                    host->tile_jobs, host->tiles_reached, 0};
  rna_goal_field_sources_info src = {n, host->blocked_sources, host->terminals, owners ? 1 : 0, 0, {0, 0, 0}};
  // (every source blocked: nothing was relaxed, the labels are the -1 of gf_init_kernel)
  if (owners && info.status == 0 && (rc = gf_owners(e, &src.owner_rounds)) != RNA_OK) return rc;
  f.info = info;
  f.sources = src;
  if (info_host) *info_host = f.info;
  return RNA_OK;
}

int gf_owners_ready(rna_engine* e, const char* who) {
  if (e->gfield.info.goal < 0) return fail(e, RNA_ESTATE, std::string(who) + ": no field has been built");
  if (!e->gfield.sources.owners) return fail(e, RNA_ESTATE, std::string(who) + ": the field was built without RNA_GOAL_FIELD_OWNERS");
  return RNA_OK;
}

}  // namespace

extern "C" int rna_goal_field_build(rna_engine* e, int32_t goal, rna_goal_field_info* info_host) {
  if (!e) return RNA_EINVAL;
  if (goal < 0 || (size_t)goal >= e->ncell) return fail(e, RNA_EINVAL, "rna_goal_field_build: goal outside the map");
  RNA_ENTER(e);
  return gf_build(e, nullptr, nullptr, 1, goal, 0u, info_host, "rna_goal_field_build");
}

extern "C" int rna_goal_field_build_multi_device(rna_engine* e, const int32_t* goals_device, const int32_t* seed_device, int n,
                                                 unsigned flags, rna_goal_field_info* info_host) {
  if (!e) return RNA_EINVAL;
  if (n < 1 || (size_t)n > e->ncell || !goals_device || (flags & ~(unsigned)RNA_GOAL_FIELD_OWNERS))
    return fail(e, RNA_EINVAL, "rna_goal_field_build_multi_device: n outside 1..cells, NULL goals or unknown flag bits");
  RNA_ENTER(e);
  return gf_build(e, goals_device, seed_device, n, -1, flags, info_host, "rna_goal_field_build_multi_device");
}

extern "C" int rna_goal_field_build_multi(rna_engine* e, const int32_t* goals_host, const int32_t* seed_host, int n, unsigned flags,
                                          rna_goal_field_info* info_host) {
  if (!e) return RNA_EINVAL;
  if (n < 1 || (size_t)n > e->ncell || !goals_host || (flags & ~(unsigned)RNA_GOAL_FIELD_OWNERS))
    return fail(e, RNA_EINVAL, "rna_goal_field_build_multi: n outside 1..cells, NULL goals or unknown flag bits");
  for (int k = 0; k < n; ++k) {
    if (goals_host[k] < 0 || (size_t)goals_host[k] >= e->ncell) return fail(e, RNA_EINVAL, "rna_goal_field_build_multi: goal outside the map");
    if (seed_host && (seed_host[k] < 0 || seed_host[k] >= (1 << 30)))
      return fail(e, RNA_EINVAL, "rna_goal_field_build_multi: start cost outside [0, 2^30)");
  }
  RNA_ENTER(e);
  Staging st(e, "rna_goal_field_build_multi");
  const int32_t* d_goals = st.in(goals_host, (size_t)n);
  const int32_t* d_seed = seed_host ? st.in(seed_host, (size_t)n) : nullptr;
  if (!st.ok()) return st.finish();
  // (a failed build may have left kernels behind that read the arrays: st waits for the stream before it frees them)
  const int rc = gf_build(e, d_goals, d_seed, n, -1, flags, info_host, "rna_goal_field_build_multi");
  return rc != RNA_OK ? rc : st.finish();
}

extern "C" int rna_goal_field_sources_info_get(const rna_engine* e, rna_goal_field_sources_info* out) {
  if (!e || !out) return RNA_EINVAL;
  *out = e->gfield.sources;
  return RNA_OK;
}

extern "C" int rna_goal_field_owners_download(rna_engine* e, int32_t* owners_host, size_t n_cells) {
  if (!e || !owners_host || n_cells != e->ncell) return RNA_EINVAL;
  const int rc = gf_owners_ready(e, "rna_goal_field_owners_download");
  if (rc != RNA_OK) return rc;
  RNA_ENTER_NOJOIN(e);
  RNA_HIP(e, hipMemcpyAsync(owners_host, e->gfield.owner, n_cells * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  RNA_HIP(e, hipStreamSynchronize(e->stream));
  return RNA_OK;
}

extern "C" void* rna_goal_field_owners_device_ptr(rna_engine* e) {
  return (e && e->gfield.info.goal >= 0 && e->gfield.sources.owners) ? (void*)e->gfield.owner : nullptr;
}

extern "C" int rna_goal_field_owners_at(rna_engine* e, const int32_t* cells_host, int n, int32_t* owners_host) {
  if (!e || n < 0 || (n > 0 && (!cells_host || !owners_host))) return RNA_EINVAL;
  const int rc = gf_owners_ready(e, "rna_goal_field_owners_at");
  if (rc != RNA_OK) return rc;
  if (n == 0) return RNA_OK;
  RNA_ENTER_NOJOIN(e);
  // a few cells (the frontier records' nearest cells): one word each, no kernel
  for (int k = 0; k < n; ++k) {
    owners_host[k] = -1;
    if (cells_host[k] >= 0 && (size_t)cells_host[k] < e->ncell)
      RNA_HIP(e, hipMemcpyAsync(&owners_host[k], e->gfield.owner + cells_host[k], sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  }
  RNA_HIP(e, hipStreamSynchronize(e->stream));
  return RNA_OK;
}

extern "C" int rna_goal_field_info_get(const rna_engine* e, rna_goal_field_info* out) {
  if (!e || !out) return RNA_EINVAL;
  *out = e->gfield.info;
  out->stale = (out->goal >= 0 && (e->gfield.epoch != e->map.epoch || e->gfield.cost_changed)) ? 1 : 0;
  return RNA_OK;
}

extern "C" int rna_goal_field_set_clearance_cost(rna_engine* e, const uint16_t* cost_by_cells, int n) {
  if (!e || n < 0 || (n > 0 && (!cost_by_cells || n < 2 || n > 64))) return RNA_EINVAL;
  GoalField& f = e->gfield;
  f.cost_n = n;
  for (int k = 0; k < 64; ++k) f.cost_tab[k] = k < n ? cost_by_cells[k] : (uint16_t)0;
  f.cost_changed = true;
  f.pen_current = false;
  return RNA_OK;
}

extern "C" int rna_goal_field_get_clearance_cost(const rna_engine* e, uint16_t* out, int cap) {
  if (!e || cap < 0 || (cap > 0 && !out)) return RNA_EINVAL;
  const GoalField& f = e->gfield;
  for (int k = 0; k < f.cost_n && k < cap; ++k) out[k] = f.cost_tab[k];
  return f.cost_n;
}

extern "C" int rna_goal_field_download(rna_engine* e, int32_t* field_host, uint8_t* next_host, size_t n_cells) {
  if (!e || (!field_host && !next_host) || n_cells != e->ncell) return RNA_EINVAL;
  if (e->gfield.info.goal < 0) return fail(e, RNA_ESTATE, "rna_goal_field_download: no field has been built");
  RNA_ENTER_NOJOIN(e);
  if (field_host) RNA_HIP(e, hipMemcpyAsync(field_host, e->gfield.field, n_cells * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  if (next_host) RNA_HIP(e, hipMemcpyAsync(next_host, e->gfield.next, n_cells, hipMemcpyDeviceToHost, e->stream));
  RNA_HIP(e, hipStreamSynchronize(e->stream));
  return RNA_OK;
}

extern "C" void* rna_goal_field_device_ptr(rna_engine* e) {
  return (e && e->gfield.info.goal >= 0) ? (void*)e->gfield.field : nullptr;
}

static int gf_paths(rna_engine* e, const int32_t* starts, int n, int32_t* paths, int max_path_len, rna_astar_result* results, bool host) {
  if (!e || n < 0 || max_path_len <= 0 || (n > 0 && (!starts || !paths || !results))) return RNA_EINVAL;
  const GoalField& f = e->gfield;
  if (f.info.goal < 0) return fail(e, RNA_ESTATE, "rna_goal_field_paths: no field has been built");
  if (n == 0) return RNA_OK;
  RNA_ENTER_NOJOIN(e);
  Staging st(e, "rna_goal_field_paths");
  const int32_t* d_starts = host ? st.in(starts, (size_t)n) : starts;
  // (cells behind a path's end come back as 0; the _device form leaves them as the caller's buffer had them)
  int32_t* d_paths = host ? st.out(paths, (size_t)n * max_path_len, true) : paths;
  rna_astar_result* d_res = host ? st.out(results, (size_t)n) : results;
  if (st.ok())
    hipLaunchKernelGGL(gf_paths_kernel, dim3(n), dim3(64), 0, e->stream, f.field, f.next, d_starts, n, d_paths, max_path_len, d_res,
                       f.rows, f.cols, f.s0, f.s1);
  return st.finish();
}

extern "C" int rna_goal_field_paths(rna_engine* e, const int32_t* starts_host, int n, int32_t* paths_host, int max_path_len,
                                    rna_astar_result* results_host) {
  return gf_paths(e, starts_host, n, paths_host, max_path_len, results_host, true);
}

extern "C" int rna_goal_field_paths_device(rna_engine* e, const int32_t* starts_device, int n, int32_t* paths_device, int max_path_len,
                                           rna_astar_result* results_device) {
  return gf_paths(e, starts_device, n, paths_device, max_path_len, results_device, false);
}
