// goal_field.hip -- the goal distance field of the grid A*: one sweep from the goal serves every start.
// What navfn / global_planner offer on a ROS stack and the reference's replan loop would use (Nav::loopPlan replans to
// the same clicked goal while the robot moves, mc/src/nav_node.cpp:103-154): the exact 1000 / 1414 integer cost-to-goal
// of every cell under the grid A* contract (oracle/astar.c), and plans from any start as a walk downhill.
//
// The field is the least fixpoint of field[c] = min over the neighbours n that c's mask allows of field[n] + w(n, c) with
// field[goal] = 0.  It is unique, so any relaxation order gives the same bits; the kernels below only decide how much
// work is redone:
//   gf_init_kernel / gf_seed_kernel   every cell unreached, the goal 0, the goal's tile and its ring pending
//   gf_round_kernel     one launch = one round: a workgroup per 64 x 64 MAP-space tile; a pending tile loads its field with
//                       a one-cell halo and its masks into LDS, relaxes there until nothing changes, stores what fell and
//                       posts the smallest improved value of each of its eight borders as the neighbour tile's pending key
//                       FOR THE NEXT LAUNCH.  No workgroup waits for another: whatever a tile reads of a neighbour that is
//                       being written in the same launch is a valid upper bound, and the neighbour's post makes the tile
//                       run again after the launch boundary.  Tiles whose key lies `width` above the smallest pending key
//                       are put off (the search kernel's f-buckets one level up); width 0 = every pending tile every round.
//   gf_finalize_kernel  per reached tile: the canonical step of every cell (`next`, the oracle's backtrace rule run over a
//                       field rooted at the goal), reached cells, largest distance
//   gf_paths_kernel     one wavefront per start: follows `next` tile by tile through LDS, writes the path start first
// Clearance cost (rna_goal_field_set_clearance_cost): with a table set the fixpoint is field[c] = pen[c] + min(field[n] + w),
// pen[c] the table's cost for c's clearance (clearance.hip) -- a non-negative integer per cell, so the least fixpoint is
// still unique and the same relaxation finds it.  gf_round_kernel<true> / gf_finalize_kernel<true> are that build; the
// <false> instantiations are the table-free kernels: no penalty load, no extra LDS, the same sweeps as before the table existed.
// Termination is the host's: it enqueues rounds in chunks, reads the pending count back and stops at zero (rna_goal_field_build).
// A field is a snapshot: the kernels read the live masks only during the build; paths follow the stored `next` bytes.
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
};

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
                               uint8_t* __restrict__ touched, int ntile) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < ncell; k += stride) {
    field[k] = GF_INF;
    next[k] = GF_NEXT_NONE;
  }
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < (size_t)ntile; k += stride) {
    keys[k] = GF_INF;
    keys[ntile + k] = GF_INF;
    touched[k] = 0;
  }
}

// one thread: the control words, and -- unless the goal cell is blocked (robot radius: the footprint's blocked set, else the
// master layer's own predicate) -- field[goal] = 0 and the goal's tile pending for round 0
__global__ void gf_seed_kernel(int32_t* __restrict__ field, int* __restrict__ keys, GfCtl* __restrict__ ctl, int goal, int rows,
                               int cols, int tiles_i, int s0, int s1, const float* __restrict__ master,
                               const unsigned long long* __restrict__ bits) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int i, j;
  map_cell_of(goal, rows, cols, s0, s1, i, j);
  const bool blocked = bits ? fp_bit(bits, tiles_i, cols, i, j) : cell_blocked(master[goal]);
  GfCtl c = {};
  c.round[0].min_key = c.round[1].min_key = GF_INF;
  c.round[2].min_key = 0;
  c.round[2].pending = blocked ? 0 : 1;
  c.status = blocked ? 2 : 0;
  *ctl = c;
  if (!blocked) {
    // the goal's tile and its ring: the 0 is stored here, not by a tile job, so no job would post it to a neighbour tile
    // when the goal lies on its tile's border (and its neighbours inside the tile are blocked)
    field[goal] = 0;
    const int tiles_j = (cols + TILE - 1) / TILE;
    for (int b = j / TILE - 1; b <= j / TILE + 1; ++b)
      for (int a = i / TILE - 1; a <= i / TILE + 1; ++a)
        if (a >= 0 && b >= 0 && a < tiles_i && b < tiles_j) keys[b * tiles_i + a] = 0;
  }
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
// the goal.  Also the build's totals.  PEN: field[n] + w + the cell's own clearance cost == field[c].
template <bool PEN>
__global__ void __launch_bounds__(256) gf_finalize_kernel(const int32_t* __restrict__ field, const uint8_t* __restrict__ nbr,
                                                          uint8_t* __restrict__ next, const uint8_t* __restrict__ touched,
                                                          GfCtl* __restrict__ ctl, int goal, int rows, int cols, int s0, int s1,
                                                          const uint16_t* __restrict__ clr, const uint16_t* __restrict__ pen_tab, int pen_r2) {
  __shared__ int F[GF_W * GF_S];
  __shared__ int tot[2];
  const int tiles_i = gridDim.x;
  const int ti = blockIdx.x, tj = blockIdx.y, t = tj * tiles_i + ti;
  if (!touched[t]) return;
  const int i0 = ti * TILE, j0 = tj * TILE;
  gf_load_field(F, field, i0, j0, rows, cols, s0, s1);
  if (threadIdx.x < 2) tot[threadIdx.x] = 0;
  __syncthreads();
  int n_reached = 0, v_max = 0;
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
      if ((int)b == goal) nx = GF_NEXT_GOAL;
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
  }
  __syncthreads();
  if (threadIdx.x == 0 && tot[0]) {
    atomicAdd(&ctl->reached, tot[0]);
    atomicMax(&ctl->max_cost, tot[1]);
    atomicAdd(&ctl->tiles_reached, 1);
  }
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
  f.pen_current = false;
  if (f.ctl) { (void)hipFree(f.ctl); f.ctl = nullptr; }
  if (f.ctl_host) { (void)hipHostFree(f.ctl_host); f.ctl_host = nullptr; }
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
  if (rc == RNA_OK && hipMalloc(&f.ctl, sizeof(GfCtl)) != hipSuccess) rc = fail(e, RNA_ENOMEM, "hipMalloc failed");
  if (rc == RNA_OK && hipHostMalloc(&f.ctl_host, sizeof(GfCtl)) != hipSuccess) rc = fail(e, RNA_ENOMEM, "hipHostMalloc failed");
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

extern "C" int rna_goal_field_build(rna_engine* e, int32_t goal, rna_goal_field_info* info_host) {
  if (!e) return RNA_EINVAL;
  if (goal < 0 || (size_t)goal >= e->ncell) return fail(e, RNA_EINVAL, "rna_goal_field_build: goal outside the map");
  RNA_ENTER(e);
  int rc = map_prepare_nbr(e);
  if (rc != RNA_OK) return rc;
  if ((rc = gf_alloc(e)) != RNA_OK) return rc;
  GoalField& f = e->gfield;
  // clearance cost: a clearance field of the table's cap for the current masks, and the table by squared clearance
  const bool pen = f.cost_n > 0;
  const int pen_r = f.cost_n - 1, pen_r2 = pen_r * pen_r;
  if (pen) {
    if (e->clearance.R != pen_r || e->clearance.epoch != e->map_epoch)
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
  GfCtl* ctl = static_cast<GfCtl*>(f.ctl);
  GfCtl* host = static_cast<GfCtl*>(f.ctl_host);
  hipLaunchKernelGGL(gf_init_kernel, dim3((unsigned)std::min<size_t>((e->ncell + 255) / 256, 8192)), dim3(256), 0, e->stream, f.field,
                     f.next, e->ncell, f.keys, f.touched, ntile);
  hipLaunchKernelGGL(gf_seed_kernel, dim3(1), dim3(1), 0, e->stream, f.field, f.keys, ctl, goal, rows, cols, e->tiles_i, s0, s1,
                     e->layer[RNA_LAYER_MASTER], e->robot_r > 0.0 ? e->fp_bits : (const unsigned long long*)nullptr);
  RNA_HIP(e, hipGetLastError());
  // Rounds in chunks; the pending count decides between them.  Hard caps, from true bounds: a
  // shortest path crosses tile borders at most once per border cell, fewer than 128 x tiles times, and after k plain rounds
  // every cell whose path has <= k crossings is final; with a width the smallest pending key grows by >= 1000 a round and no
  // finite distance exceeds 1414 x cells.  More rounds than that, or 30 s, is a bug in the kernel: an error, not a hang.
  const unsigned width = gf_width();
  const long long cap = width ? (long long)(1.5 * (double)e->ncell) + 64 : 128ll * ntile + 64;
  const auto t0 = std::chrono::steady_clock::now();
  long long round = 0;
  for (;;) {
    for (int k = 0; k < GF_CHUNK; ++k, ++round)
      hipLaunchKernelGGL(pen ? gf_round_kernel<true> : gf_round_kernel<false>, dim3(e->tiles_i, e->tiles_j), dim3(256), 0, e->stream,
                         f.field, e->nbr, f.keys, f.touched, ctl, (int)(round % 6), width, rows, cols, s0, s1,
                         pen ? e->clearance.clr : (const uint16_t*)nullptr, f.pen, pen_r2);
    RNA_HIP(e, hipGetLastError());
    RNA_HIP(e, hipMemcpyAsync(host, ctl, sizeof(GfCtl), hipMemcpyDeviceToHost, e->stream));
    RNA_HIP(e, hipStreamSynchronize(e->stream));
    if (host->round[(round + 2) % 3].pending == 0) break;
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (round > cap || secs > 30.0)
      return fail(e, RNA_ECAPACITY, "rna_goal_field_build: the relaxation did not settle within its bound (" + std::to_string(round) +
                                        " rounds, " + std::to_string(secs) + " s)");
  }
  hipLaunchKernelGGL(pen ? gf_finalize_kernel<true> : gf_finalize_kernel<false>, dim3(e->tiles_i, e->tiles_j), dim3(256), 0, e->stream,
                     f.field, e->nbr, f.next, f.touched, ctl, goal, rows, cols, s0, s1, pen ? e->clearance.clr : (const uint16_t*)nullptr,
                     f.pen, pen_r2);
  RNA_HIP(e, hipGetLastError());
  RNA_HIP(e, hipMemcpyAsync(host, ctl, sizeof(GfCtl), hipMemcpyDeviceToHost, e->stream));
  RNA_HIP(e, hipStreamSynchronize(e->stream));
  f.rows = rows; f.cols = cols; f.s0 = s0; f.s1 = s1;
  f.epoch = e->map_epoch;
  f.cost_changed = false;
  if (getenv("RNA_GOAL_FIELD_STATS"))   // developer knob
    fprintf(stderr, "[goal field] width %u: %d rounds, %d tile jobs on %d tiles, %d passes (longest job %d)\n", width, host->rounds,
            host->tile_jobs, host->tiles_reached, host->passes, host->max_passes);
  f.info = rna_goal_field_info{goal, host->status, host->reached, host->max_cost, host->rounds, host->tile_jobs, host->tiles_reached, 0};
  if (info_host) *info_host = f.info;
  return RNA_OK;
}

extern "C" int rna_goal_field_info_get(const rna_engine* e, rna_goal_field_info* out) {
  if (!e || !out) return RNA_EINVAL;
  *out = e->gfield.info;
  out->stale = (out->goal >= 0 && (e->gfield.epoch != e->map_epoch || e->gfield.cost_changed)) ? 1 : 0;
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
  int32_t *d_starts = const_cast<int32_t*>(starts), *d_paths = paths;
  rna_astar_result* d_res = results;
  hipError_t err = hipSuccess;
  if (host) {
    d_starts = d_paths = nullptr;
    d_res = nullptr;
    err = hipMalloc(&d_starts, (size_t)n * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc(&d_paths, (size_t)n * max_path_len * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc(&d_res, (size_t)n * sizeof(rna_astar_result));
    if (err == hipSuccess) err = hipMemcpyAsync(d_starts, starts, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    // (cells behind a path's end come back as 0; the _device form leaves them as the caller's buffer had them)
    if (err == hipSuccess) err = hipMemsetAsync(d_paths, 0, (size_t)n * max_path_len * sizeof(int32_t), e->stream);
  }
  if (err == hipSuccess) {
    hipLaunchKernelGGL(gf_paths_kernel, dim3(n), dim3(64), 0, e->stream, f.field, f.next, d_starts, n, d_paths, max_path_len, d_res,
                       f.rows, f.cols, f.s0, f.s1);
    err = hipGetLastError();
  }
  if (host) {
    if (err == hipSuccess)
      err = hipMemcpyAsync(paths, d_paths, (size_t)n * max_path_len * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(results, d_res, (size_t)n * sizeof(rna_astar_result), hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (d_starts) (void)hipFree(d_starts);
    if (d_paths) (void)hipFree(d_paths);
    if (d_res) (void)hipFree(d_res);
  }
  RNA_HIP(e, err);
  return RNA_OK;
}

extern "C" int rna_goal_field_paths(rna_engine* e, const int32_t* starts_host, int n, int32_t* paths_host, int max_path_len,
                                    rna_astar_result* results_host) {
  return gf_paths(e, starts_host, n, paths_host, max_path_len, results_host, true);
}

extern "C" int rna_goal_field_paths_device(rna_engine* e, const int32_t* starts_device, int n, int32_t* paths_device, int max_path_len,
                                           rna_astar_result* results_device) {
  return gf_paths(e, starts_device, n, paths_device, max_path_len, results_device, false);
}
