// map_tiles_dev.hpp -- device code shared by the kernels that work on 64 x 64 MAP-space tiles or on a window of the master
// layer in map space (engine.hip, footprint.hip, clearance.hip, frontier.hip, goal_field.hip, shortcut.hip, viewgain.hip,
// scanmatch.hip).  The decisions that live here and nowhere else: the blocked predicate, the neighbour-mask rule and the
// neighbour order, the dirty ring of a tile, the reduction over a wavefront, how a workgroup reads the rows of a window of
// `master` (window_rows_each), the occupancy bit rows of a tile in LDS, and the layout of the footprint's blocked bits.
// (The map <-> circular-buffer index pair, the range test of a cell handed in from outside and the line walk are
// gridmath.hpp's.)  Everything is __forceinline__: nothing becomes a call at run time.
#pragma once
#include "engine.hpp"

namespace rna {

// GlobalPlanner::ifBlocked predicate (mc/include/move_control/map_global_planner.h:47-50):
// blocked iff the master value is finite-or-inf (not NaN) and > 0.
__device__ __forceinline__ bool cell_blocked(float v) { return !(v != v) && v > 0.0f; }

// ---- the neighbour order (DESIGN.md "Grid A* contract"): bit k of a mask <-> neighbour (di, dj) in the order
// (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1) ----
__device__ __forceinline__ int nbr_di(int k) { return (int)((0x9224u >> (2 * k)) & 3u) - 1; }   // di + 1 = 0 1 2 0 2 0 1 2, two bits each
__device__ __forceinline__ int nbr_dj(int k) { return k < 3 ? -1 : (k < 5 ? 0 : 1); }
// the mask bit of the king move (di, dj)
__device__ __forceinline__ unsigned nbr_move_bit(int di, int dj) {
  const int k = (dj + 1) * 3 + (di + 1);
  return 1u << (k > 4 ? k - 1 : k);
}

// The 8-bit traversable-neighbour mask of a cell from blocked bytes ([j][i], i fastest, row stride S; c = the cell's byte, its
// eight neighbours addressable): 0 for a blocked cell; a diagonal needs the target and both orthogonal cells free.
__device__ __forceinline__ unsigned nbr_mask_of(const uint8_t* c, int S) {
  unsigned m = 0;
  if (!c[0]) {
    const bool up = !c[-1], dn = !c[1], lf = !c[-S], rt = !c[S];
    if (lf && up && !c[-S - 1]) m |= 1u;        // (-1,-1)
    if (lf) m |= 2u;                            // ( 0,-1)
    if (lf && dn && !c[-S + 1]) m |= 4u;        // ( 1,-1)
    if (up) m |= 8u;                            // (-1, 0)
    if (dn) m |= 16u;                           // ( 1, 0)
    if (rt && up && !c[S - 1]) m |= 32u;        // (-1, 1)
    if (rt) m |= 64u;                           // ( 0, 1)
    if (rt && dn && !c[S + 1]) m |= 128u;       // ( 1, 1)
  }
  return m;
}

// The dirty ring of tile (ti, tj): bit (dj + 1) * 3 + (di + 1) is set when the tile (ti + di, tj + dj) exists and its byte of
// `dirty` is set (bit 4: the tile itself).  != 0: the tile's masks have to be recomputed.  The nine reads depend neither on
// one another nor on a branch (a tile that does not exist reads the nearest one that does and drops it): they leave together,
// one wait for all of them.
__device__ __forceinline__ unsigned dirty_ring(const unsigned* __restrict__ dirty, int ti, int tj, int tiles_i, int tiles_j) {
  const unsigned char* dflag = reinterpret_cast<const unsigned char*>(dirty);
  unsigned dmask = 0u;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int a = ti + k % 3 - 1, b = tj + k / 3 - 1;
    const bool in = a >= 0 && b >= 0 && a < tiles_i && b < tiles_j;
    const unsigned char f = dflag[min(max(b, 0), tiles_j - 1) * tiles_i + min(max(a, 0), tiles_i - 1)];
    if (in && f) dmask |= 1u << k;
  }
  return dmask;
}

constexpr int COMPOSE_BLK_BYTES = (TILE + 2) * (TILE + 2);   // LDS of a workgroup: the tile's blocked bytes with a 1-cell ring

// One tile tt, all threads of the workgroup (any size): the block of a dirty tile copies laser -> master
// (composeMasterMapFromLayerdMap, mc/src/map_provider.cpp:216-223, restricted to where the two layers differ), and every
// block whose tile is dirty or touches a dirty tile recomputes its cells' masks.  A cell of a DIRTY tile is read from the
// laser layer -- what master holds there once the launch has finished; its own block may still be copying --, a cell of
// a clean tile from master.  The block also clears its byte of `next_dirty`.  `blk`: COMPOSE_BLK_BYTES of LDS, [jj][ii],
// ii fastest; out of map = blocked.  Two workgroup barriers inside (all threads must call, tt uniform).
__device__ __forceinline__ void compose_nbr_tile(uint8_t* __restrict__ blk, int tt, uint8_t* __restrict__ nbr, float* __restrict__ master,
                                                 const float* __restrict__ laser, const unsigned* __restrict__ dirty,
                                                 unsigned* __restrict__ next_dirty, int rows, int cols, int tiles_i, int tiles_j) {
  const int ti = tt % tiles_i, tj = tt / tiles_i;
  const unsigned dmask = dirty_ring(dirty, ti, tj, tiles_i, tiles_j);
  if (threadIdx.x == 0) reinterpret_cast<volatile unsigned char*>(next_dirty)[tj * tiles_i + ti] = 0;
  if (!dmask) return;   // (uniform across the workgroup)
  const bool own = (dmask >> 4) & 1u;
  __syncthreads();        // the previous tile's block has been read
  const int i0 = ti * TILE - 1, j0 = tj * TILE - 1;
  for (int k = threadIdx.x; k < (TILE + 2) * (TILE + 2); k += blockDim.x) {
    const int ii = k % (TILE + 2), jj = k / (TILE + 2);
    const int i = i0 + ii, j = j0 + jj;
    uint8_t b = 1;
    if (i >= 0 && j >= 0 && i < rows && j < cols) {
      const int di = ii == 0 ? 0 : (ii == TILE + 1 ? 2 : 1), dj = jj == 0 ? 0 : (jj == TILE + 1 ? 2 : 1);
      const size_t lin = (size_t)j * rows + i;
      const bool from_laser = (dmask >> (dj * 3 + di)) & 1u;
      const float v = from_laser ? laser[lin] : master[lin];
      if (own && di == 1 && dj == 1) master[lin] = v;   // the compose itself
      b = cell_blocked(v) ? 1 : 0;
    }
    blk[k] = b;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < TILE * TILE; k += blockDim.x) {
    const int li = k & (TILE - 1), lj = k >> 6;
    const int i = ti * TILE + li, j = tj * TILE + lj;
    if (i >= rows || j >= cols) continue;
    nbr[(size_t)j * rows + i] = (uint8_t)nbr_mask_of(&blk[(lj + 1) * (TILE + 2) + (li + 1)], TILE + 2);
  }
}

// ---- butterfly reductions over the 64 lanes of a wavefront: every lane returns the result ----
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

// ---- how a workgroup reads a window of `master`: the rows j0 .. j0 + H - 1, the columns i0 .. i0 + W - 1, W <= 64 NP, in map
// space (the window may overhang the map on any side).  All 256 threads call.  Wavefront w takes the rows 2w, 2w + 1, then
// + 8, ...; the 2 NP reads of a trip (2 rows x NP pieces of 64 consecutive i, through buffer_lin: coalesced, and right on a
// moved map) leave together, before anything is done with a value.  (A read per (row, piece) and trip left the loads of a
// wavefront one memory round trip apart.)  A lane without a cell -- its piece beyond ceil(W / 64), its column beyond W, its
// row beyond H, or the cell outside the map -- reads nothing.  Then f(row, piece, ok, value) is called by the whole wavefront,
// uniformly, once per (row, piece) that exists: row and piece relative to (j0, i0), ok = the lane has a cell, value = its
// master value (0 without one).  f may ballot; what it ballots and where the bits go is the caller's. ----
template <int NP, class F>
__device__ __forceinline__ void window_rows_each(const float* __restrict__ master, int i0, int j0, int W, int H, int rows, int cols, int s0,
                                                 int s1, F f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NC = (W + 63) >> 6;   // 64-cell pieces of a row
  for (int r0 = 2 * wave; r0 < H; r0 += 8) {
    float v[2][NP];
    bool ok[2][NP];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int c = p * 64 + lane, i = i0 + c, j = j0 + r0 + u;
        ok[u][p] = p < NC && r0 + u < H && c < W && i >= 0 && j >= 0 && i < rows && j < cols;
        v[u][p] = 0.0f;
        if (ok[u][p]) v[u][p] = master[buffer_lin(i, j, rows, cols, s0, s1)];
      }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (r0 + u >= H) break;   // (uniform)
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (p >= NC) break;     // (uniform)
        f(r0 + u, p, ok[u][p], v[u][p]);
      }
    }
  }
}

// ---- occupancy bit rows of a tile in LDS: occ[row][4], row jj = map row j0 - H + jj, words 0..2 = the bits of the map cells
// i0 - 64 .. i0 + 127, word 3 = 0 (so that a window may start anywhere in words 0..2) ----

// Fills the TILE + 2 H rows of tile (i0, j0) with halo H from `master`: bit = cell_blocked, 0 outside the map and beyond the
// halo along i.  256 threads, the trips of window_rows_each (3 words x 2 rows), the caller's barrier follows.  NOT a caller of
// window_rows_each, measured (profiles/window_helpers_rows_parent_vs_branch.txt): there a lane without a cell skips its read
// under a branch of its own, here it reads cell 0 and drops it, six reads and no branch -- as a caller, with the halo clip in
// the functor or in the window, footprint_tiles_kernel took 4 to 7 % longer (R = 3 .. 63) and clearance_tiles_kernel 2 to 9 %.
__device__ __forceinline__ void occ_rows_load(unsigned long long (*__restrict__ occ)[4], const float* __restrict__ master, int i0, int j0,
                                              int H, int rows, int cols, int s0, int s1) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nrow = TILE + 2 * H;
  for (int jj0 = 2 * wave; jj0 < nrow; jj0 += 8) {
    float v[2][3];
    bool ok[2][3];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int word = 0; word < 3; ++word) {
        const int i = i0 - 64 + word * 64 + lane, j = j0 - H + jj0 + u;
        ok[u][word] = jj0 + u < nrow && i >= i0 - H && i < i0 + TILE + H && i >= 0 && j >= 0 && i < rows && j < cols;
        v[u][word] = master[ok[u][word] ? buffer_lin(i, j, rows, cols, s0, s1) : 0];   // (cell 0 for lanes without a cell: read, not used)
      }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (jj0 + u >= nrow) break;   // (uniform)
#pragma unroll
      for (int word = 0; word < 3; ++word) {
        const unsigned long long m = __ballot(ok[u][word] && cell_blocked(v[u][word]));
        if (lane == 0) occ[jj0 + u][word] = m;
      }
      if (lane == 0) occ[jj0 + u][3] = 0ull;
    }
  }
}

__device__ __forceinline__ unsigned long long funnel64(unsigned long long lo, unsigned long long hi, int s) {
  return s ? (lo >> s) | (hi << (64 - s)) : lo;
}

// The two 64-bit windows of occupancy row `o` around bit p, 63 <= p <= 128 (the cell in tile column li is bit li + 64):
// lo = bits p - 63 .. p, the cell is its bit 63; hi = bits p .. p + 63, the cell is its bit 0.
__device__ __forceinline__ void occ_windows(const unsigned long long* o, int p, unsigned long long& lo, unsigned long long& hi) {
  const int q1 = p - 63, k1 = q1 >> 6, s1 = q1 & 63, k2 = p >> 6, s2 = p & 63;
  lo = funnel64(o[k1], o[k1 + 1], s1);
  hi = funnel64(o[k2], o[k2 + 1], s2);
}

// ---- the footprint's blocked bits (rna_engine::fp_bits): TILE words per map-space tile, tiles in row-major order of
// (tj, ti); word = map row j of the tile, bit = i % TILE ----
__device__ __forceinline__ size_t fp_bits_index(int tiles_i, int a, int j) { return ((size_t)(j / TILE) * tiles_i + a) * TILE + (j % TILE); }
// the word of map row j in tile column a; 0 outside the map
__device__ __forceinline__ unsigned long long fp_bits_word(const unsigned long long* __restrict__ bits, int tiles_i, int cols, int a, int j) {
  return (a >= 0 && a < tiles_i && j >= 0 && j < cols) ? bits[fp_bits_index(tiles_i, a, j)] : 0ull;
}
// the bit of the map cell (i, j)
__device__ __forceinline__ bool fp_bit(const unsigned long long* __restrict__ bits, int tiles_i, int cols, int i, int j) {
  return (fp_bits_word(bits, tiles_i, cols, i / TILE, j) >> (i % TILE)) & 1ull;
}

}  // namespace rna
