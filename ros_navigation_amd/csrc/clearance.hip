// clearance.hip -- the clearance field of the grid A*: how far every cell is from the search's blocked set.
// footprint.hip answers "is there an obstacle within r of this cell" for ONE radius; this answers it for every radius up to a
// cap at once: clr[c] = min over blocked cells b of di^2 + dj^2 (cells, map space, unwrapped indices), the exact squared
// Euclidean distance transform of the blocked set rna_astar_download_blocked returns (robot radius included), capped at R
// cells.  It is what a costmap's inflation layer is computed from; the goal field's clearance cost (goal_field.hip) reads it.
//
// Integers only, so the result is the definition's, bit for bit: a row dj of the map holds a blocked cell at squared distance
// dj^2 + d^2 from cell (i, j) where d is the distance along i from column i to the nearest set bit of row j + dj, and the
// minimum over the rows |dj| <= R of those is the minimum over all cells with |dj| <= R, |di| <= 63 -- a superset of the disc
// of radius R <= 63.  Cells outside the map hold no bit (CircleIterator does not visit them either).
#include "engine.hpp"
#include "map_tiles_dev.hpp"

#include <algorithm>

using namespace rna;

namespace {

constexpr int CLR_MAX_R = 63;                        // the footprint's bound: a tile needs its one-tile ring only
constexpr int CLR_ROWS = TILE + 2 * CLR_MAX_R;       // blocked-bit rows of a workgroup (halo R on each side)

}  // namespace

// One workgroup per 64 x 64 tile (MAP space; (s0, s1) = buffer start index), 256 threads:
//  1. blocked bits of the tile with a halo of R rows and one tile either side along i into LDS: row jj = map row j0 - R + jj,
//     words 0..2 = the map cells i0 - 64 .. i0 + 127 (word 3 stays 0; outside the map 0).  With a robot radius the bits are the
//     footprint's (`bits`, 64 x 64 per map-space tile); without one they are cell_blocked of master, a ballot per 64 cells.
//  2. per cell: best = R^2 + 1; for dj = 0, 1, -1, 2, -2, ... while dj^2 < best: the two 64-bit windows of row j + dj that end
//     and start at column i give the distance to the nearest set bit on either side (clz / ctz), best = min(best, dj^2 + d^2).
//     best <= R^2 is the answer, anything else RNA_CLEARANCE_NONE.
__global__ void __launch_bounds__(256) clearance_tiles_kernel(uint16_t* __restrict__ clr, const unsigned long long* __restrict__ bits,
                                                              const float* __restrict__ master, int R, int rows, int cols, int s0,
                                                              int s1) {
  __shared__ unsigned long long occ[CLR_ROWS][4];
  const int ti = blockIdx.x, tj = blockIdx.y, tiles_i = gridDim.x;
  const int i0 = ti * TILE, j0 = tj * TILE;
  const int nrow = TILE + 2 * R;   // <= CLR_ROWS (1 <= R <= CLR_MAX_R, checked by the host)
  if (bits) {
    // a thread per (row, word): the word of row j in tile (ti - 1 + word, j / 64), or 0 outside the map
    for (int k = threadIdx.x; k < nrow * 4; k += blockDim.x) {
      const int jj = k >> 2, word = k & 3;
      const int j = j0 - R + jj, a = ti - 1 + word;
      occ[jj][word] = word < 3 ? fp_bits_word(bits, tiles_i, cols, a, j) : 0ull;
    }
  } else {
    occ_rows_load(occ, master, i0, j0, R, rows, cols, s0, s1);
  }
  __syncthreads();
  const int none = R * R + 1;
  for (int k = threadIdx.x; k < TILE * TILE; k += blockDim.x) {
    const int li = k & (TILE - 1), lj = k >> 6;
    const int i = i0 + li, j = j0 + lj;
    if (i >= rows || j >= cols) continue;
    const int p = li + 64;                      // the cell's bit in its row (64 .. 127)
    const int jc = lj + R;                      // the cell's row in occ
    int best = none;
    for (int dj = 0; dj * dj < best; ++dj) {    // (dj <= R: (R + 1)^2 >= none)
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        if (side && !dj) continue;
        unsigned long long lo, hi;   // the cell is bit 63 of lo, bit 0 of hi
        occ_windows(occ[side ? jc - dj : jc + dj], p, lo, hi);
        const int dl = lo ? __clzll((long long)lo) : 64, dr = hi ? __ffsll((long long)hi) - 1 : 64;
        const int d = min(dl, dr);
        if (d < 64) best = min(best, dj * dj + d * d);
      }
    }
    clr[buffer_lin(i, j, rows, cols, s0, s1)] = best < none ? (uint16_t)best : (uint16_t)RNA_CLEARANCE_NONE;
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace rna {

int clearance_release(rna_engine* e) {
  dev_free(&e->clearance.clr);
  e->clearance.R = 0;
  return RNA_OK;
}

// the clearance field of the current masks with cap R, enqueued on the engine stream (the masks are refreshed first)
int clearance_refresh(rna_engine* e, int R) {
  if (R < 1 || R > CLR_MAX_R) return fail(e, RNA_EINVAL, "clearance: max_cells must satisfy 1 <= max_cells <= 63");
  int rc = map_prepare_nbr(e);
  if (rc != RNA_OK) return rc;
  Clearance& c = e->clearance;
  if (!c.clr && (rc = dev_alloc(e, &c.clr, e->ncell)) != RNA_OK) return rc;
  c.R = 0;   // (no field while this one is being built, also when the launch fails)
  const Geom& g = e->geom;
  hipLaunchKernelGGL(clearance_tiles_kernel, dim3(e->tiles_i, e->tiles_j), dim3(256), 0, e->stream, c.clr,
                     e->robot_r > 0.0 ? e->fp_bits : (const unsigned long long*)nullptr, e->layer[RNA_LAYER_MASTER], R, g.size[0], g.size[1],
                     g.start[0], g.start[1]);
  RNA_HIP(e, hipGetLastError());
  c.R = R;
  c.epoch = e->map.epoch;
  return RNA_OK;
}

}  // namespace rna

extern "C" int rna_clearance_build(rna_engine* e, int max_cells) {
  if (!e) return RNA_EINVAL;
  if (max_cells < 1 || max_cells > CLR_MAX_R) return RNA_EINVAL;
  RNA_ENTER(e);
  const int rc = clearance_refresh(e, max_cells);
  if (rc != RNA_OK) return rc;
  RNA_HIP(e, hipStreamSynchronize(e->stream));
  return RNA_OK;
}

extern "C" int rna_clearance_download(rna_engine* e, uint16_t* host, size_t n_cells) {
  if (!e || !host || n_cells != e->ncell) return RNA_EINVAL;
  if (e->clearance.R == 0) return fail(e, RNA_ESTATE, "rna_clearance_download: no clearance field has been built");
  RNA_ENTER_NOJOIN(e);
  RNA_HIP(e, hipMemcpyAsync(host, e->clearance.clr, n_cells * sizeof(uint16_t), hipMemcpyDeviceToHost, e->stream));
  RNA_HIP(e, hipStreamSynchronize(e->stream));
  return RNA_OK;
}

extern "C" void* rna_clearance_device_ptr(rna_engine* e) { return (e && e->clearance.R > 0) ? (void*)e->clearance.clr : nullptr; }

extern "C" int rna_clearance_info_get(const rna_engine* e, int* max_cells, int* stale) {
  if (!e || !max_cells || !stale) return RNA_EINVAL;
  *max_cells = e->clearance.R;
  *stale = (e->clearance.R > 0 && e->clearance.epoch != e->map.epoch) ? 1 : 0;
  return RNA_OK;
}
