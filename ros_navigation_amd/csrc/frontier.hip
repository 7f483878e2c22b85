// frontier.hip -- exploration frontiers: where the known free space of the master layer ends, clustered and ranked.
// The goal source of a robot that maps while it drives (navfn / costmap_2d users run frontier exploration on top of the
// planner): a goal field rooted at the robot is the travel cost to every cell, one lookup per frontier cell ranks every
// frontier, rna_goal_field_paths from the chosen cell, reversed, is the plan to it.
//
// Definitions (include/rna.h has the full text), map space throughout, integers and bit tests only:
//   unknown(c) = master[c] is NaN;  free(c) = !unknown(c) and c is not in the search's blocked set (robot radius included);
//   frontier(c) = free(c) and one of c's four edge neighbours inside the map is unknown;  cluster = 8-connected component of
//   frontier cells;  label = smallest BUFFER linear index of the cluster.
//
// At most six launches whatever the map holds (three when there is no frontier cell), none of which waits for another workgroup:
//   1. fr_classify_kernel   one workgroup per 64 x 64 map-space tile: frontier bits, the tile's components by row runs +
//                           union-find in LDS, labels = parent pointers (buffer indices) inside the tile, -1 off-frontier
//   2. fr_seam_kernel       frontier cells on a tile's border: union with the frontier neighbours in adjacent tiles, a
//                           lock-free union-find in global memory in which the smaller index always wins
//   3. fr_flatten_kernel    every frontier cell stores its root; roots take an entry of the record array
//   4. fr_init_kernel / fr_stats_kernel / fr_compact_kernel   size, bounding box, sums, ranking; the size filter
// Every find and every union has a stated bound; a build that exceeds one sets a control word and returns RNA_ECAPACITY.
#include "engine.hpp"
#include "map_tiles_dev.hpp"

#include <algorithm>
#include <climits>
#include <vector>

using namespace rna;

namespace {

typedef unsigned long long u64;

struct FrCtl {
  int cells;      // frontier cells
  int roots;      // clusters (entries of rec handed out)
  int kept;       // clusters that passed the size filter
  int largest;    // size of the largest cluster
  int overflow;   // a loop ran into its bound, or a root without a valid entry: the build is void
  int pad[3];
};

constexpr int FR_CELLS = TILE * TILE;

// ---- union-find in LDS: node ids are tile-local and ordered like the buffer indices of their cells (see the kernel) ----
// a path visits a node once (parents are strictly smaller): at most FR_CELLS reads
__device__ __forceinline__ int fr_lds_find(int* parent, int a, int* overflow) {
  for (int k = 0; k < FR_CELLS; ++k) {
    const int p = __hip_atomic_load(&parent[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == a) return a;
    a = p;
  }
  *overflow = 1;
  return a;
}

// find both roots, atomicMin the larger root onto the smaller; when the larger one had stopped being a root the old parent
// it returns still has to be joined with the smaller: the larger of the pair strictly decreases, at most FR_CELLS turns
__device__ __forceinline__ void fr_lds_union(int* parent, int a, int b, int* overflow) {
  for (int k = 0; k < FR_CELLS; ++k) {
    a = fr_lds_find(parent, a, overflow);
    b = fr_lds_find(parent, b, overflow);
    if (a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicMin(&parent[hi], lo);
    if (old == hi) return;
    a = old;
    b = lo;
  }
  *overflow = 1;
}

// ---- the same in global memory over buffer linear indices; every read of a parent is an agent-scope load, every write an
// atomicMin, so a stale read costs a step and never an answer.  Bounds: a path <= ncell reads, a union <= ncell turns ----
__device__ __forceinline__ int fr_find(int32_t* lab, int a, int ncell, FrCtl* ctl) {
  for (int k = 0; k < ncell; ++k) {
    const int p = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == a) return a;
    if (p < 0 || p > a) break;   // not a parent pointer: a defect, reported
    a = p;
  }
  atomicOr(&ctl->overflow, 1);
  return -1;
}

__device__ __forceinline__ void fr_union(int32_t* lab, int a, int b, int ncell, FrCtl* ctl) {
  for (int k = 0; k < ncell; ++k) {
    a = fr_find(lab, a, ncell, ctl);
    b = fr_find(lab, b, ncell, ctl);
    if (a < 0 || b < 0 || a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicMin(&lab[hi], lo);
    if (old == hi) return;
    if (old < 0) break;
    a = old;
    b = lo;
  }
  atomicOr(&ctl->overflow, 1);
}

}  // namespace

// One workgroup per 64 x 64 tile (MAP space; (s0, s1) = buffer start index), 256 threads:
//  1. unknown bits of the tile's rows with one row above and below (window_rows_each, a ballot per 64 cells of master) and
//     of the column on either side (a ballot over the rows); free bits of the tile: known and not blocked -- the footprint's
//     bits with a robot radius (`bits`, 64 x 64 per map-space tile), cell_blocked of master without one.  Outside the map
//     no bit is set.
//  2. frontier word of a row = free & (unknown above | below | left | right).
//  3. node id of a cell = its tile-local index ROTATED by where the buffer wraps inside the tile (wi, wj), so that ids order
//     like buffer indices and the smallest id of a component is its label.  Every cell starts at the smallest id of its row
//     run (the run's first cell, or the cell the buffer wraps at); runs of adjacent rows that touch (also diagonally) are
//     joined by fr_lds_union.  Not a propagation to a fixpoint: a serpentine component costs its runs' unions, nothing more.
//  4. labels[c] = buffer index of the root's cell, -1 off-frontier; the tile's frontier cells are added to ctl->cells.
__global__ void __launch_bounds__(256) fr_classify_kernel(int32_t* __restrict__ labels, const u64* __restrict__ bits,
                                                          const float* __restrict__ master, FrCtl* __restrict__ ctl, int rows, int cols,
                                                          int s0, int s1) {
  __shared__ u64 unk[TILE + 2];    // row jj = map row j0 - 1 + jj, bit = column i0 + bit
  __shared__ u64 side[2];          // bit lj: the cell left (0) / right (1) of the tile in row j0 + lj is unknown
  __shared__ u64 fre[TILE];
  __shared__ u64 fr[TILE];
  __shared__ int parent[FR_CELLS];
  __shared__ int overflow;
  const int ti = blockIdx.x, tj = blockIdx.y, tiles_i = gridDim.x;
  const int i0 = ti * TILE, j0 = tj * TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) overflow = 0;
  window_rows_each<1>(master, i0, j0 - 1, TILE, TILE + 2, rows, cols, s0, s1, [&](int jj, int, bool ok, float v) {
    const u64 un = __ballot(ok && v != v);
    const u64 known = __ballot(ok && !(v != v));
    const u64 blk = __ballot(ok && cell_blocked(v));
    if (lane == 0) {
      unk[jj] = un;
      if (jj >= 1 && jj <= TILE) {
        const int lj = jj - 1;
        fre[lj] = known & ~(bits ? fp_bits_word(bits, tiles_i, cols, ti, j0 + lj) : blk);
      }
    }
  });
  if (wave < 2) {
    const int i = wave == 0 ? i0 - 1 : i0 + TILE, j = j0 + lane;
    const bool ok = i >= 0 && i < rows && j < cols;
    const float v = master[ok ? buffer_lin(i, j, rows, cols, s0, s1) : 0];
    const u64 un = __ballot(ok && v != v);
    if (lane == 0) side[wave] = un;
  }
  __syncthreads();
  if (threadIdx.x < TILE) {
    const int lj = threadIdx.x;
    const u64 u = unk[lj + 1];
    const u64 nb = unk[lj] | unk[lj + 2] | (u << 1) | ((side[0] >> lj) & 1ull) | (u >> 1) | (((side[1] >> lj) & 1ull) << 63);
    fr[lj] = fre[lj] & nb;
  }
  __syncthreads();
  // where the buffer wraps inside this tile: map column rows - s0 is buffer column 0 (likewise rows); 0 = not inside
  const int iw = s0 > 0 ? rows - s0 - i0 : 0, jw = s1 > 0 ? cols - s1 - j0 : 0;
  const int wi = iw > 0 && iw < TILE ? iw : 0, wj = jw > 0 && jw < TILE ? jw : 0;
#define FR_ID(li, lj) (((((lj) - wj) & (TILE - 1)) << 6) | (((li) - wi) & (TILE - 1)))
  for (int k = threadIdx.x; k < FR_CELLS; k += blockDim.x) {
    const int li = k & (TILE - 1), lj = k >> 6;
    const u64 w = fr[lj];
    if (!((w >> li) & 1ull)) continue;
    const u64 below = ~w & ((1ull << li) - 1ull);              // clear bits under li
    const int a = below ? 64 - __clzll((long long)below) : 0;  // the run's first cell
    const u64 above = ~(w >> li);                              // (bit 0 is clear: the cell itself)
    const int b = above ? li + __ffsll((long long)above) - 2 : TILE - 1;   // the run's last cell
    const int rep = (wi > a && wi <= b) ? wi : a;
    parent[FR_ID(li, lj)] = FR_ID(rep, lj);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FR_CELLS; k += blockDim.x) {
    const int li = k & (TILE - 1), lj = k >> 6;
    if (lj == 0 || !((fr[lj] >> li) & 1ull)) continue;
    const u64 up = fr[lj - 1];
    const int me = FR_ID(li, lj);
    if ((up >> li) & 1ull) {
      fr_lds_union(parent, me, FR_ID(li, lj - 1), &overflow);   // (its row neighbours belong to the same run)
    } else {
      if (li > 0 && ((up >> (li - 1)) & 1ull)) fr_lds_union(parent, me, FR_ID(li - 1, lj - 1), &overflow);
      if (li < TILE - 1 && ((up >> (li + 1)) & 1ull)) fr_lds_union(parent, me, FR_ID(li + 1, lj - 1), &overflow);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FR_CELLS; k += blockDim.x) {
    const int li = k & (TILE - 1), lj = k >> 6;
    const int i = i0 + li, j = j0 + lj;
    if (i >= rows || j >= cols) continue;
    int32_t out = -1;
    if ((fr[lj] >> li) & 1ull) {
      const int r = fr_lds_find(parent, FR_ID(li, lj), &overflow);
      const int ri = i0 + (((r & (TILE - 1)) + wi) & (TILE - 1)), rj = j0 + (((r >> 6) + wj) & (TILE - 1));
      out = buffer_lin<int>(ri, rj, rows, cols, s0, s1);
    }
    labels[buffer_lin(i, j, rows, cols, s0, s1)] = out;
  }
#undef FR_ID
  if (wave == 0) {
    const int n = wave_sum(__popcll(fr[lane]));
    if (lane == 0 && n) atomicAdd(&ctl->cells, n);
  }
  __syncthreads();
  if (threadIdx.x == 0 && overflow) atomicOr(&ctl->overflow, 1);
}

// One workgroup per tile, a thread per border cell (252 of them): a frontier cell is joined with every frontier neighbour
// (all eight directions: the tile-corner diagonal included) that lies in a tile of a HIGHER number -- each pair once.
__global__ void __launch_bounds__(256) fr_seam_kernel(int32_t* __restrict__ labels, FrCtl* __restrict__ ctl, int rows, int cols, int s0, int s1,
                                                      int ncell) {
  const int ti = blockIdx.x, tj = blockIdx.y, tiles_i = gridDim.x;
  const int k = threadIdx.x;
  int li, lj;
  if (k < 64) { li = k; lj = 0; }
  else if (k < 128) { li = k - 64; lj = TILE - 1; }
  else if (k < 190) { li = 0; lj = k - 127; }
  else if (k < 252) { li = TILE - 1; lj = k - 189; }
  else return;
  const int i = ti * TILE + li, j = tj * TILE + lj;
  if (i >= rows || j >= cols) return;
  const int c = buffer_lin<int>(i, j, rows, cols, s0, s1);
  if (labels[c] < 0) return;
  const int tile = tj * tiles_i + ti;
  for (int dj = -1; dj <= 1; ++dj)
    for (int di = -1; di <= 1; ++di) {
      const int ni = i + di, nj = j + dj;
      if ((!di && !dj) || ni < 0 || nj < 0 || ni >= rows || nj >= cols) continue;
      if ((nj >> 6) * tiles_i + (ni >> 6) <= tile) continue;
      const int n = buffer_lin<int>(ni, nj, rows, cols, s0, s1);
      if (__hip_atomic_load(&labels[n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
      fr_union(labels, c, n, ncell, ctl);
    }
}

// Every frontier cell stores its root (the cluster's smallest buffer index, by construction of the unions); a root takes
// the next entry of the record array and leaves its number in slot[root].
__global__ void __launch_bounds__(256) fr_flatten_kernel(int32_t* __restrict__ labels, int32_t* __restrict__ slot, FrCtl* __restrict__ ctl,
                                                         int ncell) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += stride) {
    const int l = __hip_atomic_load(&labels[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (l < 0) continue;
    const int r = fr_find(labels, (int)c, ncell, ctl);
    if (r < 0) continue;
    if (r != l) __hip_atomic_store(&labels[c], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (still an ancestor for a find that passes by)
    if (r == (int)c) slot[c] = atomicAdd(&ctl->roots, 1);
  }
}

__global__ void __launch_bounds__(256) fr_init_kernel(rna_frontier* __restrict__ rec, int n) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  rna_frontier r;
  r.label = -1;
  r.size = 0;
  r.min_i = r.min_j = INT_MAX;
  r.max_i = r.max_j = -1;
  r.nearest = -1;   // (nearest, cost) is one 64-bit word, cost on top: all ones = larger than any (cost, cell)
  r.cost = -1;
  r.sum_i = r.sum_j = 0;
  rec[k] = r;
}

// Size, bounding box, sums and the ranking minimum of every cluster: integer atomics only (the result does not depend on
// arrival order), after the lanes of a wavefront that share a root have been combined (at most 64 turns: each retires a lane).
__global__ void __launch_bounds__(256) fr_stats_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ slot,
                                                       rna_frontier* __restrict__ rec, int n_rec, const int32_t* __restrict__ field,
                                                       FrCtl* __restrict__ ctl, int rows, int cols, int s0, int s1, int ncell) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long base = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < ncell; base += stride) {
    const long long c = base + lane;
    const int l = c < ncell ? labels[c] : -1;
    const bool is_fr = l >= 0;
    u64 pend = __ballot(is_fr);
    if (!pend) continue;   // (uniform)
    int i, j;
    map_cell_of(c, rows, cols, s0, s1, i, j);
    // (cost, cell) as one unsigned word, cost on top: the order of the raw int32 because a goal-field value is never negative
    // (a distance, RNA_GOAL_FIELD_FAR or RNA_GOAL_FIELD_UNREACHED)
    const u64 key = (field && is_fr) ? ((u64)(unsigned)field[c] << 32) | (unsigned)c : ~0ull;
    for (int turn = 0; pend && turn < 64; ++turn) {
      const int leader = __ffsll((long long)pend) - 1;
      const int r = __shfl(l, leader, 64);
      const bool mine = is_fr && l == r;
      const u64 m = __ballot(mine);
      pend &= ~m;
      int mn_i = mine ? i : INT_MAX, mx_i = mine ? i : -1, mn_j = mine ? j : INT_MAX, mx_j = mine ? j : -1;
      long long si = mine ? i : 0, sj = mine ? j : 0;
      u64 best = mine ? key : ~0ull;
      for (int o = 32; o; o >>= 1) {
        mn_i = min(mn_i, __shfl_xor(mn_i, o, 64));
        mx_i = max(mx_i, __shfl_xor(mx_i, o, 64));
        mn_j = min(mn_j, __shfl_xor(mn_j, o, 64));
        mx_j = max(mx_j, __shfl_xor(mx_j, o, 64));
        si += __shfl_xor(si, o, 64);
        sj += __shfl_xor(sj, o, 64);
        const u64 other = __shfl_xor(best, o, 64);
        best = other < best ? other : best;
      }
      if (lane == leader) {
        const int s = slot[r];
        if ((unsigned)s >= (unsigned)n_rec) {
          atomicOr(&ctl->overflow, 1);   // a root without an entry: a defect, reported
        } else {
          rna_frontier* R = &rec[s];
          atomicAdd(&R->size, __popcll(m));
          atomicMin(&R->min_i, mn_i);
          atomicMax(&R->max_i, mx_i);
          atomicMin(&R->min_j, mn_j);
          atomicMax(&R->max_j, mx_j);
          atomicAdd(reinterpret_cast<u64*>(&R->sum_i), (u64)si);
          atomicAdd(reinterpret_cast<u64*>(&R->sum_j), (u64)sj);
          if (field) atomicMin(reinterpret_cast<u64*>(&R->nearest), best);
        }
      }
      if (mine && (long long)r == c) {
        const int s = slot[r];
        if ((unsigned)s < (unsigned)n_rec) rec[s].label = r;
      }
    }
  }
}

// the size filter: clusters of at least min_size cells take an entry of `out` (arrival order; the host sorts by label)
__global__ void __launch_bounds__(256) fr_compact_kernel(const rna_frontier* __restrict__ rec, int n, int min_size, int ranked,
                                                         rna_frontier* __restrict__ out, FrCtl* __restrict__ ctl) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  rna_frontier r = rec[k];
  atomicMax(&ctl->largest, r.size);
  if (r.size < min_size) return;
  if (!ranked) {
    r.nearest = r.label;
    r.cost = RNA_GOAL_FIELD_UNREACHED;
  }
  out[atomicAdd(&ctl->kept, 1)] = r;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace rna {

int frontiers_release(rna_engine* e) {
  Frontiers& f = e->frontiers;
  dev_free(&f.labels);
  dev_free(&f.slot);
  dev_free(&f.rec);
  dev_free(&f.out);
  f.rec_cap = 0;
  f.ctl.release();
  f.built = false;
  f.info = rna_frontier_info{0, 0, 0, 0, 0, 0, 0, 0};
  return RNA_OK;
}

}  // namespace rna

namespace {

int fr_alloc(rna_engine* e) {
  Frontiers& f = e->frontiers;
  if (f.labels) return RNA_OK;
  int rc = dev_alloc(e, &f.labels, e->ncell);
  if (rc == RNA_OK) rc = dev_alloc(e, &f.slot, e->ncell);
  if (rc == RNA_OK) rc = f.ctl.alloc(e);
  if (rc != RNA_OK) {
    const std::string msg = e->err;
    frontiers_release(e);
    e->err = msg;
  }
  return rc;
}

}  // namespace

extern "C" int rna_frontiers_build(rna_engine* e, int min_size, unsigned flags, rna_frontier* out_host, int cap,
                                   rna_frontier_info* info_host) {
  // (argument checks first: none of them reads the engine)
  if (!e || min_size < 1 || cap < 0 || (flags & ~(unsigned)RNA_FRONTIER_RANK) || (cap > 0 && !out_host)) return RNA_EINVAL;
  const bool rank = (flags & RNA_FRONTIER_RANK) != 0;
  if (rank && (e->gfield.info.goal < 0 || e->gfield.epoch != e->map.epoch || e->gfield.cost_changed))
    return fail(e, RNA_ESTATE, "rna_frontiers_build: RNA_FRONTIER_RANK needs a current goal field (rna_goal_field_build)");
  if (e->ncell > (size_t)INT_MAX) return fail(e, RNA_ECAPACITY, "rna_frontiers_build: a label is an int32, the map has 2^31 cells or more");
  RNA_ENTER(e);
  int rc = map_prepare_nbr(e);   // (with a robot radius: the footprint's blocked bits are current)
  if (rc != RNA_OK) return rc;
  if ((rc = fr_alloc(e)) != RNA_OK) return rc;
  Frontiers& f = e->frontiers;
  f.built = false;   // (no snapshot while this one is being built, also when the build fails)
  f.info = rna_frontier_info{0, 0, 0, 0, 0, 0, 0, 0};
  const Geom& g = e->geom;
  const int rows = g.size[0], cols = g.size[1], s0 = g.start[0], s1 = g.start[1], ncell = (int)e->ncell;
  FrCtl* const ctl = f.ctl.dev;
  const FrCtl* const host = f.ctl.host;
  const dim3 tiles(e->tiles_i, e->tiles_j);
  const unsigned cell_blocks = (unsigned)std::min<size_t>((e->ncell + 255) / 256, 8192);
  RNA_HIP(e, hipMemsetAsync(ctl, 0, sizeof(FrCtl), e->stream));
  hipLaunchKernelGGL(fr_classify_kernel, tiles, dim3(256), 0, e->stream, f.labels, e->robot_r > 0.0 ? e->fp_bits : (const u64*)nullptr,
                     e->layer[RNA_LAYER_MASTER], ctl, rows, cols, s0, s1);
  hipLaunchKernelGGL(fr_seam_kernel, tiles, dim3(256), 0, e->stream, f.labels, ctl, rows, cols, s0, s1, ncell);
  hipLaunchKernelGGL(fr_flatten_kernel, dim3(cell_blocks), dim3(256), 0, e->stream, f.labels, f.slot, ctl, ncell);
  if ((rc = f.ctl.read(e)) != RNA_OK) return rc;
  if (host->overflow) return fail(e, RNA_ECAPACITY, "rna_frontiers_build: a union-find loop exceeded its bound");
  const int roots = host->roots;
  if (roots > f.rec_cap) {   // (no kernel in flight reads the records: a build returns when it is complete)
    const int want = std::max(roots, 1024);
    f.rec_cap = 0;
    if ((rc = dev_alloc(e, &f.rec, (size_t)want)) != RNA_OK) return rc;
    if ((rc = dev_alloc(e, &f.out, (size_t)want)) != RNA_OK) return rc;
    f.rec_cap = want;
  }
  if (roots > 0) {
    const unsigned rec_blocks = (unsigned)((roots + 255) / 256);
    hipLaunchKernelGGL(fr_init_kernel, dim3(rec_blocks), dim3(256), 0, e->stream, f.rec, roots);
    hipLaunchKernelGGL(fr_stats_kernel, dim3(cell_blocks), dim3(256), 0, e->stream, f.labels, f.slot, f.rec, roots,
                       rank ? e->gfield.field : (const int32_t*)nullptr, ctl, rows, cols, s0, s1, ncell);
    hipLaunchKernelGGL(fr_compact_kernel, dim3(rec_blocks), dim3(256), 0, e->stream, f.rec, roots, min_size, rank ? 1 : 0, f.out, ctl);
    if ((rc = f.ctl.read(e)) != RNA_OK) return rc;
    if (host->overflow) return fail(e, RNA_ECAPACITY, "rna_frontiers_build: a cluster root without a record");
  }
  f.info = rna_frontier_info{host->cells, roots, host->kept, host->largest, min_size, rank ? 1 : 0, 0, 0};
  f.epoch = e->map.epoch;
  f.built = true;
  if (info_host) *info_host = f.info;
  if (cap == 0) return RNA_OK;
  if (host->kept > cap)
    return fail(e, RNA_ECAPACITY, "rna_frontiers_build: " + std::to_string(host->kept) + " clusters, room for " + std::to_string(cap));
  if (host->kept > 0) {
    std::vector<rna_frontier> recs((size_t)host->kept);
    RNA_HIP(e, hipMemcpyAsync(recs.data(), f.out, recs.size() * sizeof(rna_frontier), hipMemcpyDeviceToHost, e->stream));
    RNA_HIP(e, hipStreamSynchronize(e->stream));
    std::sort(recs.begin(), recs.end(), [](const rna_frontier& a, const rna_frontier& b) { return a.label < b.label; });
    std::copy(recs.begin(), recs.end(), out_host);
  }
  return RNA_OK;
}

extern "C" int rna_frontiers_info_get(const rna_engine* e, rna_frontier_info* out) {
  if (!e || !out) return RNA_EINVAL;
  *out = e->frontiers.info;
  out->stale = (e->frontiers.built && e->frontiers.epoch != e->map.epoch) ? 1 : 0;
  return RNA_OK;
}

extern "C" int rna_frontiers_download(rna_engine* e, int32_t* labels_host, size_t n_cells) {
  if (!e || !labels_host || n_cells != e->ncell) return RNA_EINVAL;
  if (!e->frontiers.built) return fail(e, RNA_ESTATE, "rna_frontiers_download: no frontiers have been built");
  RNA_ENTER_NOJOIN(e);
  RNA_HIP(e, hipMemcpyAsync(labels_host, e->frontiers.labels, n_cells * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  RNA_HIP(e, hipStreamSynchronize(e->stream));
  return RNA_OK;
}

extern "C" void* rna_frontiers_device_ptr(rna_engine* e) { return (e && e->frontiers.built) ? (void*)e->frontiers.labels : nullptr; }
