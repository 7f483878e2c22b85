// footprint.hip -- the robot radius of the grid A*: GlobalPlanner::ifBlocked's disc as the search's blocked set.
// Reference call sites restated (mc/ = move_control, gmc/ = grid_map-master/grid_map_core):
//   GlobalPlanner::ifBlocked          mc/include/move_control/map_global_planner.h:39-54
//   CircleIterator                    gmc/src/iterators/CircleIterator.cpp:16-93 (isInside :74-79, bounding box :82-91)
//
// With a radius r > 0 a cell c is blocked for the search iff some cell CircleIterator(map, getPosition(c), r) visits holds
// a finite master value > 0.  footprint_tiles_kernel computes that set for 64 x 64 tiles by dilating the tile's occupancy
// bits with the disc stencil of FootprintPlan, and the neighbour masks from it by the rule of nbr_mask_tiles_kernel (nbr_mask_of).
// Why the dilation is exact (DESIGN.md "Robot radius"): the stencil's sure-in / sure-out offsets are decided with a margin
// that bounds the rounding of the reference's f64 cell-centre arithmetic; the few offsets inside the margin (ties, e.g.
// (6, 0) for 0.3 m at 0.05 m) are evaluated per cell with the reference's own expressions; and every cell near the map
// edge computes its bounding box as the reference does and, where that box is not the plain one, runs the whole
// procedure (disc_blocked) instead.
#include "engine.hpp"
#include "map_tiles_dev.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace rna;

namespace {

constexpr int FP_MAX_R = 63;                  // r / res <= 63: a changed tile affects cells of its one-tile ring only
constexpr int FP_ROWS = TILE + 2 * (FP_MAX_R + 1);   // occupancy rows of a workgroup (halo R + 1 on each side)
constexpr int FP_BLK = TILE + 2;              // blocked bytes of a workgroup: the tile with a 1-cell ring

// GlobalPlanner::ifBlocked at (px, py) with `radius`, the whole procedure, one thread: the bounding box of CircleIterator
// (limitPositionToRange + getIndexFromPosition of both corners, CircleIterator.cpp:82-91), then every box cell whose
// centre passes isInside (dx^2 + dy^2 <= r^2 from f64 cell-centre positions, :74-79).  The same walk as planners.hip's
// wave_if_blocked (whose 0.3 m form rrt_kernel runs), serial and with the radius as a parameter: a corner that fails
// getIndexFromPosition leaves index (0, 0); a non-positive box visits its first cell; an index past an unmoved map's edge
// is skipped (oracle/gridmath.c og_circle_cells, oracle/rrt.c og_if_blocked).
__device__ bool disc_blocked(const Geom& g, const float* __restrict__ master, double px, double py, double radius) {
  const double r2 = radius * radius;   // pow(radius, 2)
  double tl[2] = {px + radius, py + radius}, br[2] = {px - radius, py - radius};
  limit_position_to_range(g, tl);
  limit_position_to_range(g, br);
  int s[2] = {0, 0}, t[2] = {0, 0};
  (void)index_from_position(g, tl[0], tl[1], s);
  (void)index_from_position(g, br[0], br[1], t);
  int su[2], tu[2];
  unwrap_index(g, s, su);
  unwrap_index(g, t, tu);
  const bool whole = (tu[0] - su[0] + 1) > 0 && (tu[1] - su[1] + 1) > 0;
  const int ni = whole ? tu[0] - su[0] + 1 : 1, nj = whole ? tu[1] - su[1] + 1 : 1;
  const double ox = g.pos[0] + (0.5 * g.len[0] - 0.5 * g.res), oy = g.pos[1] + (0.5 * g.len[1] - 0.5 * g.res);
  for (int row = 0; row < nj; ++row)
    for (int col = 0; col < ni; ++col) {
      const int u[2] = {su[0] + col, su[1] + row};
      int bi[2];
      buffer_index(g, u, bi);
      if ((unsigned)bi[0] >= (unsigned)g.size[0] || (unsigned)bi[1] >= (unsigned)g.size[1]) continue;
      const int w0 = (unsigned)u[0] < (unsigned)g.size[0] ? u[0] : wrap_index(u[0], g.size[0]);
      const int w1 = (unsigned)u[1] < (unsigned)g.size[1] ? u[1] : wrap_index(u[1], g.size[1]);
      const double dx = (ox + g.res * (double)(-w0)) - px, dy = (oy + g.res * (double)(-w1)) - py;
      if (!(dx * dx + dy * dy <= r2)) continue;
      if (cell_blocked(master[(size_t)bi[1] * g.size[0] + bi[0]])) return true;
    }
  return false;
}

// The unwrapped bounding box CircleIterator takes for the centre of map-space cell (i, j) covers every in-map cell the
// stencil does not rule out, [max(0, i - K), min(rows - 1, i + K)] x [..j..] (K = FootprintPlan::K): then the visited
// cells that pass isInside are exactly the stencil's in-map ones
__device__ bool box_is_plain(const Geom& g, double px, double py, double radius, int i, int j, int K) {
  double tl[2] = {px + radius, py + radius}, br[2] = {px - radius, py - radius};
  limit_position_to_range(g, tl);
  limit_position_to_range(g, br);
  int s[2] = {0, 0}, t[2] = {0, 0};
  (void)index_from_position(g, tl[0], tl[1], s);
  (void)index_from_position(g, br[0], br[1], t);
  int su[2], tu[2];
  unwrap_index(g, s, su);
  unwrap_index(g, t, tu);
  const int lo0 = i - K < 0 ? 0 : i - K, hi0 = i + K > g.size[0] - 1 ? g.size[0] - 1 : i + K;
  const int lo1 = j - K < 0 ? 0 : j - K, hi1 = j + K > g.size[1] - 1 ? g.size[1] - 1 : j + K;
  return su[0] >= 0 && su[0] <= lo0 && tu[0] >= hi0 && tu[0] < g.size[0] && su[1] >= 0 && su[1] <= lo1 && tu[1] >= hi1 &&
         tu[1] < g.size[1];
}

}  // namespace

// One workgroup per 64 x 64 tile (MAP space, unwrapped indices; (s0, s1) = buffer start index, as nbr_mask_tiles_kernel):
//  1. occupancy bits (cell_blocked of master; outside the map 0 = not visited) of the tile with a halo of R + 1 cells into
//     LDS: row jj = map row j0 - H + jj, 4 words of bits for the map cells i0 - 64 .. i0 + 191 (word 3 stays 0);
//  2. the blocked byte of every cell of the tile and its 1-cell ring (outside the map: blocked, for the moves): the OR over
//     the stencil rows dj of "a bit within [i - w(dj), i + w(dj)] of row j + dj" (two 64-bit windows around the cell),
//     then the tie offsets in f64, then -- near the map edge -- the bounding-box check and, where it fails, disc_blocked;
//  3. the tile's blocked bits and its cells' 8-bit neighbour masks (nbr_mask_of).
// `all` != 0: every tile; otherwise only tiles that are dirty or touch a dirty tile (unmoved map).
__global__ void __launch_bounds__(256) footprint_tiles_kernel(uint8_t* __restrict__ nbr, unsigned long long* __restrict__ bits,
                                                              const float* __restrict__ master, const unsigned* __restrict__ dirty,
                                                              int all, Geom g, FootprintPlan P, const int2* __restrict__ ties) {
  const int ti = blockIdx.x, tj = blockIdx.y;
  const int tiles_i = gridDim.x, tiles_j = gridDim.y;
  const int rows = g.size[0], cols = g.size[1];
  if (!all && !dirty_ring(dirty, ti, tj, tiles_i, tiles_j)) return;
  __shared__ unsigned long long occ[FP_ROWS][4];
  __shared__ uint8_t blk[FP_BLK * FP_BLK];
  const int R = P.R, H = R + 1;
  const int i0 = ti * TILE, j0 = tj * TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  occ_rows_load(occ, master, i0, j0, H, rows, cols, g.start[0], g.start[1]);   // 1. (map_tiles_dev.hpp)
  __syncthreads();
  // 2. blocked bytes of the tile and its ring
  const double ox = g.pos[0] + (0.5 * g.len[0] - 0.5 * g.res), oy = g.pos[1] + (0.5 * g.len[1] - 0.5 * g.res);
  const double r2 = P.r * P.r;
  for (int k = threadIdx.x; k < FP_BLK * FP_BLK; k += blockDim.x) {
    const int li = k % FP_BLK - 1, lj = k / FP_BLK - 1;
    const int i = i0 + li, j = j0 + lj;
    uint8_t out = 1;
    if (i >= 0 && j >= 0 && i < rows && j < cols) {
      const int p = li + 64;                    // the cell's bit in its occupancy row (63 .. 128)
      const int jc = lj + H;                    // the cell's occupancy row
      bool hit = false;
      for (int dj = -R; dj <= R; ++dj) {
        const int w = P.w[dj < 0 ? -dj : dj];
        if (w < 0) continue;
        unsigned long long lo, hi;
        occ_windows(occ[jc + dj], p, lo, hi);
        if ((lo >> (63 - w)) | (hi << (63 - w))) hit = true;
      }
      const double px = ox + g.res * (double)(-i), py = oy + g.res * (double)(-j);
      for (int t = 0; t < P.n_ties && !hit; ++t) {
        const int2 d = ties[t];
        const int b = p + d.x;
        if (!((occ[jc + d.y][b >> 6] >> (b & 63)) & 1ull)) continue;
        const double dx = (ox + g.res * (double)(-(i + d.x))) - px, dy = (oy + g.res * (double)(-(j + d.y))) - py;
        if (dx * dx + dy * dy <= r2) hit = true;
      }
      if (i < P.band || j < P.band || i >= rows - P.band || j >= cols - P.band) {
        if (!box_is_plain(g, px, py, P.r, i, j, P.K)) hit = disc_blocked(g, master, px, py, P.r);
      }
      out = hit ? 1 : 0;
    }
    blk[k] = out;
  }
  __syncthreads();
  // 3. blocked bits (a wavefront per tile row) and neighbour masks
  for (int lj = wave; lj < TILE; lj += 4) {
    const int i = i0 + lane, j = j0 + lj;
    const bool b = i < rows && j < cols && blk[(lj + 1) * FP_BLK + lane + 1];
    const unsigned long long m = __ballot(b);
    if (lane == 0) bits[fp_bits_index(tiles_i, ti, j)] = m;
  }
  for (int k = threadIdx.x; k < TILE * TILE; k += blockDim.x) {
    const int li = k & (TILE - 1), lj = k >> 6;
    const int i = i0 + li, j = j0 + lj;
    if (i >= rows || j >= cols) continue;
    nbr[buffer_lin(i, j, rows, cols, g.start[0], g.start[1])] = (uint8_t)nbr_mask_of(&blk[(lj + 1) * FP_BLK + (li + 1)], FP_BLK);
  }
}

// the blocked set in buffer order, one byte per cell: r > 0 from the tile bits, r == 0 from master
__global__ void blocked_bytes_kernel(uint8_t* __restrict__ out, const unsigned long long* __restrict__ bits, const float* __restrict__ master,
                                     int rows, int cols, int tiles_i, int s0, int s1) {
  const size_t n = (size_t)rows * cols;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
    if (!bits) { out[k] = cell_blocked(master[k]) ? 1 : 0; continue; }
    int i, j;
    map_cell_of(k, rows, cols, s0, s1, i, j);
    out[k] = fp_bit(bits, tiles_i, cols, i, j) ? 1 : 0;
  }
}

// rna_if_blocked_batch: one thread per position
__global__ void if_blocked_kernel(const double* __restrict__ xy, int n, double radius, Geom g, const float* __restrict__ master,
                                  uint8_t* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  out[k] = disc_blocked(g, master, xy[2 * k], xy[2 * k + 1], radius) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace {

// Largest magnitude of a coordinate the reference's cell-centre / corner arithmetic meets on this geometry
double geometry_magnitude(const Geom& g, double r) {
  return fmax(fabs(g.pos[0]), fabs(g.pos[1])) + fmax(g.len[0], g.len[1]) + r + g.res;
}

// The stencil of radius r for coordinates up to `mag` (DESIGN.md "Robot radius"): every quantity of the reference's
// disc test -- a cell centre ox + res * (-u), a difference of two of them, its square -- is computed within a few ulps of
// mag; eta = 2^-48 mag bounds the error of a centre difference dx (four roundings of at most 2^-53 mag each, eightfold).
// The computed dx^2 + dy^2 then lies within m = 8 D eta + 2^-45 (D^2 + r^2) of (di^2 + dj^2) res^2, D the stencil's
// largest offset: an offset whose nominal distance is farther than m from r^2 decides the same way in every cell.
FootprintPlan make_plan(const Geom& g, double r, double mag, std::vector<int2>& ties) {
  FootprintPlan P;
  P.r = r;
  P.res = g.res;
  P.mag = mag;
  // (r <= 63 res; r / res may round to just above an integer: offset R + 1 is then still a whole cell outside the disc)
  P.R = std::min((int)ceil(r / g.res), FP_MAX_R);
  const double eta = ldexp(mag, -48);
  const double D = 1.5 * (P.R + 1) * g.res;
  const double m = 8.0 * D * eta + ldexp(D * D + r * r, -45);
  const double r2 = r * r, res2 = g.res * g.res;
  ties.clear();
  for (int dj = 0; dj <= FP_MAX_R; ++dj) P.w[dj] = -1;
  for (int dj = -P.R; dj <= P.R; ++dj)
    for (int di = -P.R; di <= P.R; ++di) {
      const double nom = (double)(di * di + dj * dj) * res2;
      if (nom - m > r2) continue;   // sure-out
      if (nom + m < r2) {           // sure-in
        const int a = dj < 0 ? -dj : dj;
        if (di > P.w[a]) P.w[a] = di;
      } else {
        ties.push_back(make_int2(di, dj));
      }
      P.K = std::max(P.K, std::max(di < 0 ? -di : di, dj < 0 ? -dj : dj));
    }
  P.n_ties = (int)ties.size();
  // The bounding box of a cell centre at least R + 1 cells from the edge is the plain one when the roundings of its corner
  // (a dozen operations on values up to mag) stay below a quarter cell: 16 eta < res.  Otherwise every cell checks its box.
  P.band = 16.0 * eta < g.res ? P.R + 1 : (1 << 30);
  return P;
}

}  // namespace

namespace rna {

int footprint_release(rna_engine* e) {
  dev_free(&e->fp_bits);
  dev_free(&e->fp_ties);
  e->fp_ties_cap = 0;
  return RNA_OK;
}

int footprint_refresh(rna_engine* e, int all) {
  const Geom& g = e->geom;
  if (!e->fp_bits) {
    const int rc = dev_alloc(e, &e->fp_bits, (size_t)e->tiles_i * e->tiles_j * TILE);
    if (rc != RNA_OK) return rc;
    all = 1;
  }
  const double mag = geometry_magnitude(g, e->robot_r);
  if (e->fp.r != e->robot_r || e->fp.res != g.res || mag > e->fp.mag) {
    std::vector<int2> ties;
    const FootprintPlan P = make_plan(g, e->robot_r, 2.0 * mag, ties);   // (twice the magnitude: moves need no new plan soon)
    RNA_HIP(e, hipStreamSynchronize(e->stream));                          // a refresh in flight may read the old ties
    if ((int)ties.size() > e->fp_ties_cap) {
      const int rc = dev_alloc(e, &e->fp_ties, ties.size());
      if (rc != RNA_OK) { e->fp_ties_cap = 0; return rc; }
      e->fp_ties_cap = (int)ties.size();
    }
    if (!ties.empty()) RNA_HIP(e, hipMemcpy(e->fp_ties, ties.data(), ties.size() * sizeof(int2), hipMemcpyHostToDevice));
    e->fp = P;
  }
  KernelTimer kt(e, RNA_K_FOOTPRINT);
  hipLaunchKernelGGL(footprint_tiles_kernel, dim3(e->tiles_i, e->tiles_j), dim3(256), 0, e->stream, e->nbr, e->fp_bits,
                     e->layer[RNA_LAYER_MASTER], e->dirty_tiles, all, g, e->fp, e->fp_ties);
  RNA_HIP(e, hipGetLastError());
  return RNA_OK;
}

}  // namespace rna

extern "C" int rna_astar_set_robot_radius(rna_engine* e, double radius) {
  if (!e) return RNA_EINVAL;
  if (!(radius >= 0.0) || !(radius <= (double)FP_MAX_R * e->geom.res))   // (63 * res itself: r / res may round to just above 63)
    return fail(e, RNA_EINVAL, "robot radius must satisfy 0 <= r and r / resolution <= 63");
  RNA_ENTER(e);   // joins the snapshots in flight: they read the masks the next refresh rebuilds
  e->robot_r = radius;
  e->map.radius_set();
  return RNA_OK;
}

extern "C" int rna_astar_get_robot_radius(const rna_engine* e, double* radius) {
  if (!e || !radius) return RNA_EINVAL;
  *radius = e->robot_r;
  return RNA_OK;
}

extern "C" int rna_astar_download_blocked(rna_engine* e, uint8_t* host, size_t n) {
  if (!e || !host || n != e->ncell) return RNA_EINVAL;
  RNA_ENTER(e);
  int rc = map_prepare_nbr(e);
  if (rc != RNA_OK) return rc;
  Staging st(e, "rna_astar_download_blocked");
  uint8_t* staging = st.out(host, n);
  const size_t blocks = std::min<size_t>((n + 255) / 256, 8192);
  if (st.ok())
    hipLaunchKernelGGL(blocked_bytes_kernel, dim3((unsigned)blocks), dim3(256), 0, e->stream, staging,
                       e->robot_r > 0.0 ? e->fp_bits : (const unsigned long long*)nullptr, e->layer[RNA_LAYER_MASTER], e->geom.size[0],
                       e->geom.size[1], e->tiles_i, e->geom.start[0], e->geom.start[1]);
  return st.finish();
}

static int if_blocked(rna_engine* e, const double* xy, int n, double radius, uint8_t* out, bool host) {
  if (!e || n < 0 || (n > 0 && (!xy || !out))) return RNA_EINVAL;
  if (!(radius >= 0.0) || !std::isfinite(radius)) return fail(e, RNA_EINVAL, "radius must be finite and >= 0");
  if (n == 0) return RNA_OK;
  RNA_ENTER(e);
  Staging st(e, "rna_if_blocked_batch");
  const double* d_xy = host ? st.in(xy, (size_t)n * 2) : xy;
  uint8_t* d_out = host ? st.out(out, (size_t)n) : out;
  if (st.ok())
    hipLaunchKernelGGL(if_blocked_kernel, dim3((n + 127) / 128), dim3(128), 0, e->stream, d_xy, n, radius, e->geom,
                       e->layer[RNA_LAYER_MASTER], d_out);
  return st.finish();
}

extern "C" int rna_if_blocked_batch(rna_engine* e, const double* xy_host, int n, double radius, uint8_t* out_host) {
  return if_blocked(e, xy_host, n, radius, out_host, true);
}

extern "C" int rna_if_blocked_batch_device(rna_engine* e, const double* xy_device, int n, double radius, uint8_t* out_device) {
  return if_blocked(e, xy_device, n, radius, out_device, false);
}
