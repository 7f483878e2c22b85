// viewgain.hip -- information gain of view points: what a sensor of range R cells would see from a candidate cell, by ray
// casting over the master layer.  The definition (include/rna.h) is a set, in map space, integers only:
//   opaque(c)  cell_blocked(master[c]) -- the RAW layer, no robot radius --, with RNA_VIEW_UNKNOWN_OPAQUE also master[c] NaN
//   ring of v  the 8R raw index pairs v + (a, b) with max(|a|, |b|) = R
//   ray to e   c_1 .. c_R of line(v, e) -- the reference's LineIterator(map, Index, Index), gridmath.hpp's closed form --: the
//              walk stops BEFORE a cell outside the map or with a^2 + b^2 > R^2, and AFTER a cell that is opaque
//   seen(v)    {v} and the cells the 8R rays see; the record counts seen, seen and unknown, seen and occupied
// A set does not depend on which thread walks which ray or in which order, so every output has exactly one right value.
#include "engine.hpp"
#include "map_tiles_dev.hpp"

#include <cstdlib>

using namespace rna;

using ViewGain = struct rna_view_gain;   // (the elaborated name: in C++ the entry point rna_view_gain hides the record's)

namespace {

constexpr int VG_U = 8;   // line cells a thread walks per division (gridmath.hpp's LineCursor)

// words of one bitmap row and of one bitmap of the (2R + 1)^2 window
inline int vg_row_words(int R) { return (2 * R + 1 + 31) / 32; }
inline size_t vg_lds_bytes(int R) { return (size_t)3 * (2 * R + 1) * vg_row_words(R) * sizeof(unsigned); }

}  // namespace

// One workgroup of 256 threads per view point; no workgroup waits for another, no global atomics.  LDS: three bitmaps over the
// window of W x W cells around v (W = 2R + 1), row wb = map row vj - R + wb, bit wa = map column vi - R + wa, NW 32-bit words
// per row: occupied, unknown, seen (3 x 255 x 8 x 4 B = 24 480 B at R = 127).
//  1. the window's rows are read as map_tiles_dev.hpp's window_rows_each reads them, one ballot per 64 cells and bitmap.
//     Cells outside the map hold no bit.  The seen bitmap starts with the bit of v alone.
//  2. the 8R rays are dealt to the threads: thread x takes the rays x, x + 256, ... of the list in which ray k ends at ring
//     position (k * stride) mod 8R, gcd(stride, 8R) = 1 (a bijection; stride 1 = neighbouring lanes walk neighbouring rays,
//     the host's other choice spreads a wavefront's lanes evenly round the ring: vg_stride below).  A thread walks in LDS only: per VG_U cells
//     one division (index_line_cursor), then the reference's numerator increments; a seen bit is one LDS atomic OR.  The
//     loops are bounded by R and by 8R / 256.
//  3. popcounts of seen, seen & unknown, seen & occupied, one reduction, one 16-byte record written by thread 0.
__global__ void __launch_bounds__(256) view_gain_kernel(const float* __restrict__ master, const int32_t* __restrict__ cells, int n, int R,
                                                        int stride, int unknown_opaque, ViewGain* __restrict__ out, int rows,
                                                        int cols, int s0, int s1) {
  extern __shared__ unsigned vg_bits[];   // occupied | unknown | seen
  __shared__ int vg_part[4][3];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (q >= n) return;
  const int W = 2 * R + 1, NW = (W + 31) >> 5, words = W * NW;
  unsigned* const occ = vg_bits;
  unsigned* const unk = vg_bits + words;
  unsigned* const seen = vg_bits + 2 * words;
  const int32_t c = cells[q];
  ViewGain r = {0, 0, 0, 0};
  if (!buffer_cell_in_range(c, rows, cols)) r.status = 1;
  else if (cell_blocked(master[c])) r.status = 2;
  if (r.status) {   // (uniform)
    if (tid == 0) out[q] = r;
    return;
  }
  int vi, vj;
  map_cell_of((unsigned)c, rows, cols, s0, s1, vi, vj);

  // ---- 1. the window's occupied and unknown bits ----
  window_rows_each<4>(master, vi - R, vj - R, W, W, rows, cols, s0, s1, [&](int wb, int p, bool ok, float v) {   // (W <= 255: 4 pieces)
    const unsigned long long mo = __ballot(ok && cell_blocked(v));
    const unsigned long long mu = __ballot(ok && v != v);
    const int w = wb * NW + 2 * p;
    if (lane == 0) { occ[w] = (unsigned)mo; unk[w] = (unsigned)mu; }
    if (lane == 1 && 2 * p + 1 < NW) { occ[w + 1] = (unsigned)(mo >> 32); unk[w + 1] = (unsigned)(mu >> 32); }
  });
  const int vw = R * NW + (R >> 5);
  for (int k = tid; k < words; k += 256) seen[k] = k == vw ? 1u << (R & 31) : 0u;
  __syncthreads();

  // ---- 2. the rays ----
  const int n_rays = 8 * R, RR = R * R;
  for (int k = tid; k < n_rays; k += 256) {
    const int p = (int)(((unsigned)k * (unsigned)stride) % (unsigned)n_rays);   // ring position, clockwise from (-R, -R)
    const int side = p / (2 * R), o = p - side * 2 * R;
    const int end[2] = {side == 0 ? o - R : (side == 1 ? R : (side == 2 ? R - o : -R)),
                        side == 0 ? -R : (side == 1 ? o - R : (side == 2 ? R : R - o))};
    const int zero[2] = {0, 0};
    const IndexLine ln = index_line(zero, end);   // (D == R: one of the two offsets has magnitude R)
    bool live = true;
    for (int t0 = 1; t0 <= R && live; t0 += VG_U) {
      LineCursor cur = index_line_cursor(ln, t0);
#pragma unroll
      for (int u = 0; u < VG_U; ++u) {
        if (live && cur.t <= R) {
          int d[2];
          index_line_cursor_offset(ln, cur, d);
          const int a = d[0], b = d[1], i = vi + a, j = vj + b;
          if (i < 0 || j < 0 || i >= rows || j >= cols || a * a + b * b > RR) {
            live = false;   // the walk stops before this cell
          } else {
            const int wa = a + R, w = (b + R) * NW + (wa >> 5);
            const unsigned bit = 1u << (wa & 31);
            atomicOr(&seen[w], bit);
            const unsigned stop = unknown_opaque ? occ[w] | unk[w] : occ[w];
            if (stop & bit) live = false;   // ... and after this one
          }
        }
        index_line_cursor_step(ln, cur);
      }
    }
  }
  __syncthreads();

  // ---- 3. the counts ----
  int visible = 0, gain = 0, surface = 0;
  for (int k = tid; k < words; k += 256) {
    const unsigned s = seen[k];
    visible += __popc(s);
    gain += __popc(s & unk[k]);
    surface += __popc(s & occ[k]);
  }
  visible = wave_sum(visible);
  gain = wave_sum(gain);
  surface = wave_sum(surface);
  if (lane == 0) { vg_part[wave][0] = visible; vg_part[wave][1] = gain; vg_part[wave][2] = surface; }
  __syncthreads();
  if (tid == 0) {
    r.visible = vg_part[0][0] + vg_part[1][0] + vg_part[2][0] + vg_part[3][0];
    r.unknown = vg_part[0][1] + vg_part[1][1] + vg_part[2][1] + vg_part[3][1];
    r.occupied = vg_part[0][2] + vg_part[1][2] + vg_part[2][2] + vg_part[3][2];
    out[q] = r;
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace {

// The ray-to-thread deal: ray k of the list ends at ring position (k * stride) mod 8R.  The spread deal puts the 64 lanes of a
// wavefront about 8R / 64 ring cells apart (the smallest odd stride >= 8R / 64 that shares no factor with 8R): their seen bits
// fall into different words.  Stride 1 lets neighbouring lanes walk neighbouring rays: they contend for the same words, but
// they also end together.  Measured on the explored bench map (profiles/view_gain_rows.json, 4 513 view points, R = 127):
// transparent unknown cells, where most rays run their full length, spread 839 us against 1 047; RNA_VIEW_UNKNOWN_OPAQUE, where
// most rays end after a few cells and a wavefront waits for its longest, adjacent 594 us against 847.  So the flag picks the
// deal; RNA_VIEW_GAIN_DEAL = 0 (adjacent) / 1 (spread) forces one (developer knob, scripts/view_gain_rows.py).
int vg_stride(int R, bool unknown_opaque) {
  static const int forced = [] { const char* v = getenv("RNA_VIEW_GAIN_DEAL"); return v ? (atoi(v) != 0 ? 1 : 0) : -1; }();
  if (forced >= 0 ? forced == 0 : unknown_opaque) return 1;
  const int n = 8 * R;
  for (int s = (n / 64) | 1;; s += 2) {
    int a = n, b = s;
    while (b) { const int t = a % b; a = b; b = t; }
    if (a == 1) return s;   // (s = n + 1 at the latest)
  }
}

int view_gain(rna_engine* e, const int32_t* cells, int n, int radius_cells, unsigned flags, ViewGain* out, bool host) {
  // (argument checks first: none of them reads the engine)
  if (!e || n < 0 || radius_cells < 1 || (flags & ~(unsigned)RNA_VIEW_UNKNOWN_OPAQUE) || (n > 0 && (!cells || !out))) return RNA_EINVAL;
  if (radius_cells > RNA_VIEW_MAX_RADIUS)
    return fail(e, RNA_ECAPACITY, "rna_view_gain: radius_cells exceeds RNA_VIEW_MAX_RADIUS (the window's bitmaps live in LDS)");
  if (n == 0) return RNA_OK;
  RNA_ENTER(e);   // behind the map updates enqueued so far, as rna_layer_download reads the layer
  Staging st(e, "rna_view_gain");
  const int32_t* d_cells = host ? st.in(cells, (size_t)n) : cells;
  ViewGain* d_out = host ? st.out(out, (size_t)n) : out;
  if (st.ok()) {
    const Geom& g = e->geom;
    const bool opaque = (flags & RNA_VIEW_UNKNOWN_OPAQUE) != 0;
    hipLaunchKernelGGL(view_gain_kernel, dim3(n), dim3(256), vg_lds_bytes(radius_cells), e->stream, e->layer[RNA_LAYER_MASTER], d_cells, n,
                       radius_cells, vg_stride(radius_cells, opaque), opaque ? 1 : 0, d_out, g.size[0], g.size[1],
                       g.start[0], g.start[1]);
  }
  return st.finish();
}

}  // namespace

extern "C" int rna_view_gain(rna_engine* e, const int32_t* cells_host, int n, int radius_cells, unsigned flags, ViewGain* out_host) {
  return view_gain(e, cells_host, n, radius_cells, flags, out_host, true);
}

extern "C" int rna_view_gain_device(rna_engine* e, const int32_t* cells_device, int n, int radius_cells, unsigned flags,
                                    ViewGain* out_device) {
  return view_gain(e, cells_device, n, radius_cells, flags, out_device, false);
}
