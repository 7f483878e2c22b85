// shortcut.hip -- line-of-sight shortcutting of cell paths: the staircase a grid planner answers with is reduced to the way
// points where it has to turn, every straight leg between two of them checked against the search's neighbour masks.
// The definition (include/rna.h) is sequential:
//   emit p[0]; a = 0; while a < L - 1: k = a + 1; while k + 1 < L and span allows and ok(a, k + 1): k += 1; emit p[k]; a = k
// with ok(a, m) = every step of line(p[a], p[m]) -- the reference's LineIterator(map, Index, Index), gridmath.hpp's closed
// form -- is a move the masks allow, and with RNA_SHORTCUT_KEEP_CLEARANCE no cell of the line has a smaller clearance than
// the smallest of p[a .. m].
//
// Cost.  An anchor on an open map sees the whole rest of its path: about L^2 / 2 mask bytes per path without max_span and
// L * max_span with it.  That is why max_span exists.
#include "engine.hpp"
#include "map_tiles_dev.hpp"

using namespace rna;

namespace {

constexpr int SC_U = 8;   // line cells a lane has in flight per turn (independent loads: no address depends on a loaded value)

}  // namespace

// One wavefront per path; no workgroup waits for another, no atomics.
//  1. the row is staged once: lane t reads cell t, t + 64, ...; a cell outside [0, ncell) makes the path invalid, every other
//     one goes to LDS as its map-space (i, j), 16 bits each (rows, cols <= 65536, checked by the host).
//  2. consecutive cells must be king moves in map space (else invalid: from here on every line lies in the bounding box of two
//     validated cells, so every gather of nbr / clr is inside the map); the steps the masks do not allow are counted.
//  3. per anchor a the candidates m = k + 1, k + 2, ... are evaluated 64 at a time, one per lane: the lane walks
//     line(p[a], p[m]), SC_U cells per turn (the closed form places the turn's first cell -- one division --, the reference's
//     numerator increments the others).  The sequential rule stops at the FIRST candidate that fails, and whether a
//     candidate fails depends on a and m alone -- not on the candidates before it -- so the lowest failing lane of the ballot
//     is that candidate: every lane below it passed, k advances by its number, the lanes above it (evaluated for nothing) are
//     dropped, as soon as a lower lane is known to have failed.  Candidates beyond the path's end or the span count as failed,
//     which ends the anchor exactly where the rule's two bounds end it, also in the middle of a chunk.
//     KEEP_CLEARANCE: min clr of p[a .. m] is a prefix minimum over the lanes' own path cells (a wave scan) joined with the
//     minimum carried from the chunks before; the line's end points belong to that piece, so only "some line cell is below it"
//     has to be tested.
template <bool CLR>
__global__ void __launch_bounds__(64) shortcut_kernel(const int32_t* __restrict__ paths, const rna_astar_result* __restrict__ results, int n,
                                                      int max_len, int max_span, const uint8_t* __restrict__ nbr,
                                                      const uint16_t* __restrict__ clr, int32_t* __restrict__ waypoints, int max_wp,
                                                      rna_shortcut_result* __restrict__ out, int rows, int cols, int s0, int s1) {
  extern __shared__ unsigned P[];   // [max_len] (j << 16) | i
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q >= n) return;
  const rna_astar_result in = results[q];
  rna_shortcut_result r = {1, 0, 0, 0};
  if (in.status != 0 || in.path_len < 1 || in.path_len > max_len) {   // (uniform)
    if (lane == 0) out[q] = r;
    return;
  }
  const int L = in.path_len;
  const int32_t* row = paths + (size_t)q * max_len;
  bool bad = false;
  for (int t = lane; t < L; t += 64) {
    int32_t c = row[t];
    if (!buffer_cell_in_range(c, rows, cols)) { bad = true; c = 0; }
    int i, j;
    map_cell_of((unsigned)c, rows, cols, s0, s1, i, j);
    P[t] = ((unsigned)j << 16) | (unsigned)i;
  }
  __syncthreads();
  int blocked = 0;
  if (!__any(bad)) {
    for (int t = lane; t + 1 < L; t += 64) {
      const unsigned a = P[t], b = P[t + 1];
      const int ai = (int)(a & 0xFFFFu), aj = (int)(a >> 16);
      const int di = (int)(b & 0xFFFFu) - ai, dj = (int)(b >> 16) - aj;
      if (di < -1 || di > 1 || dj < -1 || dj > 1 || (di == 0 && dj == 0)) bad = true;
      else if (!(nbr[buffer_lin<unsigned>(ai, aj, rows, cols, s0, s1)] & nbr_move_bit(di, dj))) ++blocked;
    }
  }
  if (__any(bad)) {
    r.status = 2;
    if (lane == 0) out[q] = r;
    return;
  }
  r.blocked_steps = wave_sum(blocked);

  int32_t* wp = waypoints + (size_t)q * max_wp;
  int nw = 1, longest = 0;
  if (lane == 0) wp[0] = row[0];   // (max_wp >= 2)
  int a = 0;
  while (a < L - 1) {
    const int lim = max_span && max_span < L - 1 - a ? a + max_span : L - 1;   // the last candidate the rule's bounds allow
    const unsigned pa = P[a];
    const int ai = (int)(pa & 0xFFFFu), aj = (int)(pa >> 16);
    int k = a + 1;
    int carry = 0;   // KEEP_CLEARANCE: min clr over p[a .. k]
    if (CLR && k < lim) {
      const unsigned p1 = P[k];
      carry = min((int)clr[buffer_lin<unsigned>(ai, aj, rows, cols, s0, s1)],
                  (int)clr[buffer_lin<unsigned>((int)(p1 & 0xFFFFu), (int)(p1 >> 16), rows, cols, s0, s1)]);
    }
    while (k < lim) {
      const int m = k + 1 + lane;
      const bool valid = m <= lim;
      const unsigned pm = P[valid ? m : lim];
      const int mi = (int)(pm & 0xFFFFu), mj = (int)(pm >> 16);
      int floor_clr = 0;   // min clr over p[a .. m]
      if (CLR) {
        int v = valid ? (int)clr[buffer_lin<unsigned>(mi, mj, rows, cols, s0, s1)] : RNA_CLEARANCE_NONE;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int o = __shfl_up(v, d, 64);
          if (lane >= d) v = min(v, o);
        }
        floor_clr = min(carry, v);
      }
      const int e0[2] = {ai, aj}, e1[2] = {mi, mj};
      const IndexLine ln = index_line(e0, e1);
      const unsigned straight = ln.major == 0 ? nbr_move_bit(ln.step[0], 0) : nbr_move_bit(0, ln.step[1]);
      const unsigned diagonal = nbr_move_bit(ln.step[0], ln.step[1]);
      const int D = valid ? ln.D : 0;
      bool failed = !valid;
      int t = 0;
      for (;;) {
        const unsigned long long fm = __ballot(failed);
        const bool beaten = fm && lane > __ffsll((long long)fm) - 1;   // a candidate before this one has failed already
        const bool act = !failed && !beaten && t < D;
        if (!__any(act)) break;
        if (act) {
          uint8_t mask[SC_U];
          uint16_t cl[SC_U];
          unsigned bit[SC_U];
          // one division per turn places the cursor at cell t, then the reference's own increments
          LineCursor cur = index_line_cursor(ln, t);   // (act: valid, 1 <= D <= 65535)
#pragma unroll
          for (int u = 0; u < SC_U; ++u) {
            const bool live = cur.t < D;   // the cell has a step to test (cells past the line's last step read cell 0 and pass)
            int d[2];
            index_line_cursor_offset(ln, cur, d);
            const unsigned c = live ? buffer_lin<unsigned>(ai + d[0], aj + d[1], rows, cols, s0, s1) : 0u;
            const uint8_t mk = nbr[c];
            mask[u] = live ? mk : (uint8_t)0xFF;
            if (CLR) {
              const uint16_t cv = clr[c];
              cl[u] = live ? cv : (uint16_t)RNA_CLEARANCE_NONE;
            }
            bit[u] = index_line_cursor_step(ln, cur) ? diagonal : straight;
          }
#pragma unroll
          for (int u = 0; u < SC_U; ++u) {
            if (!(mask[u] & bit[u])) failed = true;
            if (CLR && (int)cl[u] < floor_clr) failed = true;
          }
          t += SC_U;
        }
      }
      const unsigned long long fm = __ballot(failed);
      const int f = fm ? __ffsll((long long)fm) - 1 : 64;
      k += f;
      if (f < 64) break;
      if (CLR) carry = __shfl(floor_clr, 63, 64);
    }
    if (lane == 0 && nw < max_wp) wp[nw] = row[k];
    ++nw;
    longest = max(longest, k - a);
    a = k;
  }
  r.status = nw > max_wp ? 3 : 0;
  r.n_waypoints = nw;
  r.longest_span = longest;
  if (lane == 0) out[q] = r;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace {

int shortcut_paths(rna_engine* e, const int32_t* paths, const rna_astar_result* results, int n, int max_path_len, int max_span,
                   unsigned flags, int32_t* waypoints, int max_waypoints, rna_shortcut_result* out, bool host) {
  // (argument checks first: none of them reads the engine)
  if (!e || n < 0 || max_path_len < 1 || max_waypoints < 2 || max_span < 0 || max_span == 1 ||
      (flags & ~(unsigned)RNA_SHORTCUT_KEEP_CLEARANCE) || (n > 0 && (!paths || !results || !waypoints || !out)))
    return RNA_EINVAL;
  const bool keep = (flags & RNA_SHORTCUT_KEEP_CLEARANCE) != 0;
  if (max_path_len > RNA_SHORTCUT_MAX_PATH_LEN)
    return fail(e, RNA_ECAPACITY, "rna_shortcut_paths: max_path_len exceeds RNA_SHORTCUT_MAX_PATH_LEN (a path is staged in LDS)");
  if (e->geom.size[0] > 65536 || e->geom.size[1] > 65536)
    return fail(e, RNA_ECAPACITY, "rna_shortcut_paths: more than 65 536 cells along an axis");
  if (keep && (e->clearance.R == 0 || e->clearance.epoch != e->map.epoch))
    return fail(e, RNA_ESTATE, "rna_shortcut_paths: RNA_SHORTCUT_KEEP_CLEARANCE needs a current clearance field (rna_clearance_build)");
  if (n == 0) return RNA_OK;
  RNA_ENTER(e);
  int rc = map_prepare_nbr(e);
  if (rc != RNA_OK) return rc;
  // LDS of a workgroup = 4 B x max_path_len, the caller's row stride (not the longest path of the batch): it decides how many
  // paths a compute unit works on at a time -- 160 KiB / (4 x max_path_len), e.g. 2 at 16 384 cells, 1 at 40 960
  const size_t lds = (size_t)max_path_len * sizeof(unsigned);
  if (lds > 64 * 1024 && !e->shortcut_lds_raised) {   // beyond the default limit of a launch: one workgroup may take the compute unit's 160 KiB
    RNA_HIP(e, hipFuncSetAttribute(reinterpret_cast<const void*>(&shortcut_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   RNA_SHORTCUT_MAX_PATH_LEN * (int)sizeof(unsigned)));
    RNA_HIP(e, hipFuncSetAttribute(reinterpret_cast<const void*>(&shortcut_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   RNA_SHORTCUT_MAX_PATH_LEN * (int)sizeof(unsigned)));
    e->shortcut_lds_raised = true;
  }
  if (!host) {
    // device pointers may be the outputs of rna_astar_batch_device batches still in flight on the pipeline stages' own
    // streams: the engine stream waits for every busy stage's search (a wait on an event that is complete costs nothing).
    // Skipping a stage that is not busy is no race: `busy` is host state, set when `done` is recorded behind a search and
    // cleared only after the host has seen that event complete (an event query or a synchronisation, then stage_settled in
    // astar.hip), so a stage that is not busy has nothing in flight.
    const AstarDevice& a = e->astar;
    if (a.depth > 1)
      for (int d = 0; d < a.depth && d < AstarDevice::MAX_DEPTH; ++d)
        if (a.stage[d].busy && a.stage[d].done) RNA_HIP(e, hipStreamWaitEvent(e->stream, a.stage[d].done, 0));
  }
  Staging st(e, "rna_shortcut_paths");
  const int32_t* d_paths = host ? st.in(paths, (size_t)n * max_path_len) : paths;
  const rna_astar_result* d_res = host ? st.in(results, (size_t)n) : results;
  // (slots behind the last way point come back as 0; the _device form leaves them as the caller's buffer had them)
  int32_t* d_wp = host ? st.out(waypoints, (size_t)n * max_waypoints, true) : waypoints;
  rna_shortcut_result* d_out = host ? st.out(out, (size_t)n) : out;
  if (st.ok()) {
    const Geom& g = e->geom;
    hipLaunchKernelGGL(keep ? shortcut_kernel<true> : shortcut_kernel<false>, dim3(n), dim3(64), lds, e->stream, d_paths, d_res, n,
                       max_path_len, max_span, e->nbr, keep ? e->clearance.clr : (const uint16_t*)nullptr, d_wp, max_waypoints, d_out,
                       g.size[0], g.size[1], g.start[0], g.start[1]);
  }
  return st.finish();
}

}  // namespace

extern "C" int rna_shortcut_paths(rna_engine* e, const int32_t* paths_host, const rna_astar_result* results_host, int n, int max_path_len,
                                  int max_span, unsigned flags, int32_t* waypoints_host, int max_waypoints, rna_shortcut_result* out_host) {
  return shortcut_paths(e, paths_host, results_host, n, max_path_len, max_span, flags, waypoints_host, max_waypoints, out_host, true);
}

extern "C" int rna_shortcut_paths_device(rna_engine* e, const int32_t* paths_device, const rna_astar_result* results_device, int n,
                                         int max_path_len, int max_span, unsigned flags, int32_t* waypoints_device, int max_waypoints,
                                         rna_shortcut_result* out_device) {
  return shortcut_paths(e, paths_device, results_device, n, max_path_len, max_span, flags, waypoints_device, max_waypoints, out_device,
                        false);
}

extern "C" int rna_line_cells_index(const int32_t start[2], const int32_t end[2], int32_t* cells, int cap) {
  if (!start || !end || cap < 0 || (cap > 0 && !cells)) return RNA_EINVAL;
  const int lim = 1 << 30;
  for (int k = 0; k < 2; ++k)
    if (start[k] <= -lim || start[k] >= lim || end[k] <= -lim || end[k] >= lim) return RNA_EINVAL;
  const int a[2] = {start[0], start[1]}, b[2] = {end[0], end[1]};
  const IndexLine ln = index_line(a, b);   // (both ends inside +-2^30: the differences fit an int)
  for (int t = 0; t <= ln.D && t < cap; ++t) {
    int c[2];
    index_line_cell(ln, t, c);
    cells[2 * t] = c[0];
    cells[2 * t + 1] = c[1];
  }
  return ln.D + 1;
}
