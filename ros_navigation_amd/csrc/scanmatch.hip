// scanmatch.hip -- scan-to-map matching: correct a sensor pose by correlating the end points of a scan with the occupied cells
// of the master layer, exhaustively over a window of rotations and cell shifts (Olson's correlative matcher, single
// resolution).  The definition (include/rna.h, DESIGN.md section 4 "Scan matching") is in index space, integers only:
//   occupied(c)  cell_blocked(master[c]) -- the RAW layer, no robot radius --, false outside the map
//   bit_l(c)     some occupied cell within Chebyshev distance l of c, l = 0 .. L - 1;  w(c) = sum of the bit_l(c)
//   point        (px, py) in Q6, used iff |px|, |py| <= 32767 and px^2 + py^2 <= (64 R)^2
//   rotation r   (c, s) in Q14: qx = (c px - s py + 8192) >> 14, qy = (s px + c py + 8192) >> 14
//   cell         (gi + ((qx + sub0 + 32) >> 6), gj + ((qy + sub1 + 32) >> 6)) around the guess cell (gi, gj)
//   score        (r, da, db) -> sum over the used points of w(cell + (da, db)), |da|, |db| <= T
//   best         greatest score, then smallest da^2 + db^2, |r - r_c|, r, db, da
// Sums and a total order: every output has exactly one right value whatever the order threads and workgroups arrive in.
#include "engine.hpp"
#include "map_tiles_dev.hpp"

#include <climits>

using namespace rna;

using ScanMatch = struct rna_scan_match;   // (the elaborated name: in C++ the entry point rna_scan_match hides the record's)

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_CHUNK = 2048;   // rotated points staged in LDS per turn (8 KiB)
constexpr int SM_CAND = (2 * RNA_SCAN_MATCH_MAX_SHIFT + 1) * (2 * RNA_SCAN_MATCH_MAX_SHIFT + 1);
constexpr int SM_K = (SM_CAND + SM_THREADS - 1) / SM_THREADS;   // shift candidates a thread owns at most (5)

// The window: half-width H = R + 1 + T + (L - 1) cells round the guess cell -- a rotated point lies within R + 1 cells of it
// (R for a pair (c, s) of magnitude 16384 and sub in [-32, 31]; the kernel drops what lies further), a shift adds T, the
// widest dilation reads L - 1 further.  W = 2 H + 1 <= 295 rows of NW <= 10 words; the L bitmaps are interleaved word by
// word, LS words per bitmap word (3 levels take the stride of 4), so that one aligned LDS read returns every level of a cell.
inline int sm_half(int R, int T, int L) { return R + 1 + T + (L - 1); }
inline int sm_stride(int L) { return L == 3 ? 4 : L; }
inline size_t sm_lds_bytes(int R, int T, int L) {
  const int W = 2 * sm_half(R, T, L) + 1, NW = (W + 31) / 32;
  return ((((size_t)W * NW * sm_stride(L) + 3) & ~(size_t)3) + SM_CHUNK + 16) * sizeof(unsigned);   // bitmaps | staged points | 16 control words
}

// The best as one 64-bit key, greater = better: score (16 bits: <= 8192 points x 4 levels) | 1023 - (da^2 + db^2)
// (<= 512) | 127 - |r - r_c| | 127 - r | 63 - (db + T) | 63 - (da + T).
__device__ __forceinline__ unsigned long long sm_key(int score, int da, int db, int r, int rc, int T) {
  const int dr = r >= rc ? r - rc : rc - r;
  return ((unsigned long long)(unsigned)score << 36) | ((unsigned long long)(unsigned)(1023 - (da * da + db * db)) << 26) |
         ((unsigned long long)(unsigned)(127 - dr) << 19) | ((unsigned long long)(unsigned)(127 - r) << 12) |
         ((unsigned long long)(unsigned)(63 - (db + T)) << 6) | (unsigned long long)(unsigned)(63 - (da + T));
}

// w of the cell at bit `idx` of the interleaved bitmaps
template <int L>
__device__ __forceinline__ int sm_w(const unsigned* __restrict__ bits, int idx) {
  const int word = idx >> 5, b = idx & 31;
  if (L == 1) return (int)((bits[word] >> b) & 1u);
  if (L == 2) {
    const uint2 v = *reinterpret_cast<const uint2*>(bits + 2 * word);
    return (int)(((v.x >> b) & 1u) + ((v.y >> b) & 1u));
  }
  const uint4 v = *reinterpret_cast<const uint4*>(bits + 4 * word);
  int s = (int)(((v.x >> b) & 1u) + ((v.y >> b) & 1u) + ((v.z >> b) & 1u));
  if (L == 4) s += (int)((v.w >> b) & 1u);
  return s;
}

}  // namespace

// One workgroup of 256 threads per (query, rotation); no workgroup waits for another.  Dynamic LDS only (its base stays
// 16-byte aligned for the wide reads): the interleaved bitmaps, SM_CHUNK staged points, 16 control words.
//  1. fill: the window's rows are read as map_tiles_dev.hpp's window_rows_each reads them, one ballot per 64 cells; cells
//     outside the map hold no bit.
//  2. dilate: level l from level l - 1, a word ORed with its two shifts (carrying across words) over its three rows.
//  3. per chunk of SM_CHUNK points: the used ones are rotated once and staged as bit offsets ob * RB + oa (RB = bits of a
//     bitmap row), compacted through a counter in LDS; then every thread adds w over the staged points for the <= SM_K shift
//     candidates it owns (candidate = tid + 256 k, k < nk = ceil((2T + 1)^2 / 256) <= SM_K, da fastest: the lanes of a
//     wavefront read the same or the neighbouring word): nk bitmap reads per staged point and thread.  Scores stay in
//     registers.  A query without a used point leaves before the fill.
//  4. the volume slice, the workgroup's best as one key -> one atomicMax on the query's record; the workgroup of rotation
//     r_c also writes n_used and score_guess.
// Loops are bounded by W, L, n_points <= 8192 and SM_K.
template <int L>
__global__ void __launch_bounds__(SM_THREADS)
scan_match_kernel(const float* __restrict__ master, const rna_scan_match_query* __restrict__ queries, const int32_t* __restrict__ points,
                  size_t n_points_total, const int32_t* __restrict__ rot, int n_rot, int R, int T, ScanMatch* __restrict__ out,
                  int32_t* __restrict__ volume, int rows, int cols, int s0, int s1) {
  extern __shared__ __attribute__((aligned(16))) unsigned sm_lds[];
  constexpr int LS = L == 3 ? 4 : L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x / n_rot, r = blockIdx.x - q * n_rot, rc = n_rot >> 1;
  const int H = R + 1 + T + (L - 1), W = 2 * H + 1, NW = (W + 31) >> 5, words = W * NW, RB = NW * 32;
  const int S = 2 * T + 1, ncand = S * S;
  unsigned* const bits = sm_lds;
  int* const stage = reinterpret_cast<int*>(sm_lds + ((words * LS + 3) & ~3));   // (16-byte aligned: read four points at a time)
  unsigned* const ctl = sm_lds + ((words * LS + 3) & ~3) + SM_CHUNK;
  const rna_scan_match_query qu = queries[q];
  int32_t* const vol = volume ? volume + ((size_t)q * n_rot + r) * (size_t)ncand : nullptr;
  if (!buffer_cell_in_range(qu.cell, rows, cols)) {   // (uniform) status 1: the decode kernel says so
    if (vol)
      for (int c = tid; c < ncand; c += SM_THREADS) vol[c] = 0;
    return;
  }
  int gi, gj;
  map_cell_of((unsigned)qu.cell, rows, cols, s0, s1, gi, gj);
  // a query whose points leave the array has none (status 2)
  const int np = (qu.n_points < 0 || qu.n_points > RNA_SCAN_MATCH_MAX_POINTS || qu.points_offset < 0 ||
                  (size_t)qu.points_offset + (size_t)qu.n_points > n_points_total) ? 0 : qu.n_points;
  const unsigned RR = (unsigned)(64 * R) * (unsigned)(64 * R);
  const int32_t* const pq = points + 2 * (size_t)qu.points_offset;
  // no used point (status 2, the record stays as cleared): zeros, and neither fill nor dilation
  int any = 0;
  for (int p = tid; p < np; p += SM_THREADS) {
    const int px = pq[2 * (size_t)p], py = pq[2 * (size_t)p + 1];
    any |= px >= -32767 && px <= 32767 && py >= -32767 && py <= 32767 && (unsigned)(px * px) + (unsigned)(py * py) <= RR;
  }
  // control words: [0] points staged so far, [1] used points of the query, [2] some point is used, [4..11] the wavefronts' best keys
  if (tid < 16) ctl[tid] = 0u;
  __syncthreads();
  if (any) ctl[2] = 1u;
  __syncthreads();
  if (!ctl[2]) {   // (uniform)
    if (vol)
      for (int c = tid; c < ncand; c += SM_THREADS) vol[c] = 0;
    return;
  }

  // ---- 1. the window's occupied bits: level 0 ----
  window_rows_each<5>(master, gi - H, gj - H, W, W, rows, cols, s0, s1, [&](int wb, int p, bool ok, float v) {   // (W <= 295: 5 pieces)
    const unsigned long long mo = __ballot(ok && cell_blocked(v));
    const int w = wb * NW + 2 * p;
    if (lane == 0) bits[w * LS] = (unsigned)mo;
    if (lane == 1 && 2 * p + 1 < NW) bits[(w + 1) * LS] = (unsigned)(mo >> 32);
  });
  __syncthreads();

  // ---- 2. the dilated levels ----
#pragma unroll
  for (int l = 1; l < L; ++l) {
    for (int w = tid; w < words; w += SM_THREADS) {
      const int row = w / NW, k = w - row * NW;
      unsigned h = 0u;
#pragma unroll
      for (int dr = -1; dr <= 1; ++dr) {
        const int rr = row + dr;
        if (rr < 0 || rr >= W) continue;
        const unsigned* src = bits + (rr * NW + k) * LS + (l - 1);
        const unsigned x = src[0], left = k > 0 ? src[-LS] : 0u, right = k + 1 < NW ? src[LS] : 0u;
        h |= x | (x << 1) | (x >> 1) | (left >> 31) | (right << 31);
      }
      bits[w * LS + l] = h;
    }
    __syncthreads();
  }

  // ---- 3. the points, chunk by chunk ----
  int cb[SM_K], score[SM_K];
#pragma unroll
  for (int k = 0; k < SM_K; ++k) {
    const int c = tid + SM_THREADS * k;
    const int cc = c < ncand ? c : 0;   // (a thread without a k-th candidate scores candidate 0 and drops the sum)
    const int db = cc / S, da = cc - db * S;   // (+ T)
    cb[k] = (db - T + H) * RB + (da - T + H);
    score[k] = 0;
  }
  const int cr = rot[2 * ((size_t)q * n_rot + r)], sr = rot[2 * ((size_t)q * n_rot + r) + 1];
  const int nk = (ncand + SM_THREADS - 1) / SM_THREADS;   // candidate slots in use, 1 .. SM_K: the same for every thread
  int staged = 0;   // points staged by the chunks before this one (ctl[0] counts on)
  for (int p0 = 0; p0 < np; p0 += SM_CHUNK) {
    const int pend = min(np, p0 + SM_CHUNK);
    for (int b = p0 + 64 * wave; b < pend; b += SM_THREADS) {   // (b is uniform: whole wavefronts enter, the ballots need every lane)
      const int p = b + lane;
      const bool have = p < pend;
      const int px = have ? pq[2 * (size_t)p] : 0, py = have ? pq[2 * (size_t)p + 1] : 0;
      const bool used = have && px >= -32767 && px <= 32767 && py >= -32767 && py <= 32767 &&
                        (unsigned)(px * px) + (unsigned)(py * py) <= RR;
      // (unsigned arithmetic: a pair (c, s) beyond 16384 wraps instead of overflowing; the window test below drops such a point)
      const int qx = (int)((unsigned)cr * (unsigned)px - (unsigned)sr * (unsigned)py + 8192u) >> 14;
      const int qy = (int)((unsigned)sr * (unsigned)px + (unsigned)cr * (unsigned)py + 8192u) >> 14;
      const int oa = (int)((unsigned)qx + (unsigned)qu.sub[0] + 32u) >> 6, ob = (int)((unsigned)qy + (unsigned)qu.sub[1] + 32u) >> 6;
      const bool in = used && oa >= -(R + 1) && oa <= R + 1 && ob >= -(R + 1) && ob <= R + 1;
      const unsigned long long mu = __ballot(used), mi = __ballot(in);
      int base = 0;
      if (lane == 0) {
        if (mi) base = (int)atomicAdd(&ctl[0], (unsigned)__popcll(mi)) - staged;
        if (mu) atomicAdd(&ctl[1], (unsigned)__popcll(mu));
      }
      base = __shfl(base, 0, 64);
      if (in) stage[base + __popcll(mi & ((1ull << lane) - 1ull))] = ob * RB + oa;
    }
    __syncthreads();
    const int cnt = (int)ctl[0] - staged;
    staged += cnt;
    int p = 0;
    for (; p + 4 <= cnt; p += 4) {
      const int4 pb = *reinterpret_cast<const int4*>(stage + p);
#pragma unroll
      for (int k = 0; k < SM_K; ++k) {
        if (k >= nk) break;   // (uniform: a small window pays for the slots it has)
        score[k] += sm_w<L>(bits, pb.x + cb[k]) + sm_w<L>(bits, pb.y + cb[k]) + sm_w<L>(bits, pb.z + cb[k]) + sm_w<L>(bits, pb.w + cb[k]);
      }
    }
    for (; p < cnt; ++p) {
      const int pb = stage[p];
#pragma unroll
      for (int k = 0; k < SM_K; ++k) {
        if (k >= nk) break;   // (uniform)
        score[k] += sm_w<L>(bits, pb + cb[k]);
      }
    }
    __syncthreads();   // the staged points have been read: the next chunk may overwrite them
  }

  // ---- 4. the volume slice, the best, the guess ----
  unsigned long long best = 0ull;
  const int c0 = T * S + T;   // the candidate (0, 0)
#pragma unroll
  for (int k = 0; k < SM_K; ++k) {
    const int c = tid + SM_THREADS * k;
    if (c < ncand) {
      if (vol) vol[c] = score[k];
      const int db = c / S, da = c - db * S;
      const unsigned long long key = sm_key(score[k], da - T, db - T, r, rc, T);
      best = key > best ? key : best;
      if (c == c0 && r == rc) {
        out[q].n_used = (int32_t)ctl[1];
        out[q].score_guess = score[k];
      }
    }
  }
  best = wave_max(best);
  unsigned long long* const wbest = reinterpret_cast<unsigned long long*>(ctl + 4);
  if (lane == 0) wbest[wave] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < 4; ++k) best = wbest[k] > best ? wbest[k] : best;
    atomicMax(reinterpret_cast<unsigned long long*>(&out[q]), best);   // (the record's first 8 bytes hold the key until the decode)
  }
}

// one thread per query: the key in the record's first 8 bytes -> the record
__global__ void __launch_bounds__(SM_THREADS)
scan_match_decode_kernel(const rna_scan_match_query* __restrict__ queries, int n, int n_rot, int T, int L, ScanMatch* __restrict__ out,
                         int rows, int cols) {
  const int q = blockIdx.x * SM_THREADS + threadIdx.x;
  if (q >= n) return;
  const unsigned long long key = *reinterpret_cast<const unsigned long long*>(&out[q]);
  ScanMatch m = {0, 0, n_rot >> 1, {0, 0}, 0, 0, 0};
  if (!buffer_cell_in_range(queries[q].cell, rows, cols)) m.status = 1;
  else if (out[q].n_used == 0) m.status = 2;
  else {
    m.score = (int32_t)(key >> 36);
    m.rot = 127 - (int)((key >> 12) & 127u);
    m.shift[0] = 63 - (int)(key & 63u) - T;
    m.shift[1] = 63 - (int)((key >> 6) & 63u) - T;
    m.n_used = out[q].n_used;
    m.score_guess = out[q].score_guess;
    m.score_max = m.n_used * L;
  }
  out[q] = m;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace {

int scan_match(rna_engine* e, const rna_scan_match_query* queries, int n, const int32_t* points, size_t n_points_total, const int32_t* rot,
               int n_rot, int range_cells, int max_shift, int levels, ScanMatch* out, int32_t* volume, bool host) {
  // (argument checks first: none of them reads the engine)
  if (!e || n < 0 || n_rot < 1 || range_cells < 1 || levels < 1 || max_shift < 0 ||
      (n > 0 && (!queries || !rot || !out || (!points && n_points_total > 0))))
    return RNA_EINVAL;
  if (!host && ((uintptr_t)out & 7u)) return RNA_EINVAL;   // (the records hold the 64-bit keys while the kernels run)
  if (range_cells > RNA_SCAN_MATCH_MAX_RANGE || max_shift > RNA_SCAN_MATCH_MAX_SHIFT || levels > RNA_SCAN_MATCH_MAX_LEVELS ||
      n_rot > RNA_SCAN_MATCH_MAX_ROT)
    return fail(e, RNA_ECAPACITY,
                "rna_scan_match: range_cells, max_shift, levels or n_rot exceeds RNA_SCAN_MATCH_MAX_RANGE / _SHIFT / _LEVELS / _ROT "
                "(the window's bitmaps live in LDS, the best is one 64-bit key)");
  // (a launch holds fewer than 2^32 threads: 2^24 workgroups of 256)
  if ((long long)n * n_rot >= (1ll << 24)) return fail(e, RNA_ECAPACITY, "rna_scan_match: n * n_rot reaches 2^24 workgroups, more than one launch holds");
  if (host)
    for (int q = 0; q < n; ++q)
      if (queries[q].n_points < 0 || queries[q].n_points > RNA_SCAN_MATCH_MAX_POINTS || queries[q].points_offset < 0 ||
          (size_t)queries[q].points_offset + (size_t)queries[q].n_points > n_points_total)
        return RNA_EINVAL;
  if (n == 0) return RNA_OK;
  RNA_ENTER(e);   // behind the map updates enqueued so far, as rna_layer_download reads the layer
  Staging st(e, "rna_scan_match");
  const int S = 2 * max_shift + 1;
  const rna_scan_match_query* d_q = host ? st.in(queries, (size_t)n) : queries;
  const int32_t* d_pts = host ? st.in(points, 2 * n_points_total) : points;
  const int32_t* d_rot = host ? st.in(rot, 2 * (size_t)n * n_rot) : rot;
  ScanMatch* d_out = host ? st.out(out, (size_t)n) : out;
  int32_t* d_vol = host && volume ? st.out(volume, (size_t)n * n_rot * S * S) : volume;
  if (st.ok()) {
    const Geom& g = e->geom;
    // three enqueues: the keys start at 0 (below every key a workgroup offers), the scores, the decode
    if (hipMemsetAsync(d_out, 0, (size_t)n * sizeof(ScanMatch), e->stream) != hipSuccess)
      return fail(e, RNA_EHIP, "rna_scan_match: hipMemsetAsync failed");
    const dim3 grid((unsigned)(n * n_rot)), block(SM_THREADS);
    const size_t lds = sm_lds_bytes(range_cells, max_shift, levels);
#define RNA_SM_LAUNCH(LV)                                                                                                              \
  hipLaunchKernelGGL(scan_match_kernel<LV>, grid, block, lds, e->stream, e->layer[RNA_LAYER_MASTER], d_q, d_pts, n_points_total, d_rot, \
                     n_rot, range_cells, max_shift, d_out, d_vol, g.size[0], g.size[1], g.start[0], g.start[1])
    switch (levels) {
      case 1: RNA_SM_LAUNCH(1); break;
      case 2: RNA_SM_LAUNCH(2); break;
      case 3: RNA_SM_LAUNCH(3); break;
      default: RNA_SM_LAUNCH(4); break;
    }
#undef RNA_SM_LAUNCH
    hipLaunchKernelGGL(scan_match_decode_kernel, dim3((n + SM_THREADS - 1) / SM_THREADS), block, 0, e->stream, d_q, n, n_rot, max_shift,
                       levels, d_out, g.size[0], g.size[1]);
  }
  return st.finish();
}

}  // namespace

extern "C" int rna_scan_match(rna_engine* e, const rna_scan_match_query* queries_host, int n, const int32_t* points_host,
                              size_t n_points_total, const int32_t* rot_host, int n_rot, int range_cells, int max_shift, int levels,
                              ScanMatch* out_host, int32_t* volume_host) {
  return scan_match(e, queries_host, n, points_host, n_points_total, rot_host, n_rot, range_cells, max_shift, levels, out_host,
                    volume_host, true);
}

extern "C" int rna_scan_match_device(rna_engine* e, const rna_scan_match_query* queries_device, int n, const int32_t* points_device,
                                     size_t n_points_total, const int32_t* rot_device, int n_rot, int range_cells, int max_shift,
                                     int levels, ScanMatch* out_device, int32_t* volume_device) {
  return scan_match(e, queries_device, n, points_device, n_points_total, rot_device, n_rot, range_cells, max_shift, levels, out_device,
                    volume_device, false);
}
