// vfh_tables.hpp -- the host side of VFH+ that needs no GPU: VFH::VFH + VFH::Init tables (vfh.cpp:53-110,144-166,237-416), the
// arithmetic they share with vfh_step_kernel, and the layout of the two device blocks.  Plain C++ outside hipcc: the tables are
// compared with the oracle's on the CPU (tests/cpp/vfh_tables_dump.cpp, tests/test_vfh_tables_host.py).
#pragma once

#include <vector>

#include "../../include/rna.h"
#include "gridmath.hpp"

namespace rna {

constexpr int MAX_W = 64;
constexpr int MAX_H = 128;

// ---- small pieces of vfh.cpp that are pure arithmetic (usable on host and device) --------------
RNA_HD int k_max_turnrate(int mt0, int mt1, int speed) {  // vfh.cpp:130-138
  int val = (mt0 - (int)(speed * (mt0 - mt1) / 1000.0));
  return val < 0 ? 0 : val;
}
RNA_HD int k_safety_dist(float sd0, float sd1, int speed) {  // vfh.cpp:194-205
  int val = (int)(sd0 + (int)(speed * (sd1 - sd0) / 1000.0));
  return val < 0 ? 0 : val;
}
RNA_HD float k_delta_angle(float a1, float a2) {  // vfh.cpp:673-686
  const float diff = a2 - a1;
  // (both corrections are computed and one value is picked: as an if / else-if the device compiler keeps two nested
  // branches with their exec-mask bookkeeping at every one of the kernel's twenty call sites)
  const float down = diff - 360, up = diff + 360;
  return diff > 180 ? down : (diff < -180 ? up : diff);
}
// glibc 2.35 hypotf() is (float)sqrt((double)x*x + (double)y*y); restated so host tables and the
// device agree bit for bit (the blocked circles against libm's hypotf in tests/test_vfh_tables_host.py)
RNA_HD float k_hypotf(float x, float y) { return (float)sqrt((double)x * (double)x + (double)y * (double)y); }

// q = y W + x numbers the cells of rows 0..YH (y outer, x inner); the first NQF of them are the front cells
struct VfhDims { int W, H, T, CX, CY, YH, NQ, NQF, NW, max_speed; };

// The two device blocks of an instance set: where every sub-array starts (a multiple of 256 bytes) and how long it is.
struct VfhSpan { size_t off, bytes; };
template <typename T, typename B>
void place(T*& field, B* block, const VfhSpan& s) { field = reinterpret_cast<T*>(block + s.off); }   // `field` = its sub-array of `block`
struct VfhLayout {
  // table block, built by build_tables and uploaded whole
  VfhSpan cell_dist, cell_base_mag, cell_dir;   // float [NQ]
  VfhSpan range_idx;                            // int [NQ] rint(2 * dir)
  VfhSpan memb;                                 // unsigned [T][H][NW] sector-major membership bit masks over q, and 16 spare words
  VfhSpan in_circle;                            // unsigned [max_speed + 1][2][NW] cell inside the right / left blocked circle
  VfhSpan min_turning_radius, bcr;              // int, float [max_speed + 1]: Min_Turning_Radius, the blocked circle's radius
  // state block, written by vfh_reset_kernel
  VfhSpan last_binary, hist, origin;            // float [n_robots][H]
  VfhSpan picked, last_picked, blocked_radius;  // float [n_robots]
  VfhSpan last_chosen_speed, max_speed_picked;  // int [n_robots]
  size_t table_bytes, state_bytes;
  VfhLayout(const VfhDims& d, size_t n_robots) {
    size_t at = 0;
    auto take = [&at](size_t words) { const VfhSpan s{at, words * 4}; at = (at + s.bytes + 255) & ~(size_t)255; return s; };
    const size_t cells = (size_t)d.NQ, speeds = (size_t)d.max_speed + 1, nh = n_robots * d.H;
    cell_dist = take(cells); cell_base_mag = take(cells); cell_dir = take(cells); range_idx = take(cells);
    memb = take((size_t)d.T * d.H * d.NW + 16);   // (+16: the kernel reads sixteen words from a row's start whatever NW is)
    in_circle = take(speeds * 2 * d.NW); min_turning_radius = take(speeds); bcr = take(speeds);
    table_bytes = at; at = 0;
    last_binary = take(nh); hist = take(nh); origin = take(nh);
    picked = take(n_robots); last_picked = take(n_robots); blocked_radius = take(n_robots);
    last_chosen_speed = take(n_robots); max_speed_picked = take(n_robots);
    state_bytes = at;
  }
};

struct HostTables : VfhDims {
  std::vector<unsigned char> block;   // VfhLayout's table block on the host, and its sub-arrays
  float *cell_dist, *cell_base_mag, *cell_dir, *bcr;
  int *range_idx, *mtr;
  unsigned *memb, *in_circle;
};

inline float sector_to_dir(float sector, float dir) {  // the four wrap-aware differences of vfh.cpp:343-381
  if ((sector - dir) > 180) return dir - (sector - 360);
  if ((dir - sector) > 180) return sector - (dir + 360);
  return dir - sector;
}

inline bool build_tables(const rna_vfh_params& p, HostTables& t) {
  const float CELL_WIDTH = (float)p.cell_size;
  const float SD0 = (float)p.safety_dist_0ms, SD1 = (float)p.safety_dist_1ms;
  const float ROBOT_RADIUS = (float)p.robot_radius;
  const int W = p.window_diameter, SA = p.sector_angle, MAX_SPEED = p.max_speed;
  if (W < 2 || W > MAX_W || SA < 1 || MAX_SPEED < 1 || MAX_SPEED > 100000) return false;
  t.W = W;
  t.T = (SD0 == SD1) ? 1 : 20;  // vfh.cpp:100-109
  t.CX = t.CY = (int)floor(W / 2.0);
  t.H = (int)rint(360.0 / SA);
  if (t.H < 1 || t.H > MAX_H || t.H != 360 / SA) return false;   // (H 0: a sector angle of 720 and more rounds to no sector at all)
  // Two sectors that do not close the circle (sector angles 144..179): the second one, at SA degrees, can open, a valley can
  // end in it, and the reference then closes that valley at -SA + 360 where the kernel's `last * SA` says SA (Select_Direction).
  if (t.H == 2 && SA != 180) return false;
  t.YH = (int)ceil(W / 2.0);
  t.NQ = (t.YH + 1) * W;
  t.NQF = t.YH * W;
  t.NW = (t.NQ + 31) / 32;
  t.max_speed = MAX_SPEED;
  if (t.YH + 1 > W) return false;
  const int H = t.H, T = t.T, CX = t.CX, CY = t.CY;

  const VfhLayout L(t, 0);
  t.block.assign(L.table_bytes, 0);   // (every table starts as zeros)
  unsigned char* const b = t.block.data();
  place(t.cell_dist, b, L.cell_dist); place(t.cell_base_mag, b, L.cell_base_mag); place(t.cell_dir, b, L.cell_dir); place(t.bcr, b, L.bcr);
  place(t.range_idx, b, L.range_idx); place(t.mtr, b, L.min_turning_radius); place(t.memb, b, L.memb); place(t.in_circle, b, L.in_circle);

  // Min_Turning_Radius (SetCurrentMaxSpeed, vfh.cpp:144-166) and per-speed blocked circles
  for (int x = 0; x <= MAX_SPEED; x++) {
    const double dx = (double)x / 1e6;
    const double dtheta = ((M_PI / 180) * (double)(k_max_turnrate(p.max_turnrate_0ms, p.max_turnrate_1ms, x))) / 1000.0;
    t.mtr[x] = (int)(((dx / tan(dtheta)) * 1000.0) * p.min_turn_radius_safety_factor);
    t.bcr[x] = t.mtr[x] + ROBOT_RADIUS + k_safety_dist(SD0, SD1, x);  // vfh.cpp:1148
  }

  for (int x = 0; x < W; x++) {
    for (int y = 0; y <= t.YH; y++) {
      const int q = y * W + x;
      const float dist = (float)(sqrt(pow((double)(CX - x), 2.0) + pow((double)(CY - y), 2.0)) * CELL_WIDTH);
      const float base = (float)(15 * pow((3000.0 - dist), 4.0) / 100000000.0);
      float d = 0.0f;
      if (x < CX) {
        if (y < CY) { d = atanf((float)(CY - y) / (float)(CX - x)); d = (float)(d * (360.0 / 6.28)); d = (float)(180.0 - d); }
        else if (y == CY) d = 180.0f;
        else { d = atanf((float)(y - CY) / (float)(CX - x)); d = (float)(d * (360.0 / 6.28)); d = (float)(180.0 + d); }
      } else if (x == CX) {
        d = (y < CY) ? 90.0f : (y == CY ? -1.0f : 270.0f);
      } else {
        if (y < CY) { d = atanf((float)(CY - y) / (float)(x - CX)); d = (float)(d * (360.0 / 6.28)); }
        else if (y == CY) d = 0.0f;
        else { d = atanf((float)(y - CY) / (float)(x - CX)); d = (float)(d * (360.0 / 6.28)); d = (float)(360.0 - d); }
      }
      t.cell_dist[q] = dist;
      t.cell_base_mag[q] = base;
      t.cell_dir[q] = d;
      if (y < t.YH && d < 0) {
        // The centre cell of an odd window (direction -1) is a front cell: the reference reads laser_ranges[-2] for it, memory
        // in front of the caller's scan.  Defined here as in oracle/vfh.c: the robot's own cell is never occupied -- a base
        // magnitude of zero leaves its magnitude zero whatever bin it reads.
        t.cell_base_mag[q] = 0.f;
        t.range_idx[q] = 0;
      } else if (y < t.YH) {
        const int ri = (int)rint(d * 2.0);  // vfh.cpp:1018
        if (ri < 0 || ri > 360) return false;  // cannot happen for front cells (y < CY, or y == CY beside the centre of an odd window)
        t.range_idx[q] = ri;
      }
      for (int tb = 0; tb < T; tb++) {
        const int max_speed_this_table = (int)(((float)(tb + 1) / (float)T) * (float)MAX_SPEED);
        float enlarge;
        if (dist > 0) {
          const float r = ROBOT_RADIUS + k_safety_dist(SD0, SD1, max_speed_this_table);
          enlarge = (float)((float)asinf(r / dist) * (180 / M_PI));
        } else {
          enlarge = 0;
        }
        const float plus_dir = d + enlarge, neg_dir = d - enlarge;
        for (int i = 0; i < (360 / SA); i++) {
          const float plus_sector = (i + 1) * (float)SA, neg_sector = i * (float)SA;
          const float nn = sector_to_dir(neg_sector, neg_dir), pn = sector_to_dir(plus_sector, neg_dir);
          const float pp = sector_to_dir(plus_sector, plus_dir), np = sector_to_dir(neg_sector, plus_dir);
          bool plus_dir_bw = false, neg_dir_bw = false, around = false;
          if ((nn >= 0) && (pn <= 0)) neg_dir_bw = true;
          if ((np >= 0) && (pp <= 0)) plus_dir_bw = true;
          if ((nn <= 0) && (np >= 0)) around = true;
          if ((pn <= 0) && (pp >= 0)) plus_dir_bw = true;
          if (plus_dir_bw || neg_dir_bw || around) t.memb[((size_t)tb * H + i) * t.NW + (q >> 5)] |= 1u << (q & 31);
        }
      }
      if (y < t.YH) {  // blocked-circle membership per speed (vfh.cpp:1140-1189)
        for (int s = 0; s <= MAX_SPEED; s++) {
          const float cxr = CX + (t.mtr[s] / (float)CELL_WIDTH);
          const float cxl = CX - (t.mtr[s] / (float)CELL_WIDTH);
          const float cy = (float)CY;
          const float dr = k_hypotf(cxr - x, cy - y) * CELL_WIDTH;
          const float dl = k_hypotf(cxl - x, cy - y) * CELL_WIDTH;
          if (dr < t.bcr[s]) t.in_circle[((size_t)s * 2 + 0) * t.NW + (q >> 5)] |= 1u << (q & 31);
          if (dl < t.bcr[s]) t.in_circle[((size_t)s * 2 + 1) * t.NW + (q >> 5)] |= 1u << (q & 31);
        }
      }
    }
  }
  return true;
}

}  // namespace rna
