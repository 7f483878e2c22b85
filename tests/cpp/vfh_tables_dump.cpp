// build_tables and VfhLayout of csrc/vfh_tables.hpp on the host alone, for tests/test_vfh_tables_host.py:
//   vfh_tables_dump <the twenty values of rna_vfh_params in the header's order> [n_robots ...]
// prints "dims W H T CX CY YH NQ NQF NW max_speed", for every n_robots given (and for 0, whose table half locates the
// sub-arrays of the block below) "layout <n_robots> table_bytes state_bytes" followed by "<name> <offset> <bytes>" of every
// sub-array, then "block <bytes>" and the table block itself.  Parameters that build_tables refuses: "refused", exit code 2.
#include <cstdio>
#include <cstdlib>

#include "../../ros_navigation_amd/csrc/vfh_tables.hpp"

using namespace rna;

int main(int argc, char** argv) {
  if (argc < 21) return 64;
  int at = 1;
  auto d = [&] { return std::strtod(argv[at++], nullptr); };
  auto i = [&] { return (int32_t)std::strtol(argv[at++], nullptr, 10); };
  rna_vfh_params p;
  p.cell_size = d(); p.window_diameter = i(); p.sector_angle = i(); p.safety_dist_0ms = d(); p.safety_dist_1ms = d();
  p.max_speed = i(); p.max_speed_narrow_opening = i(); p.max_speed_wide_opening = i(); p.max_acceleration = i();
  p.min_turnrate = i(); p.max_turnrate_0ms = i(); p.max_turnrate_1ms = i(); p.min_turn_radius_safety_factor = d();
  p.free_space_cutoff_0ms = d(); p.obs_cutoff_0ms = d(); p.free_space_cutoff_1ms = d(); p.obs_cutoff_1ms = d();
  p.weight_desired_dir = d(); p.weight_current_dir = d(); p.robot_radius = d();
  HostTables t;
  if (!build_tables(p, t)) {
    std::printf("refused\n");
    return 2;
  }
  std::printf("dims %d %d %d %d %d %d %d %d %d %d\n", t.W, t.H, t.T, t.CX, t.CY, t.YH, t.NQ, t.NQF, t.NW, t.max_speed);
  for (int k = 20; k < argc; ++k) {
    const size_t n = k == 20 ? 0 : (size_t)std::strtoull(argv[k], nullptr, 10);
    const VfhLayout L(t, n);
    std::printf("layout %zu %zu %zu\n", n, L.table_bytes, L.state_bytes);
#define SPAN(name) std::printf(#name " %zu %zu\n", L.name.off, L.name.bytes)
    SPAN(cell_dist); SPAN(cell_base_mag); SPAN(cell_dir); SPAN(range_idx); SPAN(memb); SPAN(in_circle); SPAN(min_turning_radius); SPAN(bcr);
    SPAN(last_binary); SPAN(hist); SPAN(origin); SPAN(picked); SPAN(last_picked); SPAN(blocked_radius); SPAN(last_chosen_speed);
    SPAN(max_speed_picked);
  }
  std::printf("block %zu\n", t.block.size());
  return std::fwrite(t.block.data(), 1, t.block.size(), stdout) == t.block.size() ? 0 : 1;
}
