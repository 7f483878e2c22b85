"""CPU-only checks of the grid A*'s robot radius (rna_astar_set_robot_radius and friends, csrc/footprint.hip): the entry
points are exported and bound, the three places that name the ABI version agree, argument checks that need no device,
the C++ planner's new constructor argument compiles, and the footprint kernel's resource budget on gfx950."""
import ctypes as C
import os
import re
import subprocess

from _build import HPP, INCLUDE, LIB_DIR, capi, needs_hipcc, resources  # noqa: F401  (capi: the fixture)

NEW = ["rna_astar_set_robot_radius", "rna_astar_get_robot_radius", "rna_astar_download_blocked", "rna_if_blocked_batch",
       "rna_if_blocked_batch_device"]
RNA_EINVAL = -1


def test_new_symbols_are_exported_and_bound(capi):
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes, "%s has no ctypes signature" % s


def test_abi_version_is_6_everywhere(capi):
    hdr = open(os.path.join(INCLUDE, "rna.h")).read()
    assert int(re.search(r"#define RNA_ABI_VERSION (\d+)", hdr).group(1)) == 6
    assert capi.ABI_VERSION == 6 and capi.lib().rna_abi_version() == 6
    hpp = open(HPP).read()
    assert "RNA_ABI_VERSION >= 6" in hpp


def test_footprint_profile_slot_is_last(capi):
    assert capi.KERNELS[-1] == "footprint"
    assert capi.lib().rna_kernel_name(len(capi.KERNELS) - 1) == b"footprint"
    assert capi.lib().rna_kernel_name(len(capi.KERNELS)) == b"?"


def test_null_engine_and_null_buffers_are_einval(capi):
    L = capi.lib()
    r = C.c_double(7.0)
    buf = (C.c_uint8 * 4)()
    xy = (C.c_double * 2)(0.0, 0.0)
    assert L.rna_astar_set_robot_radius(None, 0.3) == RNA_EINVAL
    assert L.rna_astar_get_robot_radius(None, C.byref(r)) == RNA_EINVAL and r.value == 7.0
    assert L.rna_astar_download_blocked(None, buf, 4) == RNA_EINVAL
    assert L.rna_if_blocked_batch(None, xy, 1, 0.3, buf) == RNA_EINVAL
    assert L.rna_if_blocked_batch_device(None, xy, 1, 0.3, buf) == RNA_EINVAL


def test_grid_astar_planner_robot_radius_compiles(capi, tmp_path):
    src = tmp_path / "planner_radius.cpp"
    src.write_text(r'''
#include "%s"
int main(int argc, char**) {
  if (argc > 5) {   // compiled and linked, not run: constructing a GridMap needs a device
    grid_map::GridMap map;
    map.setGeometry(grid_map::Length(4.8, 4.0), 0.05);
    move_control::GridAStarPlanner planner(map, 1, 0.3);
    planner.setRobotRadius(0.25);
    return planner.getRobotRadius() == 0.25 ? 0 : 1;
  }
  move_control::GridAStarPlanner* (*make)(grid_map::GridMap&) = nullptr;
  (void)make;
  return 0;
}
''' % HPP)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", str(src), "-o", str(tmp_path / "planner_radius"), "-L" + LIB_DIR, "-lrna",
                           "-Wl,-rpath," + LIB_DIR, "-lpthread"])


@needs_hipcc
def test_footprint_kernel_budget():
    """footprint_tiles_kernel (one 256-thread workgroup per 64 x 64 tile) and the if_blocked kernel compile for gfx950
    without scratch; the tile kernel's LDS (occupancy bits of the tile with a 64-cell halo + its blocked bytes) stays
    small enough for many workgroups per CU."""
    res = resources("footprint.hip")
    tiles = next(v for k, v in res.items() if "footprint_tiles_kernel" in k)
    point = next(v for k, v in res.items() if "if_blocked_kernel" in k)
    assert tiles["ScratchSize"] == 0 and point["ScratchSize"] == 0, res
    assert tiles["LDS"] <= 16 * 1024, tiles
    assert tiles["VGPRs"] <= 64, tiles     # eight wavefronts per SIMD
