"""CPU-only checks of the goal field with many sources and owner labels (rna_goal_field_build_multi and friends,
csrc/goal_field.hip): the entry points are exported, bound and listed, the info struct and the flag agree between the header,
a compiled C snippet and the Python mirror, argument checks that need no device, the C++ additions compile and link, and
the kernels' resource budget on gfx950."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from _build import HPP, LIB_DIR, c_values, capi, needs_hipcc, resources  # noqa: F401  (capi: the fixture)

NEW = ["rna_goal_field_build_multi", "rna_goal_field_build_multi_device", "rna_goal_field_sources_info_get",
       "rna_goal_field_owners_download", "rna_goal_field_owners_device_ptr", "rna_goal_field_owners_at"]
RNA_EINVAL = -1


def test_symbols_list_contains_the_six_new_names():
    """needs neither a device nor a build: the binding module alone"""
    from ros_navigation_amd import capi as binding
    assert set(NEW) <= set(binding.SYMBOLS) and len(set(binding.SYMBOLS)) == len(binding.SYMBOLS)


def test_new_symbols_are_exported_and_bound(capi):
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes, "%s has no ctypes signature" % s
    assert L.rna_goal_field_owners_device_ptr.restype is C.c_void_p
    for m in ("goal_field_multi", "goal_field_multi_device", "goal_field_sources_info", "goal_field_owners", "goal_field_owners_ptr",
              "goal_field_owners_at", "goal_field_from_frontiers"):
        assert callable(getattr(capi.Engine, m))


def test_sources_info_struct_and_flag_match_the_header(capi, tmp_path):
    got = c_values(tmp_path, r'''
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %zu\n", sizeof(rna_goal_field_sources_info), offsetof(rna_goal_field_sources_info, sources),
         offsetof(rna_goal_field_sources_info, blocked_sources), offsetof(rna_goal_field_sources_info, terminals),
         offsetof(rna_goal_field_sources_info, owners), offsetof(rna_goal_field_sources_info, owner_rounds),
         offsetof(rna_goal_field_sources_info, reserved), sizeof(((rna_goal_field_sources_info*)0)->reserved), RNA_GOAL_FIELD_OWNERS,
         RNA_ABI_VERSION, sizeof(rna_goal_field_info));''')
    dt = capi.GOAL_FIELD_SOURCES_INFO_DTYPE
    names = ("sources", "blocked_sources", "terminals", "owners", "owner_rounds", "reserved")
    assert dt.names == names
    assert got[0] == dt.itemsize == 32
    assert got[1:7] == [dt.fields[n][1] for n in names]
    assert got[7] == 12 == dt.fields["reserved"][0].itemsize
    assert got[8] == capi.GOAL_FIELD_OWNERS == 1
    assert got[9] == capi.ABI_VERSION == 6          # entry points were added, nothing changed: the ABI version stays
    assert got[10] == capi.GOAL_FIELD_INFO_DTYPE.itemsize == 32     # rna_goal_field_info keeps its layout


def test_null_engine_and_bad_arguments_are_einval(capi):
    L = capi.lib()
    info = np.full(1, 7, capi.GOAL_FIELD_INFO_DTYPE)
    src = np.full(1, 7, capi.GOAL_FIELD_SOURCES_INFO_DTYPE)
    cells = (C.c_int32 * 8)()
    fake = C.c_void_p(1)     # never dereferenced: the argument checks that are tested with it come first
    for fn in (L.rna_goal_field_build_multi, L.rna_goal_field_build_multi_device):
        assert fn(None, cells, cells, 8, 0, info.ctypes.data) == RNA_EINVAL
        assert fn(None, cells, None, 8, 1, None) == RNA_EINVAL
    assert info["goal"][0] == 7
    assert L.rna_goal_field_sources_info_get(None, src.ctypes.data) == RNA_EINVAL and src["sources"][0] == 7
    assert L.rna_goal_field_sources_info_get(fake, None) == RNA_EINVAL
    assert L.rna_goal_field_owners_download(None, cells, 8) == RNA_EINVAL
    assert L.rna_goal_field_owners_download(fake, None, 8) == RNA_EINVAL
    assert L.rna_goal_field_owners_device_ptr(None) is None
    assert L.rna_goal_field_owners_at(None, cells, 8, cells) == RNA_EINVAL
    assert L.rna_goal_field_owners_at(fake, cells, -1, cells) == RNA_EINVAL
    assert L.rna_goal_field_owners_at(fake, None, 8, cells) == RNA_EINVAL
    assert L.rna_goal_field_owners_at(fake, cells, 8, None) == RNA_EINVAL


@pytest.mark.parametrize("header", ["move_control_amd.hpp", "move_control_api.hpp"])
def test_multi_goal_class_compiles_and_links(capi, tmp_path, header):
    """through the core header and through the header with the reference's signatures, which re-exports the class"""
    src = tmp_path / "goal_field_multi_host.cpp"
    src.write_text(r'''
#include "%s"
int main(int argc, char**) {
  if (argc > 5) {   // compiled and linked, not run: constructing a GridMap needs a device
    grid_map::GridMap map;
    map.setGeometry(grid_map::Length(4.8, 4.0), 0.05);
    std::vector<grid_map::Position> robots;
    robots.push_back(grid_map::Position(1.0, 1.0));
    robots.push_back(grid_map::Position(-1.0, -0.5));
    std::vector<int32_t> busy;
    busy.push_back(0);
    busy.push_back(12000);
    move_control::GridGoalField nearest(map, robots);
    move_control::GridGoalField field(map, robots, busy, true);
    grid_map::Position start(0.2, 0.3);
    std::vector<grid_map::Position> path;
    int32_t cost = 0;
    bool ok = field.makePlan(start, path) && field.costToGoal(start, cost) && field.ownerOf(start) >= 0;
    if (field.stale()) ok = field.rebuild() && ok;
    field.setShortcut(0, false);
    std::vector<move_control::Frontier> fr;
    ok = field.frontiers(3, fr) && ok;
    std::vector<int> who = field.assignFrontiers(fr);
    rna_goal_field_sources_info s;
    ok = rna_goal_field_sources_info_get(map.engine(), &s) == RNA_OK && ok;
    return ok && who.size() == fr.size() && field.info().reached > 0 && s.owners == RNA_GOAL_FIELD_OWNERS ? 0 : 1;
  }
  return 0;
}
''' % HPP.replace("move_control_amd.hpp", header))
    subprocess.check_call(["g++", "-std=c++11", "-Wall", str(src), "-o", str(tmp_path / "goal_field_multi_host"), "-L" + LIB_DIR, "-lrna",
                           "-Wl,-rpath," + LIB_DIR, "-lpthread"])


@needs_hipcc
def test_goal_field_multi_kernel_budget():
    """No kernel of goal_field.hip uses scratch.  The owner pass: the tile kernel (one 256-thread workgroup per 64 x 64 tile)
    holds two copies of the tile's 4096 successor indices as uint16 (2 x 8 KiB) and one int32 root value per cell (16 KiB):
    32 KiB, so LDS <= 40 KiB leaves four workgroups to a CU's 160 KiB as the relaxation kernel has, and VGPRs <= 128 four
    wavefronts to a SIMD; the jump kernel is one word in, one word out per cell and uses no LDS at all.  The limits of
    test_goal_field_kernel_budget hold for the kernels it names, which this feature touched (seed, finalize) or left alone."""
    res = resources("goal_field.hip")

    def of(k):
        found = [v for n, v in res.items() if k in n]
        assert found, (k, sorted(res))
        return found

    for n, v in res.items():
        assert v["ScratchSize"] == 0, (n, v)
    for v in of("gf_owner_tile_kernel"):
        assert v["LDS"] <= 40 * 1024 and v["VGPRs"] <= 128, v
    assert len(of("gf_owner_jump_kernel")) == 2                                 # the border rounds and the gather
    for v in of("gf_owner_jump_kernel"):
        assert v["LDS"] == 0, v
    for k in ("gf_init_kernel", "gf_seed_kernel", "gf_terminal_kernel"):
        assert len(of(k)) == 1
    for v in of("gf_round_kernel"):
        assert v["LDS"] <= 40 * 1024 and v["VGPRs"] <= 128, v
    for v in of("gf_finalize_kernel"):
        assert v["LDS"] <= 40 * 1024, v
    for v in of("gf_paths_kernel"):
        assert v["LDS"] <= 8 * 1024 and v["VGPRs"] <= 64, v
