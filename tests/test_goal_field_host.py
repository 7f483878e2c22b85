"""CPU-only checks of the goal distance field (rna_goal_field_*, csrc/goal_field.hip): the entry points are exported and
bound, the info struct and the two sentinels agree between the header, a compiled C snippet and the Python mirror, argument
checks that need no device, the C++ host class compiles and links, and the kernels' resource budget on gfx950."""
import ctypes as C
import subprocess

import numpy as np

from _build import HPP, LIB_DIR, c_values, capi, needs_hipcc, resources  # noqa: F401  (capi: the fixture)

NEW = ["rna_goal_field_build", "rna_goal_field_info_get", "rna_goal_field_download", "rna_goal_field_device_ptr",
       "rna_goal_field_paths", "rna_goal_field_paths_device"]
RNA_EINVAL = -1


def test_new_symbols_are_exported_and_bound(capi):
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes, "%s has no ctypes signature" % s
    for m in ("goal_field", "goal_field_info", "goal_field_download", "goal_field_ptr", "goal_field_paths", "goal_field_paths_device"):
        assert callable(getattr(capi.Engine, m))


def test_info_struct_and_sentinels_match_the_header(capi, tmp_path):
    got = c_values(tmp_path, r'''
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(rna_goal_field_info), offsetof(rna_goal_field_info, goal),
         offsetof(rna_goal_field_info, status), offsetof(rna_goal_field_info, reached), offsetof(rna_goal_field_info, max_cost),
         offsetof(rna_goal_field_info, rounds), offsetof(rna_goal_field_info, tile_jobs), offsetof(rna_goal_field_info, tiles_reached),
         offsetof(rna_goal_field_info, stale), RNA_GOAL_FIELD_UNREACHED, RNA_GOAL_FIELD_FAR, RNA_ABI_VERSION);''')
    dt = capi.GOAL_FIELD_INFO_DTYPE
    names = ("goal", "status", "reached", "max_cost", "rounds", "tile_jobs", "tiles_reached", "stale")
    assert dt.names == names
    assert got[0] == dt.itemsize == 32
    assert got[1:9] == [dt.fields[n][1] for n in names]
    assert got[9] == capi.GOAL_FIELD_UNREACHED == 0x7fffffff and got[10] == capi.GOAL_FIELD_FAR == 0x7ffffffe
    assert got[11] == 6          # entry points were added, nothing changed: the ABI version stays


def test_null_engine_null_buffers_and_bad_counts_are_einval(capi):
    L = capi.lib()
    info = np.full(1, 7, capi.GOAL_FIELD_INFO_DTYPE)
    cells = (C.c_int32 * 8)()
    nx = (C.c_uint8 * 8)()
    res = np.zeros(2, capi.ASTAR_RESULT_DTYPE)
    assert L.rna_goal_field_build(None, 0, info.ctypes.data) == RNA_EINVAL
    assert L.rna_goal_field_info_get(None, info.ctypes.data) == RNA_EINVAL and info["goal"][0] == 7
    fake = C.c_void_p(1)     # never dereferenced: the argument checks come first
    assert L.rna_goal_field_info_get(fake, None) == RNA_EINVAL
    assert L.rna_goal_field_download(None, cells, nx, 8) == RNA_EINVAL
    assert L.rna_goal_field_device_ptr(None) is None
    for fn in (L.rna_goal_field_paths, L.rna_goal_field_paths_device):
        assert fn(None, cells, 2, cells, 4, res.ctypes.data) == RNA_EINVAL
        assert fn(fake, cells, -1, cells, 4, res.ctypes.data) == RNA_EINVAL
        assert fn(fake, cells, 2, cells, 0, res.ctypes.data) == RNA_EINVAL
        assert fn(fake, None, 2, cells, 4, res.ctypes.data) == RNA_EINVAL
        assert fn(fake, cells, 2, None, 4, res.ctypes.data) == RNA_EINVAL
        assert fn(fake, cells, 2, cells, 4, None) == RNA_EINVAL


def test_grid_goal_field_class_compiles_and_links(capi, tmp_path):
    src = tmp_path / "goal_field_host.cpp"
    src.write_text(r'''
#include "%s"
int main(int argc, char**) {
  if (argc > 5) {   // compiled and linked, not run: constructing a GridMap needs a device
    grid_map::GridMap map;
    map.setGeometry(grid_map::Length(4.8, 4.0), 0.05);
    grid_map::Position goal(1.0, 1.0), start(-1.0, -0.5);
    move_control::GridGoalField field(map, goal);
    std::vector<grid_map::Position> path;
    int32_t cost = 0;
    bool ok = field.makePlan(start, path) && field.costToGoal(start, cost);
    if (field.stale()) ok = field.rebuild() && ok;
    return ok && field.info().reached > 0 ? 0 : 1;
  }
  return 0;
}
''' % HPP)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", str(src), "-o", str(tmp_path / "goal_field_host"), "-L" + LIB_DIR, "-lrna",
                           "-Wl,-rpath," + LIB_DIR, "-lpthread"])


@needs_hipcc
def test_goal_field_kernel_budget():
    """Every kernel of goal_field.hip compiles for gfx950 without scratch.  Budget of the relaxation kernel (one 256-thread
    workgroup per 64 x 64 tile): the tile's field with a one-cell halo (66 rows of 67 words, 17.3 KiB), its mask bytes in
    both lane layouts (2 x 4 KiB) and a few words must leave room for at least 4 workgroups per CU -- a round holds a few
    hundred tile jobs whose sweeps wait on LDS round trips, so it is other workgroups on the CU that hide them: LDS <= 40 KiB
    (4 x 40 = the CU's 160 KiB) and VGPRs <= 128 (4 wavefronts per SIMD of 512 registers per lane)."""
    res = resources("goal_field.hip")
    kernels = {k: next(v for n, v in res.items() if k in n) for k in
               ("gf_init_kernel", "gf_seed_kernel", "gf_round_kernel", "gf_finalize_kernel", "gf_paths_kernel")}
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0, (k, v)
    assert kernels["gf_round_kernel"]["LDS"] <= 40 * 1024 and kernels["gf_round_kernel"]["VGPRs"] <= 128, kernels["gf_round_kernel"]
    assert kernels["gf_finalize_kernel"]["LDS"] <= 40 * 1024
    assert kernels["gf_paths_kernel"]["LDS"] <= 8 * 1024 and kernels["gf_paths_kernel"]["VGPRs"] <= 64, kernels["gf_paths_kernel"]
