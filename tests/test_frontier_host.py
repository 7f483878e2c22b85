"""CPU-only checks of the exploration frontiers (rna_frontiers_build / _info_get / _download / _device_ptr, csrc/frontier.hip):
the entry points are exported and bound, rna_frontier and rna_frontier_info have the header's layout, the ABI version and the
profile slots did not move, argument checks that need no device, the kernels' resource budget on gfx950, and the C++
additions compile and link."""
import ctypes as C
import os
import subprocess

import numpy as np

from _build import (HOST, INCLUDE, LIB_DIR, c_values, capi, needs_hipcc, resources,  # noqa: F401  (capi: the fixture)
                    sources_in_build_files)

NEW = ["rna_frontiers_build", "rna_frontiers_info_get", "rna_frontiers_download", "rna_frontiers_device_ptr"]
RNA_EINVAL = -1


def test_new_symbols_are_exported_and_bound(capi):
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes, "%s has no ctypes signature" % s
    assert L.rna_frontiers_device_ptr.restype is C.c_void_p
    for m in ("frontiers", "frontier_labels", "frontier_labels_ptr", "frontiers_info"):
        assert callable(getattr(capi.Engine, m))


def test_struct_layouts_abi_version_and_profile_slots(capi, tmp_path):
    rec = ("label", "size", "min_i", "max_i", "min_j", "max_j", "nearest", "cost", "sum_i", "sum_j")
    info = ("cells", "clusters_all", "clusters", "largest", "min_size", "ranked", "stale", "reserved")
    got = c_values(tmp_path,
                   '  printf("%zu %zu %d %d %d\\n", sizeof(rna_frontier), sizeof(rna_frontier_info), RNA_FRONTIER_RANK, RNA_ABI_VERSION,'
                   ' (int)RNA_K_COUNT);\n'
                   + "".join('  printf("%%zu ", offsetof(rna_frontier, %s));\n' % f for f in rec)
                   + "".join('  printf("%%zu ", offsetof(rna_frontier_info, %s));\n' % f for f in info))
    F, D, I, DI = capi.Frontier, capi.FRONTIER_DTYPE, capi.FrontierInfo, capi.FRONTIER_INFO_DTYPE
    assert got[0] == C.sizeof(F) == D.itemsize == 48 and got[1] == C.sizeof(I) == DI.itemsize == 32
    assert got[2] == capi.FRONTIER_RANK == 1
    assert got[3] == 6 == capi.ABI_VERSION == capi.lib().rna_abi_version()      # entry points were added, nothing changed
    assert got[4] == len(capi.KERNELS) == 12 and capi.KERNELS[-1] == "footprint"      # no new profile slot
    want = [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    assert got[5:15] == [getattr(F, f).offset for f in rec] == [D.fields[f][1] for f in rec] == want
    assert D.names == rec and [D.fields[f][0] for f in rec] == [np.dtype("<i4")] * 8 + [np.dtype("<i8")] * 2
    # (nearest, cost) is one aligned 64-bit word with cost on top: the ranking minimum is one 64-bit atomic
    assert D.fields["nearest"][1] % 8 == 0 and D.fields["cost"][1] == D.fields["nearest"][1] + 4
    assert got[15:23] == [getattr(I, f).offset for f in info] == [DI.fields[f][1] for f in info] == list(range(0, 32, 4))
    assert DI.names == info and all(DI.fields[f][0] == np.dtype("<i4") for f in info)
    assert open(os.path.join(INCLUDE, "rna.h")).read().count('extern "C"') == 1


def test_argument_checks_that_need_no_device(capi):
    L = capi.lib()
    fake = C.c_void_p(1)     # never dereferenced: the argument checks come first
    out = np.zeros(4, capi.FRONTIER_DTYPE)
    info = np.zeros(1, capi.FRONTIER_INFO_DTYPE)
    P, I = out.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p)
    fn = L.rna_frontiers_build
    assert fn(None, 1, 0, P, 4, I) == RNA_EINVAL
    assert fn(fake, 0, 0, P, 4, I) == RNA_EINVAL                               # min_size < 1
    assert fn(fake, -3, 0, P, 4, I) == RNA_EINVAL
    assert fn(fake, 1, 0, P, -1, I) == RNA_EINVAL                              # cap < 0
    assert fn(fake, 1, 2, P, 4, I) == RNA_EINVAL                               # unknown flag bits
    assert fn(fake, 1, 0x80000001, P, 4, I) == RNA_EINVAL
    assert fn(fake, 1, 0, None, 4, I) == RNA_EINVAL                            # NULL out with cap > 0
    assert fn(fake, 1, 1, None, 1, None) == RNA_EINVAL
    assert not out.view(np.uint8).any() and not info.view(np.uint8).any()
    assert L.rna_frontiers_info_get(None, I) == RNA_EINVAL and L.rna_frontiers_info_get(fake, None) == RNA_EINVAL
    lab = np.zeros(4, np.int32)
    assert L.rna_frontiers_download(None, lab.ctypes.data_as(C.c_void_p), 4) == RNA_EINVAL
    assert L.rna_frontiers_download(fake, None, 4) == RNA_EINVAL
    assert L.rna_frontiers_device_ptr(None) is None


@needs_hipcc
def test_kernel_budget():
    """frontier.hip cross-compiles for gfx950; no kernel uses scratch, and static LDS stays at or below 40 KiB per workgroup:
    four tiles per compute unit (the classify kernel holds a 64 x 64 int32 parent tile, 16 KiB, plus its bit rows)"""
    res = resources("frontier.hip")
    want = {"fr_classify_kernel", "fr_seam_kernel", "fr_flatten_kernel", "fr_init_kernel", "fr_stats_kernel", "fr_compact_kernel"}
    assert len(res) == len(want) and all(any(w in k for k in res) for w in want), list(res)
    for k, v in res.items():
        assert v["ScratchSize"] == 0 and v["LDS"] <= 40 * 1024, (k, v)
    classify = [v for k, v in res.items() if "fr_classify_kernel" in k][0]
    assert 16 * 1024 <= classify["LDS"] <= 20 * 1024, classify


def test_sources_are_in_both_build_files():
    sources_in_build_files("frontier")


def test_cpp_additions_compile_and_link(capi, tmp_path):
    """move_control::Frontier, findFrontiers and GridGoalField::frontiers, against move_control_amd.hpp (C++11, as the
    host-mirror test compiles it) and against the reference-signature header"""
    src = tmp_path / "frontier_host.cpp"
    src.write_text(r'''
#include "move_control_amd.hpp"
int main(int argc, char**) {
  if (argc > 5) {   // compiled and linked, not run: constructing a GridMap needs a device
    grid_map::GridMap map;
    map.setGeometry(grid_map::Length(4.8, 4.0), 0.05);
    std::vector<move_control::Frontier> all, ranked;
    bool ok = move_control::findFrontiers(map, 3, all);
    grid_map::Position robot(1.0, 1.0);
    move_control::GridGoalField field(map, robot);
    ok = field.frontiers(3, ranked) && ok;
    double sum = 0.0;
    for (size_t k = 0; k < ranked.size(); ++k) {
      const move_control::Frontier& f = ranked[k];
      sum += f.centroid[0] + f.centroid[1] + f.size + f.cost + f.label[0] + f.nearest[1] + f.min[0] + f.max[1];
    }
    return ok && sum >= 0.0 ? 0 : 1;
  }
  return 0;
}
''')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + HOST, str(src), "-o", str(tmp_path / "frontier_host"), "-L" + LIB_DIR,
                           "-lrna", "-Wl,-rpath," + LIB_DIR, "-lpthread"])
    api = tmp_path / "frontier_api.cpp"
    api.write_text(r'''
#include "move_control_api.hpp"
bool f(grid_map::GridMap& map, std::vector<move_control::Frontier>& out) { return move_control::findFrontiers(map, 2, out); }
''')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-fsyntax-only", "-I" + HOST, str(api)])
