"""CPU-only checks of the view-point information gain (rna_view_gain / rna_view_gain_device, csrc/viewgain.hip): the entry
points are exported and bound, struct rna_view_gain has the header's layout, the two constants, the ABI version and the profile
slots did not move, argument checks that need no device, the kernel's resource budget on gfx950, and the C++ additions
compile and link."""
import ctypes as C
import os
import subprocess

import numpy as np

from _build import (HOST, INCLUDE, LIB_DIR, c_values, capi, needs_hipcc, resources,  # noqa: F401  (capi: the fixture)
                    sources_in_build_files)

NEW = ["rna_view_gain", "rna_view_gain_device"]
RNA_EINVAL, RNA_ECAPACITY = -1, -4
FIELDS = ("status", "unknown", "visible", "occupied")


def test_new_symbols_are_exported_and_bound(capi):
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes, "%s has no ctypes signature" % s
    for m in ("view_gain", "view_gain_device", "frontier_view_gain"):
        assert callable(getattr(capi.Engine, m))


def test_struct_layout_constants_abi_version_and_profile_slots(capi, tmp_path):
    got = c_values(tmp_path,
                   '  printf("%zu %d %d %d %d\\n", sizeof(struct rna_view_gain), RNA_VIEW_MAX_RADIUS, RNA_VIEW_UNKNOWN_OPAQUE,'
                   ' RNA_ABI_VERSION, (int)RNA_K_COUNT);\n'
                   + "".join('  printf("%%zu ", offsetof(struct rna_view_gain, %s));\n' % f for f in FIELDS))
    V, D = capi.ViewGain, capi.VIEW_GAIN_DTYPE
    assert got[0] == C.sizeof(V) == D.itemsize == 16
    assert got[1] == capi.VIEW_MAX_RADIUS == 127 and got[2] == capi.VIEW_UNKNOWN_OPAQUE == 1
    assert got[3] == 6 == capi.ABI_VERSION == capi.lib().rna_abi_version()      # entry points were added, nothing changed
    assert got[4] == len(capi.KERNELS) == 12 and capi.KERNELS[-1] == "footprint"      # no new profile slot
    assert got[5:9] == [getattr(V, f).offset for f in FIELDS] == [D.fields[f][1] for f in FIELDS] == [0, 4, 8, 12]
    assert D.names == FIELDS and all(D.fields[f][0] == np.dtype("<i4") for f in FIELDS)
    assert open(os.path.join(INCLUDE, "rna.h")).read().count('extern "C"') == 1


def test_argument_checks_that_need_no_device(capi):
    L = capi.lib()
    fake = C.c_void_p(1)     # never dereferenced: the argument checks come first
    cells = np.zeros(4, np.int32)
    out = np.zeros(4, capi.VIEW_GAIN_DTYPE)
    out.view(np.uint8)[:] = 0xA5
    before = out.tobytes()
    P, O = cells.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for fn in (L.rna_view_gain, L.rna_view_gain_device):
        assert fn(None, P, 4, 10, 0, O) == RNA_EINVAL
        assert fn(fake, P, -1, 10, 0, O) == RNA_EINVAL                         # n < 0
        assert fn(fake, P, 4, 0, 0, O) == RNA_EINVAL                           # radius < 1
        assert fn(fake, P, 4, -5, 1, O) == RNA_EINVAL
        assert fn(fake, P, 4, 10, 2, O) == RNA_EINVAL                          # unknown flag bits
        assert fn(fake, P, 4, 10, 0x80000001, O) == RNA_EINVAL
        assert fn(fake, None, 4, 10, 0, O) == RNA_EINVAL                       # NULL buffers with n > 0
        assert fn(fake, P, 4, 10, 1, None) == RNA_EINVAL
        assert fn(fake, P, 0, 0, 0, O) == RNA_EINVAL                           # ... the radius is checked for n == 0 too
        assert fn(fake, None, 0, 10, 1, None) == 0                             # n == 0 with valid arguments: nothing to do
    assert out.tobytes() == before
    # (RNA_ECAPACITY beyond RNA_VIEW_MAX_RADIUS writes the engine's error text: it needs a real engine,
    # tests/test_gpu_view_gain.py has it)


@needs_hipcc
def test_kernel_budget():
    """viewgain.hip cross-compiles for gfx950 with one kernel; it uses no scratch, and its static LDS plus the dynamic share of
    the largest radius (three bitmaps of 255 rows x 8 words) stays at or below 32 KiB: at least four workgroups fit the LDS of
    a compute unit"""
    res = resources("viewgain.hip")
    assert len(res) == 1 and "view_gain_kernel" in list(res)[0], list(res)
    v = list(res.values())[0]
    R = 127
    W = 2 * R + 1
    dynamic = 3 * W * ((W + 31) // 32) * 4
    assert dynamic == 24480
    assert v["ScratchSize"] == 0 and v["LDS"] + dynamic <= 32 * 1024, v


def test_sources_are_in_both_build_files():
    sources_in_build_files("viewgain")


def test_cpp_additions_compile_and_link(capi, tmp_path):
    """move_control::ViewGain, viewGain and GridGoalField::frontierGains, against move_control_amd.hpp (C++11, as the
    host-mirror test compiles it) and against the reference-signature header"""
    src = tmp_path / "view_gain_host.cpp"
    src.write_text(r'''
#include "move_control_amd.hpp"
int main(int argc, char**) {
  if (argc > 5) {   // compiled and linked, not run: constructing a GridMap needs a device
    grid_map::GridMap map;
    map.setGeometry(grid_map::Length(4.8, 4.0), 0.05);
    std::vector<grid_map::Position> at(2, grid_map::Position(1.0, 1.0));
    std::vector<move_control::ViewGain> gains, pessimistic, at_frontiers;
    bool ok = move_control::viewGain(map, at, 3.0, gains);
    ok = move_control::viewGain(map, at, 3.0, pessimistic, true) && ok;
    grid_map::Position robot(1.0, 1.0);
    move_control::GridGoalField field(map, robot);
    std::vector<move_control::Frontier> ranked;
    ok = field.frontiers(3, ranked) && field.frontierGains(ranked, 3.0, at_frontiers) && ok;
    long sum = 0;
    for (size_t k = 0; k < at_frontiers.size(); ++k) {
      const move_control::ViewGain& g = at_frontiers[k];
      sum += g.unknown + g.visible + g.occupied + g.status;
    }
    struct rna_view_gain raw = {0, 0, 0, 0};
    const int32_t cell = 0;
    ok = rna_view_gain_device(map.engine(), &cell, 0, 1, 0u, &raw) == RNA_OK && ok;
    return ok && sum >= 0 ? 0 : 1;
  }
  return 0;
}
''')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + HOST, str(src), "-o", str(tmp_path / "view_gain_host"), "-L" + LIB_DIR,
                           "-lrna", "-Wl,-rpath," + LIB_DIR, "-lpthread"])
    api = tmp_path / "view_gain_api.cpp"
    api.write_text(r'''
#include "move_control_api.hpp"
bool f(grid_map::GridMap& map, const std::vector<grid_map::Position>& at, std::vector<move_control::ViewGain>& out) {
  return move_control::viewGain(map, at, 2.5, out, true);
}
bool g(move_control::GridGoalField& field, const std::vector<move_control::Frontier>& fr, std::vector<move_control::ViewGain>& out) {
  return field.frontierGains(fr, 2.5, out);
}
''')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-fsyntax-only", "-I" + HOST, str(api)])
