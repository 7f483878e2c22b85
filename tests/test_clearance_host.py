"""CPU-only checks of the clearance field (rna_clearance_*, csrc/clearance.hip) and the goal field's clearance cost
(rna_goal_field_set / _get_clearance_cost): the entry points are exported and bound, RNA_CLEARANCE_NONE agrees between the
header, a compiled C snippet and the Python mirror, the ABI version and the profile slots did not move, argument checks that
need no device, the C++ additions compile and link, the inflation curve is the same table in C++ and in Python, and the
kernels' resource budgets on gfx950."""
import ctypes as C
import subprocess

import numpy as np

from _build import HPP, LIB_DIR, c_values, capi, needs_hipcc, resources  # noqa: F401  (capi: the fixture)

NEW = ["rna_clearance_build", "rna_clearance_download", "rna_clearance_device_ptr", "rna_clearance_info_get",
       "rna_goal_field_set_clearance_cost", "rna_goal_field_get_clearance_cost"]
RNA_EINVAL = -1


def test_new_symbols_are_exported_and_bound(capi):
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes, "%s has no ctypes signature" % s
    for m in ("clearance", "clearance_download", "clearance_ptr", "clearance_info", "goal_field_clearance_cost"):
        assert callable(getattr(capi.Engine, m))
    assert callable(capi.inflation_cost_table)


def test_sentinel_abi_version_and_profile_slots(capi, tmp_path):
    got = c_values(tmp_path, r'''
  uint16_t v = RNA_CLEARANCE_NONE;
  printf("%d %d %d %d\n", RNA_CLEARANCE_NONE, (int)v, RNA_ABI_VERSION, (int)RNA_K_COUNT);''')
    assert got[0] == got[1] == capi.CLEARANCE_NONE == 0xFFFF
    assert got[2] == 6 == capi.ABI_VERSION == capi.lib().rna_abi_version()      # entry points were added, nothing changed
    assert got[3] == len(capi.KERNELS) and capi.KERNELS[-1] == "footprint"      # no new profile slot
    assert capi.lib().rna_kernel_name(len(capi.KERNELS) - 1) == b"footprint"


def test_null_engine_null_buffers_and_bad_counts_are_einval(capi):
    L = capi.lib()
    buf = (C.c_uint16 * 64)()
    r, st = C.c_int(7), C.c_int(7)
    fake = C.c_void_p(1)     # never dereferenced: the argument checks come first
    assert L.rna_clearance_build(None, 7) == RNA_EINVAL
    assert L.rna_clearance_build(fake, 0) == RNA_EINVAL and L.rna_clearance_build(fake, 64) == RNA_EINVAL
    assert L.rna_clearance_build(fake, -3) == RNA_EINVAL
    assert L.rna_clearance_download(None, buf, 64) == RNA_EINVAL
    assert L.rna_clearance_download(fake, None, 64) == RNA_EINVAL
    assert L.rna_clearance_device_ptr(None) is None
    assert L.rna_clearance_info_get(None, C.byref(r), C.byref(st)) == RNA_EINVAL and (r.value, st.value) == (7, 7)
    assert L.rna_clearance_info_get(fake, None, C.byref(st)) == RNA_EINVAL
    assert L.rna_clearance_info_get(fake, C.byref(r), None) == RNA_EINVAL
    assert L.rna_goal_field_set_clearance_cost(None, buf, 8) == RNA_EINVAL
    assert L.rna_goal_field_set_clearance_cost(None, None, 0) == RNA_EINVAL
    for n in (1, 65, -1):
        assert L.rna_goal_field_set_clearance_cost(fake, buf, n) == RNA_EINVAL
    assert L.rna_goal_field_set_clearance_cost(fake, None, 8) == RNA_EINVAL
    assert L.rna_goal_field_get_clearance_cost(None, buf, 64) == RNA_EINVAL
    assert L.rna_goal_field_get_clearance_cost(fake, None, 4) == RNA_EINVAL
    assert L.rna_goal_field_get_clearance_cost(fake, buf, -1) == RNA_EINVAL


def test_cpp_additions_compile_and_link(capi, tmp_path):
    src = tmp_path / "clearance_host.cpp"
    src.write_text(r'''
#include "%s"
int main(int argc, char**) {
  if (argc > 5) {   // compiled and linked, not run: constructing a GridMap needs a device
    grid_map::GridMap map;
    map.setGeometry(grid_map::Length(4.8, 4.0), 0.05);
    std::vector<uint16_t> clr;
    map.clearance(20, clr);
    grid_map::Position goal(1.0, 1.0), start(-1.0, -0.5);
    const std::vector<uint16_t> table = move_control::inflationCostTable(0.05, 0.15, 0.55, 10.0, 5000.0);
    move_control::GridGoalField field(map, goal, table);
    std::vector<grid_map::Position> path;
    bool ok = field.makePlan(start, path) && field.clearanceCost() == table;
    field.setClearanceCost(std::vector<uint16_t>());
    if (field.stale()) ok = field.rebuild() && ok;
    return ok && clr[0] != RNA_CLEARANCE_NONE ? 0 : 1;
  }
  return 0;
}
''' % HPP)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", str(src), "-o", str(tmp_path / "clearance_host"), "-L" + LIB_DIR, "-lrna",
                           "-Wl,-rpath," + LIB_DIR, "-lpthread"])


PARAMS = [(0.05, 0.15, 0.55, 10.0, 5000.0),      # costmap_2d's defaults at the project's resolution
          (0.1, 0.0, 3.0, 1.5, 70000.0),         # clipped to 65535 near the obstacle, 31 entries
          (0.05, 0.3, 10.0, 3.0, 253.0),         # an inflation radius beyond the 63-cell cap: 64 entries
          (0.25, 0.2, 0.1, 4.0, 900.0)]          # an inflation radius below one cell: the shortest table


def test_inflation_cost_table_is_the_same_in_cpp_and_python(capi, tmp_path):
    src = tmp_path / "inflation.cpp"
    calls = "\n".join('  show(move_control::inflationCostTable(%r, %r, %r, %r, %r));' % p for p in PARAMS)
    src.write_text(r'''
#include <cstdio>
#include "%s"
static void show(const std::vector<uint16_t>& t) {
  for (size_t k = 0; k < t.size(); ++k) printf("%%u ", (unsigned)t[k]);
  printf("\n");
}
int main() {
%s
  return 0;
}
''' % (HPP, calls))
    exe = tmp_path / "inflation"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", str(src), "-o", str(exe), "-L" + LIB_DIR, "-lrna", "-Wl,-rpath," + LIB_DIR,
                           "-lpthread"])
    lines = subprocess.check_output([str(exe)]).decode().strip().split("\n")
    assert len(lines) == len(PARAMS)
    for p, line in zip(PARAMS, lines):
        want = capi.inflation_cost_table(*p)
        assert want.dtype == np.uint16 and 2 <= len(want) <= 64
        assert [int(v) for v in line.split()] == [int(v) for v in want], p
    t = capi.inflation_cost_table(*PARAMS[0])
    assert len(t) == 12 and t[0] == t[3] == 5000 and t[4] == 3033 and t[11] == 92       # 5000 exp(-10 (0.05 k - 0.15))
    assert (np.diff(t[3:].astype(int)) < 0).all()
    assert capi.inflation_cost_table(*PARAMS[1])[0] == 65535 and len(capi.inflation_cost_table(*PARAMS[1])) == 31
    assert len(capi.inflation_cost_table(*PARAMS[2])) == 64
    assert list(capi.inflation_cost_table(*PARAMS[3])) == [900, 0]


@needs_hipcc
def test_kernel_budgets():
    """clearance.hip: no kernel uses scratch; the tile kernel (one 256-thread workgroup per 64 x 64 tile, the blocked bits of
    the tile with a 63-cell halo in LDS) stays inside the footprint kernel's own budget, LDS <= 16 KiB and VGPRs <= 64.
    goal_field.hip: EVERY instantiation of the relaxation and finalize kernels, with and without the clearance cost, stays
    inside the goal field's budget (tests/test_goal_field_host.py): LDS <= 40 KiB, VGPRs <= 128, no scratch."""
    clr = resources("clearance.hip")
    assert clr and all(v["ScratchSize"] == 0 for v in clr.values()), clr
    tiles = [v for k, v in clr.items() if "clearance_tiles_kernel" in k]
    assert len(tiles) == 1 and tiles[0]["LDS"] <= 16 * 1024 and tiles[0]["VGPRs"] <= 64, tiles
    gf = resources("goal_field.hip")
    rounds = {k: v for k, v in gf.items() if "gf_round_kernel" in k}
    finals = {k: v for k, v in gf.items() if "gf_finalize_kernel" in k}
    assert len(rounds) == 2 and len(finals) == 2, (list(rounds), list(finals))      # with and without the cost
    for k, v in list(rounds.items()) + list(finals.items()):
        assert v["ScratchSize"] == 0 and v["LDS"] <= 40 * 1024 and v["VGPRs"] <= 128, (k, v)
    assert len({v["LDS"] for v in rounds.values()}) == 2                             # the cost's LDS is in one of them only
