"""CPU-only checks of the line-of-sight shortcut (rna_shortcut_paths[_device], rna_line_cells_index, csrc/shortcut.hip): the
entry points are exported and bound, rna_shortcut_result has the header's layout, the ABI version and the profile slots did
not move, rna_line_cells_index -- the closed form the kernel walks a leg with -- equals the oracle's restatement of the
reference's LineIterator(map, Index, Index) (og_line_cells_index, pinned to the reference's compiled code by
tests/test_oracle_refpin.py), argument checks that need no device, the kernel's resource budget on gfx950, and the C++
additions compile and link."""
import ctypes as C
import subprocess

import numpy as np

import _oracle as O
from _build import (HOST, LIB_DIR, c_values, capi, needs_hipcc, resources,  # noqa: F401  (capi: the fixture)
                    sources_in_build_files)

NEW = ["rna_shortcut_paths", "rna_shortcut_paths_device", "rna_line_cells_index"]
RNA_EINVAL = -1


def test_new_symbols_are_exported_and_bound(capi):
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes, "%s has no ctypes signature" % s
    for m in ("shortcut_paths", "shortcut_paths_device"):
        assert callable(getattr(capi.Engine, m))
    assert callable(capi.line_cells_index)


def test_struct_layout_abi_version_and_profile_slots(capi, tmp_path):
    got = c_values(tmp_path, r'''
  printf("%zu %zu %zu %zu %zu %d %d %d %d\n", sizeof(rna_shortcut_result), offsetof(rna_shortcut_result, status),
         offsetof(rna_shortcut_result, n_waypoints), offsetof(rna_shortcut_result, blocked_steps),
         offsetof(rna_shortcut_result, longest_span), RNA_SHORTCUT_KEEP_CLEARANCE, RNA_SHORTCUT_MAX_PATH_LEN, RNA_ABI_VERSION,
         (int)RNA_K_COUNT);''')
    S, D = capi.ShortcutResult, capi.SHORTCUT_RESULT_DTYPE
    names = ("status", "n_waypoints", "blocked_steps", "longest_span")
    assert got[0] == C.sizeof(S) == D.itemsize == 16
    assert got[1:5] == [getattr(S, f).offset for f in names] == [D.fields[f][1] for f in names] == [0, 4, 8, 12]
    assert D.names == names and all(D.fields[f][0] == np.dtype("<i4") for f in names)
    assert got[5] == capi.SHORTCUT_KEEP_CLEARANCE == 1 and got[6] == capi.SHORTCUT_MAX_PATH_LEN
    assert got[6] * 4 <= 160 * 1024                                              # a staged path fits one compute unit's LDS
    assert got[7] == 6 == capi.ABI_VERSION == capi.lib().rna_abi_version()      # entry points were added, nothing changed
    assert got[8] == len(capi.KERNELS) == 12 and capi.KERNELS[-1] == "footprint"      # no new profile slot


def test_line_cells_index_equals_the_oracle_on_every_pair_of_a_13_box(capi):
    """every ordered pair of cells of a 13 x 13 box: all octants, D / 2 odd and even, A == D, D == 0"""
    L = capi.lib()
    buf = np.zeros(2 * 13, np.int32)
    p = buf.ctypes.data_as(C.POINTER(C.c_int32))
    cells = [(i, j) for i in range(13) for j in range(13)]
    pairs = 0
    for a in cells:
        sa = (C.c_int32 * 2)(*a)
        for b in cells:
            n = L.rna_line_cells_index(sa, (C.c_int32 * 2)(*b), p, 13)
            want = O.line_cells_index(a, b)
            assert n == len(want) and np.array_equal(buf[:2 * n].reshape(-1, 2), want), (a, b)
            d = np.abs(np.diff(want, axis=0))
            assert (d.max(axis=1) == 1).all() if n > 1 else n == 1                # consecutive cells are king moves
            pairs += 1
    assert pairs == 169 * 169


def test_line_cells_index_equals_the_oracle_on_random_long_lines(capi):
    rng = np.random.default_rng(11)
    for _ in range(300):
        a = tuple(int(v) for v in rng.integers(0, 4096, 2))
        b = tuple(int(v) for v in rng.integers(0, 4096, 2))
        assert np.array_equal(capi.line_cells_index(a, b), O.line_cells_index(a, b)), (a, b)
    for a, b in (((-7, 3), (5, -9)), ((0, 0), (70000, 69999)), ((100000, 5), (3, 70001)), ((4095, 0), (0, 4095))):
        assert np.array_equal(capi.line_cells_index(a, b), O.line_cells_index(a, b)), (a, b)     # negative and beyond-16-bit coordinates
    # only the first cap cells are written, the length is returned all the same
    buf = np.full(8, -1, np.int32)
    n = capi.lib().rna_line_cells_index((C.c_int32 * 2)(0, 0), (C.c_int32 * 2)(9, 4), buf.ctypes.data_as(C.POINTER(C.c_int32)), 3)
    assert n == 10 and np.array_equal(buf[:6].reshape(-1, 2), O.line_cells_index((0, 0), (9, 4))[:3]) and (buf[6:] == -1).all()


def test_argument_checks_that_need_no_device(capi):
    L = capi.lib()
    fake = C.c_void_p(1)     # never dereferenced: the argument checks come first
    paths = np.zeros(8, np.int32)
    res = np.zeros(1, capi.ASTAR_RESULT_DTYPE)
    wp = np.zeros(8, np.int32)
    out = np.zeros(1, capi.SHORTCUT_RESULT_DTYPE)
    P, R, W, Out = (a.ctypes.data_as(C.c_void_p) for a in (paths, res, wp, out))
    for fn in (L.rna_shortcut_paths, L.rna_shortcut_paths_device):
        assert fn(None, P, R, 1, 8, 0, 0, W, 8, Out) == RNA_EINVAL
        assert fn(fake, P, R, -1, 8, 0, 0, W, 8, Out) == RNA_EINVAL            # n < 0
        assert fn(fake, P, R, 1, 0, 0, 0, W, 8, Out) == RNA_EINVAL             # max_path_len < 1
        assert fn(fake, P, R, 1, 8, 0, 0, W, 1, Out) == RNA_EINVAL             # max_waypoints < 2
        assert fn(fake, P, R, 1, 8, -1, 0, W, 8, Out) == RNA_EINVAL            # max_span < 0
        assert fn(fake, P, R, 1, 8, 1, 0, W, 8, Out) == RNA_EINVAL             # max_span == 1: the identity, refused
        assert fn(fake, P, R, 1, 8, 0, 2, W, 8, Out) == RNA_EINVAL             # unknown flag bits
        assert fn(fake, P, R, 1, 8, 0, 0x80000001, W, 8, Out) == RNA_EINVAL
        for bad in range(4):
            a = [P, R, W, Out]
            a[bad] = None
            assert fn(fake, a[0], a[1], 1, 8, 0, 0, a[2], 8, a[3]) == RNA_EINVAL   # a NULL buffer with n > 0
    s, e = (C.c_int32 * 2)(0, 0), (C.c_int32 * 2)(3, 3)
    buf = (C.c_int32 * 16)()
    assert L.rna_line_cells_index(None, e, buf, 8) == RNA_EINVAL and L.rna_line_cells_index(s, None, buf, 8) == RNA_EINVAL
    assert L.rna_line_cells_index(s, e, None, 8) == RNA_EINVAL and L.rna_line_cells_index(s, e, buf, -1) == RNA_EINVAL
    assert L.rna_line_cells_index(s, e, None, 0) == 4                           # length only
    assert L.rna_line_cells_index(s, (C.c_int32 * 2)(1 << 30, 0), buf, 8) == RNA_EINVAL
    assert L.rna_line_cells_index((C.c_int32 * 2)(0, -(1 << 30)), e, buf, 8) == RNA_EINVAL


@needs_hipcc
def test_kernel_budget():
    """shortcut.hip cross-compiles for gfx950; both instantiations of the kernel (with and without the clearance test) use no
    scratch, declare no static LDS (the staged path is the launch's dynamic LDS, 4 B per cell) and stay at or below 64 VGPRs
    (one wavefront per path: register pressure is not what limits it, spills would be)."""
    res = resources("shortcut.hip")
    kernels = {k: v for k, v in res.items() if "shortcut_kernel" in k}
    assert len(kernels) == 2 and len(res) == 2, list(res)
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0 and v["LDS"] == 0 and v["VGPRs"] <= 64, (k, v)


def test_sources_are_in_both_build_files():
    sources_in_build_files("shortcut")


def test_cpp_additions_compile_and_link(capi, tmp_path):
    """shortcutPlan, setShortcut on both grid planners and LineIterator's (map, Index, Index) constructor, against
    move_control_amd.hpp (C++11, as the host-mirror test compiles it) and against the reference-signature header"""
    src = tmp_path / "shortcut_host.cpp"
    src.write_text(r'''
#include "move_control_amd.hpp"
int main(int argc, char**) {
  if (argc > 5) {   // compiled and linked, not run: constructing a GridMap needs a device
    grid_map::GridMap map;
    map.setGeometry(grid_map::Length(4.8, 4.0), 0.05);
    grid_map::Position goal(1.0, 1.0), start(-1.0, -0.5);
    std::vector<grid_map::Position> path, plan;
    move_control::GridAStarPlanner planner(map);
    planner.setShortcut(64, false);
    bool ok = planner.makePlan(start, goal, path);
    planner.setShortcut(0, false, false);
    ok = planner.makePlan(start, goal, plan) && ok;
    int blocked = 0;
    ok = move_control::shortcutPlan(map, plan) && move_control::shortcutPlan(map, plan, 17, true, &blocked) && ok;
    move_control::GridGoalField field(map, goal);
    field.setShortcut();
    ok = field.makePlan(start, path) && ok;
    size_t n = 0;
    for (grid_map::LineIterator it(map, grid_map::Index(0, 0), grid_map::Index(7, 3)); !it.isPastEnd(); ++it) n += (*it)[0];
    return ok && n ? 0 : 1;
  }
  return 0;
}
''')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + HOST, str(src), "-o", str(tmp_path / "shortcut_host"), "-L" + LIB_DIR,
                           "-lrna", "-Wl,-rpath," + LIB_DIR, "-lpthread"])
    api = tmp_path / "shortcut_api.cpp"
    api.write_text(r'''
#include "move_control_api.hpp"
bool f(grid_map::GridMap& map, std::vector<grid_map::Position>& plan) { return move_control::shortcutPlan(map, plan, 32); }
''')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-fsyntax-only", "-I" + HOST, str(api)])
