"""CPU-only checks of scan matching (rna_scan_match / rna_scan_match_device, csrc/scanmatch.hip, and the two host helpers
rna_scan_match_prepare / rna_scan_match_pose): the entry points are exported and bound, the record and the query have the
header's layout, the five constants, the ABI version and the profile slots did not move, argument checks that need no device,
the kernels' resource budget on gfx950, the C++ additions compile and link, and the helpers' arithmetic."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from _build import (HOST, INCLUDE, LIB_DIR, c_values, capi, needs_hipcc, resources,  # noqa: F401  (capi: the fixture)
                    sources_in_build_files)

NEW = ["rna_scan_match", "rna_scan_match_device", "rna_scan_match_prepare", "rna_scan_match_pose"]
RNA_EINVAL, RNA_ECAPACITY = -1, -4
REC = ("status", "score", "rot", "shift", "n_used", "score_guess", "score_max")
QRY = ("cell", "sub", "points_offset", "n_points")


def test_new_symbols_are_exported_and_bound(capi):
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes, "%s has no ctypes signature" % s
    for m in ("scan_match", "scan_match_device", "scan_match_poses"):
        assert callable(getattr(capi.Engine, m))
    assert callable(capi.scan_match_prepare) and callable(capi.scan_match_pose)


def test_struct_layouts_constants_abi_version_and_profile_slots(capi, tmp_path):
    got = c_values(tmp_path,
                   '  printf("%zu %zu %d %d %d %d %d %d %d\\n", sizeof(struct rna_scan_match), sizeof(rna_scan_match_query),'
                   ' RNA_SCAN_MATCH_MAX_RANGE, RNA_SCAN_MATCH_MAX_SHIFT, RNA_SCAN_MATCH_MAX_LEVELS, RNA_SCAN_MATCH_MAX_ROT,'
                   ' RNA_SCAN_MATCH_MAX_POINTS, RNA_ABI_VERSION, (int)RNA_K_COUNT);\n'
                   + "".join('  printf("%%zu ", offsetof(struct rna_scan_match, %s));\n' % f for f in REC)
                   + "".join('  printf("%%zu ", offsetof(rna_scan_match_query, %s));\n' % f for f in QRY))
    M, Q, DM, DQ = capi.ScanMatch, capi.ScanMatchQuery, capi.SCAN_MATCH_DTYPE, capi.SCAN_MATCH_QUERY_DTYPE
    assert got[0] == C.sizeof(M) == DM.itemsize == 32
    assert got[1] == C.sizeof(Q) == DQ.itemsize == 20
    assert got[2:7] == [capi.SCAN_MATCH_MAX_RANGE, capi.SCAN_MATCH_MAX_SHIFT, capi.SCAN_MATCH_MAX_LEVELS, capi.SCAN_MATCH_MAX_ROT,
                        capi.SCAN_MATCH_MAX_POINTS] == [127, 16, 4, 128, 8192]
    assert got[7] == 6 == capi.ABI_VERSION == capi.lib().rna_abi_version()      # entry points were added, nothing changed
    assert got[8] == len(capi.KERNELS) == 12 and capi.KERNELS[-1] == "footprint"      # no new profile slot
    assert got[9:16] == [getattr(M, f).offset for f in REC] == [DM.fields[f][1] for f in REC] == [0, 4, 8, 12, 20, 24, 28]
    assert got[16:20] == [getattr(Q, f).offset for f in QRY] == [DQ.fields[f][1] for f in QRY] == [0, 4, 12, 16]
    assert DM.names == REC and DQ.names == QRY
    assert all(DM.fields[f][0].base == np.dtype("<i4") for f in REC) and all(DQ.fields[f][0].base == np.dtype("<i4") for f in QRY)
    assert DM.fields["shift"][0].shape == (2,) and DQ.fields["sub"][0].shape == (2,)
    assert open(os.path.join(INCLUDE, "rna.h")).read().count('extern "C"') == 1


def test_argument_checks_that_need_no_device(capi):
    L = capi.lib()
    fake = C.c_void_p(1)     # never dereferenced: the argument checks come first
    qs = np.zeros(2, capi.SCAN_MATCH_QUERY_DTYPE)
    qs["n_points"] = [3, 1]
    qs["points_offset"] = [0, 3]
    pts = np.zeros((4, 2), np.int32)
    rot = np.zeros((2, 3, 2), np.int32)
    out = np.zeros(2, capi.SCAN_MATCH_DTYPE)
    vol = np.zeros(2 * 3 * 9, np.int32)
    out.view(np.uint8)[:] = 0xA5
    vol.view(np.uint8)[:] = 0xA5
    before = out.tobytes(), vol.tobytes()
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    Q, P, R, O, V = p(qs), p(pts), p(rot), p(out), p(vol)
    for fn in (L.rna_scan_match, L.rna_scan_match_device):
        assert fn(None, Q, 2, P, 4, R, 3, 10, 1, 2, O, V) == RNA_EINVAL            # NULL engine
        assert fn(fake, Q, -1, P, 4, R, 3, 10, 1, 2, O, V) == RNA_EINVAL           # n < 0
        assert fn(fake, Q, 2, P, 4, R, 0, 10, 1, 2, O, V) == RNA_EINVAL            # n_rot < 1
        assert fn(fake, Q, 2, P, 4, R, 3, 0, 1, 2, O, V) == RNA_EINVAL             # range_cells < 1
        assert fn(fake, Q, 2, P, 4, R, 3, 10, 1, 0, O, V) == RNA_EINVAL            # levels < 1
        assert fn(fake, Q, 2, P, 4, R, 3, 10, -1, 2, O, V) == RNA_EINVAL           # max_shift < 0
        assert fn(fake, None, 2, P, 4, R, 3, 10, 1, 2, O, V) == RNA_EINVAL         # NULL buffers with n > 0
        assert fn(fake, Q, 2, None, 4, R, 3, 10, 1, 2, O, V) == RNA_EINVAL
        assert fn(fake, Q, 2, P, 4, None, 3, 10, 1, 2, O, V) == RNA_EINVAL
        assert fn(fake, Q, 2, P, 4, R, 3, 10, 1, 2, None, V) == RNA_EINVAL
        assert fn(fake, Q, 0, P, 4, R, 3, 0, 1, 2, O, V) == RNA_EINVAL             # ... the window is checked for n == 0 too
        assert fn(fake, None, 0, None, 0, None, 3, 10, 1, 2, None, None) == 0      # n == 0 with valid arguments: nothing to do
        assert fn(fake, None, 0, None, 0, None, 128, 127, 16, 4, None, None) == 0  # ... at the caps
    # the host form reads its queries (host memory) before the engine: points that leave the array
    for field, k, bad in (("n_points", 1, 2), ("points_offset", 0, 2), ("points_offset", 1, -1), ("n_points", 0, -1), ("n_points", 0, 8193)):
        worse = qs.copy()
        worse[field][k] = bad
        assert L.rna_scan_match(fake, p(worse), 2, P, 4, R, 3, 10, 1, 2, O, V) == RNA_EINVAL, (field, k, bad)
    # the _device form keeps its keys in the records: they are 8-byte aligned
    assert L.rna_scan_match_device(fake, Q, 2, P, 4, R, 3, 10, 1, 2, C.c_void_p(out.ctypes.data + 4), V) == RNA_EINVAL
    assert (out.tobytes(), vol.tobytes()) == before
    # (RNA_ECAPACITY beyond the caps writes the engine's error text: it needs a real engine, tests/test_gpu_scan_match.py has it)


@needs_hipcc
def test_kernel_budget():
    """scanmatch.hip cross-compiles for gfx950: one score kernel per number of levels and the decode kernel, none of them
    with scratch; the score kernels hold everything in dynamic LDS (no static LDS in front of it: the base stays 16-byte
    aligned for the wide reads), and at the caps -- R = 127, T = 16, L = 4: 295 rows x 10 words x 4 interleaved bitmaps,
    2048 staged points, 16 control words -- that is 55 456 bytes, at or below 64 KiB"""
    res = resources("scanmatch.hip")
    score = {k: v for k, v in res.items() if "scan_match_kernel" in k}
    assert len(res) == 5 and len(score) == 4 and any("scan_match_decode_kernel" in k for k in res), list(res)
    R, T, L = 127, 16, 4
    W = 2 * (R + 1 + T + (L - 1)) + 1
    dynamic = (W * ((W + 31) // 32) * L + 2048 + 16) * 4
    assert W == 295 and dynamic == 55456
    for k, v in res.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDS"] == 0 and v["LDS"] + dynamic <= 64 * 1024, (k, v)


def test_sources_are_in_both_build_files():
    sources_in_build_files("scanmatch")


def test_cpp_additions_compile_and_link(capi, tmp_path):
    """move_control::ScanMatch, ScanMatchWindow and both forms of matchScan, against move_control_amd.hpp (C++11, as the
    host-mirror test compiles it) and against the reference-signature header"""
    src = tmp_path / "scan_match_host.cpp"
    src.write_text(r'''
#include "move_control_amd.hpp"
int main(int argc, char**) {
  if (argc > 5) {   // compiled and linked, not run: constructing a GridMap needs a device
    grid_map::GridMap map;
    map.setGeometry(grid_map::Length(4.8, 4.0), 0.05);
    std::vector<grid_map::Position> points(3, grid_map::Position(1.0, 0.5));
    move_control::ScanMatchWindow window = {0.005, 21, 8, 3, 6.0};
    move_control::Pose2D fixed;
    move_control::ScanMatch rec;
    bool ok = move_control::matchScan(map, points, 0.1, -0.2, 0.3, window, fixed, rec);
    std::vector<std::vector<grid_map::Position> > scans(2, points);
    std::vector<move_control::Pose2D> guesses(2), poses;
    std::vector<move_control::ScanMatch> recs;
    ok = move_control::matchScan(map, scans, guesses, window, poses, recs) && ok;
    long sum = rec.status + rec.score + rec.rot + rec.shift[0] + rec.shift[1] + rec.n_used + rec.score_guess + rec.score_max;
    struct rna_scan_match raw;
    rna_scan_match_query q = {0, {0, 0}, 0, 0};
    const int32_t rot[2] = {16384, 0};
    ok = rna_scan_match_device(map.engine(), &q, 0, 0, 0, rot, 1, 1, 0, 1, &raw, 0) == RNA_OK && ok;
    return ok && sum >= 0 && fixed.yaw == poses[0].yaw ? 0 : 1;
  }
  return 0;
}
''')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + HOST, str(src), "-o", str(tmp_path / "scan_match_host"), "-L" + LIB_DIR,
                           "-lrna", "-Wl,-rpath," + LIB_DIR, "-lpthread"])
    api = tmp_path / "scan_match_api.cpp"
    api.write_text(r'''
#include "move_control_api.hpp"
bool f(grid_map::GridMap& map, const std::vector<grid_map::Position>& points, const move_control::ScanMatchWindow& w,
       move_control::Pose2D& pose, move_control::ScanMatch& rec) {
  return move_control::matchScan(map, points, 1.0, 2.0, 0.5, w, pose, rec);
}
''')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-fsyntax-only", "-I" + HOST, str(api)])


# ---- rna_scan_match_prepare / rna_scan_match_pose ----
RES = 0.05


def _geom(capi, start=(0, 0)):
    return capi.make_geometry(96 * RES, 80 * RES, RES, position=(1.0, -2.0), start_index=start)


def test_prepare_exact_rotations_and_a_hand_computed_point(capi):
    g = _geom(capi)
    # the map's centre is (1, -2): its cells' centres lie at odd multiples of res / 2 from it.  The cell of (1.0125, -2.03):
    # index = -(int)((x - len / 2 - pos) / res) per axis = (47, 40), centre (1.025, -2.025); the sensor is 0.0125 m below the
    # centre in x = + 1/4 cell in index orientation = sub 16, and 0.005 m below it in y = 0.1 cell = lrint(6.4) = 6
    x, y = 1.0125, -2.03
    assert capi.geometry_index(g, x, y) == (47, 40)
    xy = np.array([[0.05, 0.0], [-0.1, 0.025], [0.0, -1.0], [1e12, 0.0], [np.nan, 0.0], [0.0004, -0.0004]])
    for yaw, cs in ((0.0, (16384, 0)), (math.pi / 2, (0, 16384)), (-math.pi / 2, (0, -16384)), (math.pi, (-16384, 0))):
        inside, q, q6, rot = capi.scan_match_prepare(g, xy, x, y, yaw, 0.01, 5)
        assert inside and int(q["cell"]) == 47 + 40 * 96 and q["sub"].tolist() == [16, 6]
        assert (int(q["points_offset"]), int(q["n_points"])) == (0, 6)
        assert tuple(rot[2]) == cs                                                     # r_c = 5 // 2 carries the guess's yaw
        # one metre is 20 cells = 1280 units; the sign flips; beyond 2^30 and NaN: 2^30
        assert q6.tolist() == [[-64, 0], [128, -32], [0, 1280], [1 << 30, 0], [1 << 30, 0], [-1, 1]]
    inside, q, q6, rot = capi.scan_match_prepare(g, xy, x, y, 0.0, 0.0, 4)                # an even count: r_c = 2
    assert rot.tolist() == [[16384, 0]] * 4
    # the far corner cell and a moved buffer: cell is a BUFFER index, as rna_geometry_index gives it
    gm = _geom(capi, start=(37, 58))
    for gg in (g, gm):
        for px, py in ((x, y), (1.0 + 2.39, -2.0 + 1.99), (1.0 - 2.39, -2.0 - 1.99)):
            i, j = capi.geometry_index(gg, px, py)
            inside, q, _, _ = capi.scan_match_prepare(gg, xy[:1], px, py, 0.3, 0.01, 3)
            assert inside and int(q["cell"]) == i + j * 96
            cx, cy = capi.geometry_position(gg, i, j)
            assert q["sub"].tolist() == [min(31, max(-32, round(-(px - cx) / RES * 64))), min(31, max(-32, round(-(py - cy) / RES * 64)))]
    # outside the map: 0, cell -1, points and rotations still written
    inside, q, q6, rot = capi.scan_match_prepare(g, xy, 100.0, 0.0, 0.0, 0.01, 3)
    assert not inside and int(q["cell"]) == -1 and q["sub"].tolist() == [0, 0] and q6[0].tolist() == [-64, 0] and tuple(rot[1]) == (16384, 0)
    # bad arguments
    L = capi.lib()
    one = np.zeros(1, capi.SCAN_MATCH_QUERY_DTYPE)
    buf = np.zeros(64, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.rna_scan_match_prepare(None, p(xy), 1, 0.0, 0.0, 0.0, 0.1, 3, p(one), p(buf), p(buf)) == RNA_EINVAL
    assert L.rna_scan_match_prepare(C.byref(g), p(xy), -1, 0.0, 0.0, 0.0, 0.1, 3, p(one), p(buf), p(buf)) == RNA_EINVAL
    assert L.rna_scan_match_prepare(C.byref(g), p(xy), 8193, 0.0, 0.0, 0.0, 0.1, 3, p(one), p(buf), p(buf)) == RNA_EINVAL
    assert L.rna_scan_match_prepare(C.byref(g), p(xy), 1, 0.0, 0.0, 0.0, 0.1, 0, p(one), p(buf), p(buf)) == RNA_EINVAL
    assert L.rna_scan_match_prepare(C.byref(g), p(xy), 1, 0.0, 0.0, 0.0, 0.1, 129, p(one), p(buf), p(buf)) == RNA_EINVAL
    assert L.rna_scan_match_prepare(C.byref(g), p(xy), 1, 0.0, 0.0, 0.0, 0.1, 3, None, p(buf), p(buf)) == RNA_EINVAL
    assert L.rna_scan_match_prepare(C.byref(g), None, 1, 0.0, 0.0, 0.0, 0.1, 3, p(one), p(buf), p(buf)) == RNA_EINVAL


def test_prepare_matches_numpy_within_one_unit(capi):
    """general angles and points: libm's last ulp may move an lrint across a half, so +-1 unit; never more"""
    g = _geom(capi)
    rng = np.random.default_rng(7)
    for _ in range(20):
        n, n_rot = int(rng.integers(0, 300)), int(rng.integers(1, 129))
        xy = rng.uniform(-8.0, 8.0, (n, 2))
        x, y = rng.uniform(1.0 - 2.3, 1.0 + 2.3), rng.uniform(-2.0 - 1.9, -2.0 + 1.9)
        yaw, step = rng.uniform(-4.0, 4.0), rng.uniform(0.0, 0.02)
        inside, q, q6, rot = capi.scan_match_prepare(g, xy, x, y, yaw, step, n_rot)
        assert inside and q6.shape == (n, 2) and rot.shape == (n_rot, 2)
        assert np.abs(q6 - np.rint(-xy / RES * 64)).max(initial=0) <= 1
        ang = yaw + (np.arange(n_rot) - n_rot // 2) * step
        assert np.abs(rot[:, 0] - np.rint(16384 * np.cos(ang))).max() <= 1 and np.abs(rot[:, 1] - np.rint(16384 * np.sin(ang))).max() <= 1
        i, j = capi.geometry_index(g, x, y)
        cx, cy = capi.geometry_position(g, i, j)
        want = np.clip(np.rint([-(x - cx) / RES * 64, -(y - cy) / RES * 64]), -32, 31)
        assert int(q["cell"]) == i + j * 96 and np.abs(q["sub"] - want).max() <= 1


def test_pose_of_a_record(capi):
    g = _geom(capi)
    rec = np.zeros(1, capi.SCAN_MATCH_DTYPE)[0]
    x, y, yaw, step = 0.7, -1.3, 0.25, 0.004
    for n_rot in (1, 2, 41):
        rec["rot"] = n_rot // 2
        assert capi.scan_match_pose(g, x, y, yaw, step, n_rot, rec) == (x, y, yaw)      # rot = r_c, zero shift: the guess
    rec["rot"], rec["shift"] = 20, (1, 0)
    assert capi.scan_match_pose(g, x, y, yaw, step, 41, rec) == (x - RES, y, yaw)       # shift0 = +1 lowers x by one resolution
    rec["rot"], rec["shift"] = 23, (-3, 2)
    assert capi.scan_match_pose(g, x, y, yaw, step, 41, rec) == (x + 3 * RES, y - 2 * RES, yaw + 3 * step)
    rec["rot"] = 0
    assert capi.scan_match_pose(g, x, y, yaw, step, 2, rec)[2] == yaw - step           # an even count: r_c = 1
    L = capi.lib()
    pose = (C.c_double * 3)()
    one = np.zeros(1, capi.SCAN_MATCH_DTYPE)
    assert L.rna_scan_match_pose(None, x, y, yaw, step, 3, one.ctypes.data_as(C.c_void_p), pose) == RNA_EINVAL
    assert L.rna_scan_match_pose(C.byref(g), x, y, yaw, step, 0, one.ctypes.data_as(C.c_void_p), pose) == RNA_EINVAL
    assert L.rna_scan_match_pose(C.byref(g), x, y, yaw, step, 3, None, pose) == RNA_EINVAL
