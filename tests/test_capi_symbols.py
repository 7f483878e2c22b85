"""CPU-only: librna.so loads and exports every symbol include/rna.h declares; struct layouts of the
ctypes binding match the header; the product refuses to run without a device instead of falling back."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _build import capi  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "rna.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rna_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(capi):
    L = capi.lib()
    syms = header_symbols()
    assert len(syms) >= 35
    for s in syms:
        assert hasattr(L, s), "librna.so does not export %s" % s
    assert sorted(capi.SYMBOLS) == syms
    assert L.rna_abi_version() == capi.ABI_VERSION == int(re.search(r"#define RNA_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "rna.h")).read()).group(1))


def test_struct_layouts_match_header(capi, tmp_path):
    src = open(os.path.join(ROOT, "include", "rna.h")).read()
    prog = r"""
    #include <stdio.h>
    #include "rna.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu ", sizeof(rna_geometry), sizeof(rna_ray), sizeof(rna_vfh_params),
             sizeof(rna_pose), sizeof(rna_vfh_out), sizeof(rna_astar_query), sizeof(rna_astar_result),
             sizeof(rna_rrt_query), sizeof(rna_rrt_result), (size_t)RNA_K_COUNT, sizeof(rna_laser_scan));
      printf("%zu %zu %zu %zu\n", sizeof(rna_submap_info), sizeof(rna_range_reading), sizeof(rna_laser_scan_tf), sizeof(rna_range_reading_tf));
      return 0;
    }"""
    exe = str(tmp_path / "rna_layout_check")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=prog.encode(), check=True)
    sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [C.sizeof(capi.Geometry), capi.RAY_DTYPE.itemsize, C.sizeof(capi.VfhParams),
                     capi.POSE_DTYPE.itemsize, capi.VFH_OUT_DTYPE.itemsize, capi.ASTAR_QUERY_DTYPE.itemsize,
                     capi.ASTAR_RESULT_DTYPE.itemsize, capi.RRT_QUERY_DTYPE.itemsize, capi.RRT_RESULT_DTYPE.itemsize,
                     len(capi.KERNELS), capi.SCAN_DTYPE.itemsize, C.sizeof(capi.SubmapInfo), capi.RANGE_READING_DTYPE.itemsize,
                     capi.SCAN_TF_DTYPE.itemsize, capi.RANGE_READING_TF_DTYPE.itemsize]
    assert src.count("extern \"C\"") == 1


def test_no_device_means_error_not_fallback(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    rc = capi.lib().rna_create(C.byref(h), 1.0, 1.0, 0.05, 0.0, 0.0, 0)
    assert rc == -6 and not h.value  # RNA_ENODEVICE
    with pytest.raises(capi.RnaError):
        capi.Engine(1.0, 1.0, 0.05)


def test_tailor_plan_host_entry_point(capi):
    """rna_tailor_plan (Nav::taileredPlan, mc/src/nav_node.cpp:192-204) is host-only: checked here against the oracle"""
    import numpy as np
    import _oracle as O
    rng = np.random.default_rng(0)
    for n in (0, 1, 2, 5, 6, 11, 57):
        plan = rng.normal(size=(n, 2))
        for stride in (1, 2, 5):
            assert np.array_equal(capi.tailor_plan(plan, stride), O.tailor_plan(plan, stride))


def test_follow_plan_host_entry_point(capi):
    """rna_follow_plan (Steerer::acceptPlan + head of Steerer::update, mc/src/steerer.cpp:27-33,222-256) is host-only:
    hand-checked cases, then random plans / robot tracks against the oracle, bit for bit."""
    import numpy as np
    import _oracle as O
    plan = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 2.0], [1.1, 2.0]])
    # robot at the origin looking along +x: way point 1 is 1000 mm straight ahead = 90 deg
    ok, idx, pose = capi.follow_plan(plan, 1, 0.0, 0.0, 0.0, linear_velocity=0.3456, dt=0.25)
    assert ok and idx == 1 and pose["goal_distance"] == np.float32(1000.0) and pose["goal_direction"] == np.float32(90.0)
    assert pose["current_speed"] == 345 and pose["goal_tolerance"] == 250.0 and pose["dt"] == 0.25
    # within 250 mm of way point 1: skipped; way point 2 is up-left of a robot looking along +x
    ok, idx, pose = capi.follow_plan(plan, 1, 0.9, 0.1, 0.0)
    assert ok and idx == 2 and abs(float(pose["goal_direction"]) - (90.0 + np.degrees(np.arctan2(1.9, 0.1)))) < 1e-4
    # last two way points both within tolerance: the plan is finished, index runs past the end
    ok, idx, _ = capi.follow_plan(plan, 2, 1.05, 2.05, 1.0)
    assert (ok, idx) == (False, 4)
    for short in (plan[:0], plan[:1]):                       # the reference would read plan_[1] out of bounds
        assert capi.follow_plan(short, 1, 0.0, 0.0, 0.0)[0] is False
    with pytest.raises(capi.RnaError):
        capi.follow_plan(plan, -1, 0.0, 0.0, 0.0)
    rng = np.random.default_rng(3)
    for _ in range(300):
        n = int(rng.integers(2, 40))
        plan = np.cumsum(rng.normal(scale=0.2, size=(n, 2)), 0)
        idx_c = idx_o = 1
        pos = plan[0] + rng.normal(scale=0.05, size=2)
        for step in range(60):
            yaw = float(rng.uniform(-7, 7))
            ok, idx_c, pose = capi.follow_plan(plan, idx_c, pos[0], pos[1], yaw, float(rng.uniform(-0.2, 0.7)))
            ook, idx_o, ang, dist = O.follow_plan(plan, idx_o, pos[0], pos[1], yaw)
            assert (ok, idx_c) == (ook, idx_o)
            if not ok:
                break
            assert np.float32(pose["goal_direction"]).tobytes() == ang.tobytes()
            assert np.float32(pose["goal_distance"]).tobytes() == dist.tobytes()
            assert 0.0 <= pose["goal_direction"] <= 360.0 and pose["goal_distance"] >= 250.0
            pos = pos + 0.6 * (plan[idx_c] - pos) + rng.normal(scale=0.02, size=2)   # the robot moves towards it


def test_range_to_rays_host_entry_point(capi):
    """rna_range_to_rays (RangeMapUpdater::bufferIncomingMsg, mc/src/range_map_updater.cpp:38-76), host-only."""
    import numpy as np
    import _oracle as O
    m = np.zeros(4, capi.RANGE_READING_DTYPE)
    m[0] = (2.0, 4.0, 1.0, -1.0, 0.0)                 # looking along +x: hit 2 m ahead
    m[1] = (4.0, 4.0, 0.0, 0.0, np.pi / 2)            # range == max_range: nothing seen, clear the end cell too
    m[2] = (np.inf, 4.0, 0.5, 0.5, 1.0)
    m[3] = (np.nan, 4.0, 0.5, 0.5, 1.0)               # NaN < max is false -> ifClearEnd
    r = capi.range_to_rays(m)
    assert (r["sx"][0], r["sy"][0], r["ex"][0], r["ey"][0], r["clear_end"][0]) == (1.0, -1.0, 3.0, -1.0, 0)
    assert r["clear_end"].tolist() == [0, 1, 1, 1] and abs(r["ey"][1] - 4.0) < 1e-15 and abs(r["ex"][1]) < 1e-15
    rng = np.random.default_rng(5)
    m = np.zeros(5000, capi.RANGE_READING_DTYPE)
    m["range"] = rng.uniform(0.0, 5.0, len(m))
    m["max_range"] = rng.choice([3.0, 4.0], len(m))
    m["x"], m["y"], m["yaw"] = rng.uniform(-20, 20, len(m)), rng.uniform(-20, 20, len(m)), rng.uniform(-7, 7, len(m))
    assert capi.range_to_rays(m).tobytes() == O.range_to_rays(m).tobytes()
    assert len(capi.range_to_rays(m[:0])) == 0
    # the same sensors with their full pose: a mount pitched down by 30 degrees sees its 2 m reading 1.73 m ahead on the map
    from scipy.spatial.transform import Rotation
    t = np.zeros(3, capi.RANGE_READING_TF_DTYPE)
    t[0] = (2.0, 4.0, (1.0, -1.0, 0.4), Rotation.from_euler("y", 30, degrees=True).as_quat())
    t[1] = (4.0, 4.0, (0.0, 0.0, 0.2), Rotation.from_euler("z", 90, degrees=True).as_quat())
    t[2] = (1.0, 4.0, (0.5, 0.5, 0.0), Rotation.from_euler("zyx", [40, 10, -5], degrees=True).as_quat())
    r = capi.range_to_rays_tf(t)
    assert (r["sx"][0], r["sy"][0]) == (1.0, -1.0) and abs(r["ex"][0] - (1.0 + 2.0 * np.cos(np.pi / 6))) < 1e-12 and abs(r["ey"][0] + 1.0) < 1e-12
    assert r["clear_end"].tolist() == [0, 1, 0] and abs(r["ey"][1] - 4.0) < 1e-12 and abs(r["ex"][1]) < 1e-12
    want = Rotation.from_quat(t["q"][2]).apply([1.0, 0.0, 0.0])[:2] + 0.5
    assert np.allclose([r["ex"][2], r["ey"][2]], want, rtol=0, atol=1e-12)
    t = np.zeros(3000, capi.RANGE_READING_TF_DTYPE)
    t["range"], t["max_range"] = rng.uniform(0.0, 5.0, len(t)), rng.choice([3.0, 4.0], len(t))
    t["t"] = rng.uniform(-20, 20, (len(t), 3))
    t["q"] = Rotation.random(len(t), random_state=6).as_quat()
    assert capi.range_to_rays_tf(t).tobytes() == O.range_to_rays_tf(t).tobytes()


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "ros_navigation_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "rna_oracle" not in txt and "_oracle" not in txt and "librna_oracle" not in txt, f


def test_hw_queue_advice_text_and_the_load_time_default(capi):
    """Library-side guard for the hardware queues of a pipelined engine: librna.so sets GPU_MAX_HW_QUEUES=8 when it is
    loaded with the variable unset (in time for any host that loads it before touching the GPU), leaves a host's own
    value alone, and rna_hw_queue_advice says in one line when the value in force is too small for a pipeline depth --
    the text rna_astar_set_pipeline_depth leaves in rna_last_error.  The advice speaks of the value the library FOUND WHEN IT
    WAS LOADED (what the HIP runtime latches at its first call), not of what the environment reads at the time of the call
    (round 4's advisor finding), and it says so when the process had opened the GPU before the library set the variable."""
    import sys
    base = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "RNA_KEEP_HW_QUEUES")}

    def advice(depth, env, cap=400, pre=""):
        prog = ("import ctypes, os\n%s\nL = ctypes.CDLL(%r)\nos.environ['GPU_MAX_HW_QUEUES'] = '1'\n"     # (a later change of the environment must not matter)
                "buf = ctypes.create_string_buffer(400)\nL.rna_hw_queue_advice.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]\n"
                "rc = L.rna_hw_queue_advice(%d, buf if %d else None, %d)\nprint(rc); print(buf.value.decode())" % (pre, capi.LIB_PATH, depth, cap, cap))
        out = subprocess.check_output([sys.executable, "-c", prog], env=env, text=True).split("\n")
        return int(out[0]), out[1]

    assert advice(13, dict(base, GPU_MAX_HW_QUEUES="8")) == (0, "")
    assert advice(13, base) == (0, "")                                   # unset: the library set 8 itself, nobody had opened the GPU
    rc, text = advice(13, dict(base, GPU_MAX_HW_QUEUES="4"))
    assert rc == 1 and "depth 13" in text and "GPU_MAX_HW_QUEUES >= 8" in text and "it was 4" in text and "before the first HIP call" in text
    assert advice(2, dict(base, GPU_MAX_HW_QUEUES="4")) == (0, "")      # two stages fit the default four queues
    rc, text = advice(4, dict(base, RNA_KEEP_HW_QUEUES="1"))
    assert rc == 1 and "unset" in text
    assert advice(4, dict(base, RNA_KEEP_HW_QUEUES="1"), cap=0)[0] == 1      # no buffer: just the answer
    rc, text = advice(4, dict(base, RNA_KEEP_HW_QUEUES="1"), cap=8)
    assert rc == 1 and len(text) <= 7                                          # truncated, terminated
    if os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK | os.W_OK):
        # the process has the GPU open before the library is loaded: the library's own setting may have come too late
        rc, text = advice(13, base, pre="fd = os.open('/dev/kfd', os.O_RDWR)")
        assert rc == 2 and "had opened the GPU before" in text and "\n" not in text
        assert advice(13, dict(base, GPU_MAX_HW_QUEUES="8"), pre="fd = os.open('/dev/kfd', os.O_RDWR)") == (0, "")   # the host's own setting: fine
    prog = ("import ctypes, sys; ctypes.CDLL(%r); g = ctypes.CDLL(None).getenv; g.restype = ctypes.c_char_p; "
            "print(g(b'GPU_MAX_HW_QUEUES'))" % capi.LIB_PATH)
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "RNA_KEEP_HW_QUEUES")}
    assert subprocess.check_output([sys.executable, "-c", prog], env=env, text=True).strip() == "b'8'"
    assert subprocess.check_output([sys.executable, "-c", prog], env=dict(env, GPU_MAX_HW_QUEUES="5"), text=True).strip() == "b'5'"
    assert subprocess.check_output([sys.executable, "-c", prog], env=dict(env, RNA_KEEP_HW_QUEUES="1"), text=True).strip() == "None"
