"""C++ host mirror (reference class names over the C ABI): compiles everywhere, runs on the GPU box."""
import os
import subprocess
import uuid

import numpy as np
import pytest

import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_mirror_compiles_against_the_c_abi():
    assert os.path.exists(_build.cpp("host_mirror_test"))


def test_node_main_with_the_reference_signatures_compiles():
    """nav_graph_node.cpp's members, constructor initialiser list and goalCb, verbatim, against move_control_api.hpp"""
    assert os.path.exists(_build.cpp("nav_graph_node_shaped"))


def test_nav_node_main_with_the_reference_signatures_compiles():
    """nav_node.cpp's members, constructor and makePlan / taileredPlan / ifGoalAchieved (the RRT flow), against move_control_api.hpp"""
    assert os.path.exists(_build.cpp("nav_node_shaped"))


def test_ros_seams_rate_keeping_without_ros():
    """ros/rate_loop.hpp -- what ros/ros_seams.cpp runs the reference's three loops on -- with a simulated clock: 5 / 2 / 5 Hz
    kept the way ros::Rate keeps them, overruns counted, latest-message cache, 0.2 s scan rate limit"""
    out = subprocess.run([_build.cpp("rate_loop_test")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "rate loop ok" in out.stdout, out.stdout + out.stderr


def test_ros_sources_compile_against_api_shaped_ros_headers():
    """This image has no ROS, so ros/*.cpp would never meet a compiler: tests/cpp/ros_stub/ holds declarations shaped like
    the roscpp / tf / message headers they use (nothing else), and g++ -fsyntax-only type-checks the seams against them AND
    against move_control_api.hpp -- that is how the clash between the generated `move_control::Histogram` message and the
    API's own struct of that name was found.  (The node mains are move_control's own, see the next test.)"""
    stub = os.path.join(ROOT, "tests", "cpp", "ros_stub")
    for src in ("ros_seams.cpp",):
        out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + stub, "-I" + os.path.join(ROOT, "include"),
                              "-I" + os.path.join(ROOT, "ros_navigation_amd", "host"), "-I" + os.path.join(ROOT, "ros"),
                              os.path.join(ROOT, "ros", src)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (src, out.stderr[-3000:])


def test_ros_sources_are_guarded_and_name_the_reference_topics():
    """The ROS nodes cannot be built here (no ROS in this image): what can be checked is that every ROS source compiles to
    nothing without <ros/ros.h> (seams), that topics, frames and rates are the reference's, and that the catkin branch builds
    move_control's own node mains (no copies of them live in this repository)."""
    ros_dir = os.path.join(ROOT, "ros")
    seams = open(os.path.join(ros_dir, "ros_seams.cpp")).read()
    for topic in ("/left_range", "/right_range", "/front_left_range", "/front_right_range", "/front_range", "/laser_scan", "/odom",
                  "global_map", "local_map", "/mobile_base/commands/velocity", '"hist"', '"odom"', '"base_link"'):
        assert topic in seams, topic
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "ros_navigation_amd", "host"), os.path.join(ros_dir, "ros_seams.cpp")])
    assert not [f for f in os.listdir(ros_dir) if f.startswith("nav_")]
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    for name in ("mapTest_graph", "mapTest_vfh", "OUTPUT_NAME mapTest)", "ros/ros_seams.cpp", "RNA_ROS_AUTOWIRE", "${MOVE_CONTROL_SOURCE_DIR}/src/${node}.cpp"):
        assert name in cm, name


@pytest.mark.gpu
def test_nav_node_rrt_flow_through_the_reference_signatures_on_gpu():
    """mapTest's planning flow (10 m window -> RrtPlanner -> taileredPlan -> Steerer) on the default 600 x 600 map, against the oracle"""
    out = subprocess.run([_build.cpp("nav_node_shaped")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "nav_node-shaped main OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_config1_moving_map_loop_through_the_reference_signatures_on_gpu():
    """BASELINE config 1 as shipped: 80 x 80 map following the robot, update / move / VFH+ loop, against the oracle"""
    out = subprocess.run([_build.cpp("nav_graph_node_shaped")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "nav_graph_node-shaped main OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_host_mirror_matches_oracle_on_gpu():
    out = subprocess.run([_build.cpp("host_mirror_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "host mirror OK" in out.stdout, out.stdout + out.stderr


def test_rccl_tiled_host_compiles_against_rocm_rccl():
    """include/rna_rccl.h + csrc/rccl_tiled.hip (ncclSend / ncclRecv / ncclAllGather on the pack / unpack buffers) and
    the C++ host example build against ROCm's rccl headers; the exchange semantics are proven by the gloo tests of
    ros_navigation_amd/dist.py, which packs and unpacks through the same C ABI."""
    assert os.path.exists(_build.cpp("tiled_host"))


def test_tiled_host_refuses_a_multi_rank_job_without_a_session_token(tmp_path):
    """round 4's advisor finding: the default token (parent pid, parent start time) is the same for two jobs that one
    long-lived launcher starts one after the other -- a rank > 0 could accept the earlier job's ncclUniqueId and hang in
    ncclCommInitRank.  A job of more than one rank therefore has to name its session; checked before any HIP call."""
    exe = _build.cpp("tiled_host")
    env = {k: v for k, v in os.environ.items() if k != "RNA_TILED_SESSION"}
    out = subprocess.run([exe, "1", "2", str(tmp_path / "id")], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 2 and "session token" in out.stderr, out.stderr[-500:]


def test_cmake_configures_the_targets():
    import shutil
    import tempfile
    if shutil.which("cmake") is None:
        pytest.skip("cmake not installed")
    d = tempfile.mkdtemp(prefix="rna_cmake_")
    try:
        subprocess.check_call(["cmake", "-S", ROOT, "-B", d], stdout=subprocess.DEVNULL)
        out = subprocess.check_output(["cmake", "--build", d, "--target", "help"], text=True)
        for t in ("rna_build", "mapTest_graph_amd", "tiled_host_build"):
            assert t in out, out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def read_tiled_dump(path):
    """records of examples/tiled_host.cpp's RNA_TILED_DUMP file: (tag, round, bytes)"""
    recs = []
    with open(path, "rb") as f:
        while True:
            head = f.read(16)
            if len(head) < 16:
                break
            tag, rnd = np.frombuffer(head[:8], "<i4")
            n = int(np.frombuffer(head[8:], "<i8")[0])
            recs.append((int(tag), int(rnd), f.read(n)))
    return recs


def test_tiled_host_id_file_bootstrap_ignores_a_stale_file():
    """examples/id_bootstrap.hpp on the CPU: a file left by an earlier job (another session token) is never taken for
    this job's -- round 3's rank > 0 read whatever /tmp/rna_nccl_id held --, a reader times out rather than accept it,
    takes the right one the moment rank 0 publishes it, and never sees half a file."""
    out = subprocess.run([_build.cpp("id_bootstrap_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "id bootstrap ok" in out.stdout, out.stdout + out.stderr


def test_gridmath_fast_index_pair_equals_wrap_index():
    """csrc/gridmath.hpp on the host alone: map_to_buffer / buffer_to_map (one add, one compare, one conditional subtract) equal
    wrap_index(x + s, n) and its inverse for every start and index of n in {1, 2, 63, 64, 65, 130}; buffer_lin / map_cell_of the
    same on 130 x 70 for every start from {0, 1, 63, 64, 65, size - 1} per axis, against buffer_index / unwrap_index"""
    out = subprocess.run([_build.cpp("gridmath_index_test")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "gridmath index ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_rccl_tiled_host_runs_as_a_single_rank_and_matches_the_oracle(tmp_path):
    """one rank = one GPU: ncclCommInitRank with world 1, every exchange a no-op, the rest of the loop for real -- and
    every output of it (laser / master layers, VFH+ commands and histograms of both rounds, A* statuses, costs and
    paths) against the oracle, from the inputs the program dumped.  The program names its phase on stderr and its own
    watchdog ends it after 60 s without progress (exit 3; 300 s while the HIP / RCCL runtimes start up, which on a box
    whose image was just pulled means paging in librccl.so's 570 MB): a hang fails this test and says where."""
    import _oracle as O
    exe = _build.cpp("tiled_host")
    dump = str(tmp_path / "tiled.dump")
    n, rounds = 1024, 2
    out = subprocess.run([exe, "0", "1", str(tmp_path / "nccl_id"), str(n), str(rounds), uuid.uuid4().hex], capture_output=True, text=True,
                         timeout=500, env=dict(os.environ, RNA_TILED_DUMP=dump))
    assert out.returncode == 0 and "tiled_host rank 0/1 OK" in out.stdout, out.stdout + out.stderr[-3000:]
    from ros_navigation_amd import capi
    recs = read_tiled_dump(dump)
    head = np.frombuffer(recs[0][2], "<i4")
    assert recs[0][0] == 0 and list(head[:8]) == [n, rounds, 0, 1, 0, n, 0, n]
    by = {}
    for tag, rnd, data in recs[1:]:
        by.setdefault((tag, rnd), []).append(data)
    g = O.make_geom(n * 0.05, n * 0.05, 0.05)
    laser = np.zeros(n * n, np.float32)
    oracles = None
    gw = np.empty(n * n, np.int32)
    found = 0
    for r in range(rounds):
        rays = np.frombuffer(by[(1, r)][0], capi.RAY_DTYPE)
        assert len(rays) == 20000
        O.himm_update(g, laser, rays.view(O.RAY_DTYPE))
        poses = np.frombuffer(by[(2, r)][0], capi.POSE_DTYPE)
        vout = np.frombuffer(by[(3, r)][0], capi.VFH_OUT_DTYPE)
        origin = np.frombuffer(by[(4, r)][0], "<f4").reshape(len(poses), 72)
        hist = np.frombuffer(by[(5, r)][0], "<f4").reshape(len(poses), 72)
        if oracles is None:
            oracles = [O.OracleVfh() for _ in range(len(poses))]
        for k, p in enumerate(poses):
            cs, ct = oracles[k].step_pose(g, laser, p["x"], p["y"], p["yaw"], int(p["current_speed"]), p["goal_direction"],
                                          p["goal_distance"], p["goal_tolerance"], float(p["dt"]))
            assert (vout["chosen_speed"][k], vout["chosen_turnrate"][k]) == (cs, ct), (r, k)
            assert origin[k].tobytes() == oracles[k].origin_hist().tobytes() and hist[k].tobytes() == oracles[k].hist().tobytes(), (r, k)
        queries = np.frombuffer(by[(6, r)][0], capi.ASTAR_QUERY_DTYPE)
        results = np.frombuffer(by[(7, r)][0], capi.ASTAR_RESULT_DTYPE)
        assert len(queries) == 32 and len(by[(8, r)]) == 32
        _, nbr = O.astar_masks(laser, n, n)
        for k, q in enumerate(queries):
            ores, opath, _ = O.astar_query(nbr, n, n, q["start"], q["goal"], g_work=gw)
            assert results["status"][k] == ores.status, (r, k)
            if ores.status == 0:
                path = np.frombuffer(by[(8, r)][k], "<i4")
                assert results["cost"][k] == ores.cost and np.array_equal(path, opath), (r, k)
                found += 1
    assert found > 0 and ("%d paths" % found) in out.stdout
    for tag in (9, 10):     # the final laser and master layers
        got = np.frombuffer(by[(tag, rounds)][0], "<f4")
        assert np.array_equal(np.isnan(got), np.isnan(laser)) and np.array_equal(got[~np.isnan(got)], laser[~np.isnan(laser)]), tag
