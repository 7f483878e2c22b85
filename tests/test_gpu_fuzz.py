"""Randomised parity in the driver-run suite: the time-boxed fuzzers of scripts/ (the same code the developer runs for
hours) with a FIXED seed and a short budget each, as subprocesses -- random map shapes that are not multiples of the
64 x 16 search tiles, densities 0..0.6, unknown cells, bucket widths 2828..400000, chunked batches, engine reuse, maps
moved once or twice (grid A*); random geometry / resolution / moved buffers, end points on cell centres, edges and the
map border, poses past the border, for half of the cases one of the VFH parameter sets of tests/_vfh_cases.py
(map update + VFH+); resolutions 0.025-0.2 m, origins up to 2000 m, radii of k and k + 1/2
cells, moved maps (robot radius); sequences of map operations on one engine against the model of tests/_mapmodel.py (map state);
waypoint graphs of up to 256 vertices and batches of up to 200 queries, a quarter of them held to Dijkstra as well (graph A*);
occupancy-grid conversions and LaserScan batches of unlike scans through the host and the device forms, every end point held to the
accepted-value rule of tests/_scan_reference.py (messages); RRT on maps of 4-30 m at 0.025-0.2 m, moved or not, through the host and
the device form, with max_path_len above and below the paths, bit for bit against oracle/rrt.c in the kernel's formulation (RRT).
A fuzzer exits non-zero at the first difference from the oracle
and prints the configuration that reproduces it.  The search kernel's correctness rests on an asynchronous scheduler,
`asm volatile` fences and on what the optimiser may hoist: this net catches what the hand-picked cases do not."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_fuzzer(script, seconds, seed):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), str(seconds), str(seed)], capture_output=True, text=True,
                         timeout=seconds + 240, cwd=ROOT)
    assert out.returncode == 0, (script, seed, out.stdout[-3000:], out.stderr[-2000:])
    assert "fuzz ok" in out.stdout, out.stdout[-1000:]
    return out.stdout


@pytest.mark.parametrize("seed", [301, 302])
def test_fuzz_grid_astar_fixed_seed(seed):
    text = run_fuzzer("fuzz_astar.py", 15, seed)
    maps = int(text.split("):")[1].split("maps")[0])
    assert maps >= 10, text     # the budget was spent on searches, not on start-up


def test_fuzz_map_update_and_vfh_fixed_seed():
    run_fuzzer("fuzz_himm_vfh.py", 15, 303)


def test_fuzz_footprint_fixed_seed():
    text = run_fuzzer("fuzz_footprint.py", 10, 304)
    maps = int(text.split("):")[1].split("maps")[0])
    # The per-cell oracle in Python is what a case costs.  Measured on a CPU-only machine, with the engine's answers replaced
    # by the oracle's own so that only the oracle side runs: 25 maps in 10 s with this seed (16 and 24 with seeds 1 and 2).
    # The floor is below half of that, because the GPU host's CPUs are shared.
    assert maps >= 8, text


def test_fuzz_map_sequences_fixed_seed():
    text = run_fuzzer("fuzz_map_sequences.py", 10, 306)
    sequences = int(text.split("fuzz ok:")[1].split("sequences")[0])
    # 12 sequences in 10 s with this seed on an MI355X host (DESIGN.md section 4 has the per-test times), most of it the oracles in
    # Python; the floor is far below that because the GPU host's CPUs are shared.
    assert sequences >= 2, text


def test_fuzz_graph_fixed_seed():
    text = run_fuzzer("fuzz_graph.py", 5, 307)
    graphs = int(text.split("fuzz ok:")[1].split("graphs")[0])
    # What a case costs is the oracle, and for a quarter of the graphs Dijkstra, in Python.  Measured on a CPU-only machine with
    # the engine's answers replaced by the oracle's own (so the oracle side ran twice): 1187 and 1219 graphs in 5 s with this
    # seed (1151 with seed 1), 79 000 queries.  The floor is far below half of that: the GPU host's CPUs are shared, and there a
    # graph also costs a launch and its staging.
    assert graphs >= 200, text
    assert int(text.split("(")[1].split("held to Dijkstra")[0]) >= 40, text


def test_fuzz_msgs_fixed_seed():
    text = run_fuzzer("fuzz_msgs.py", 10, 308)
    maps = int(text.split("fuzz ok:")[1].split("maps")[0])
    # What a case costs is the mpmath side of the scan reference (tests/_scan_reference.py) and the oracle's conversions.  Measured
    # on a CPU-only machine with the engine's answers replaced by the oracle's own: 123 maps and 93 000 rays in 10 s with this
    # seed (125 and 120 maps with seeds 1 and 2).  The floor is far below half of that: the GPU host's CPUs are shared, and there
    # a map also costs an engine, its uploads and the launches.
    assert maps >= 30, text
    assert int(text.split("(")[1].split("batches through the device form")[0]) >= 10, text


def test_fuzz_rrt_fixed_seed():
    text = run_fuzzer("fuzz_rrt.py", 10, 309)
    maps = int(text.split("fuzz ok:")[1].split("maps")[0])
    # What a case costs is the oracle (budgets up to 30 000 samples a query).  Measured on a CPU-only machine with the engine's
    # answers replaced by the oracle's own (so the oracle side ran twice): 25 maps and 310 queries in 10 s with this seed (39 and
    # 32 maps with seeds 1 and 2).  The floor is below half of that: the GPU host's CPUs are shared, and there a map also costs
    # an engine, its uploads and the launch.  The first 8 maps of this seed hold 5 device-form batches, 4 moved maps and 4 values
    # of max_path_len below the paths.
    assert maps >= 8, text
    assert int(text.split("maps (")[1].split("through the device form")[0]) >= 3, text
    assert int(text.split("out of budget;")[1].split("paths cut")[0]) >= 1, text
