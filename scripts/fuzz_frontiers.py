"""Developer tool: time-boxed random parity run of the exploration frontiers (csrc/frontier.hip) against the integer oracle of
tests/test_gpu_frontiers.py: the label of every cell, every record, the info and the order, over random explored maps (shapes
that are no multiples of the 64-cell tile, known rectangles, obstacles, unknown holes, single known cells, corridors), moved
maps, robot radii, min_size 1..12, and ranking on and off (by a goal field rooted at a random free cell, with and without a
clearance-cost table).
usage: python scripts/fuzz_frontiers.py [seconds] [seed]
Exits non-zero on the first mismatch and prints the configuration that reproduces it."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (initialises the HIP runtime before librna.so loads)
import ros_navigation_amd as R  # noqa: E402
import test_gpu_frontiers as T  # noqa: E402
from _gpu import to_buffer  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
torch.zeros(1, device="cuda")
rng = np.random.default_rng(seed)
t_end = time.time() + budget
maps = builds = ranked = moved = with_radius = cells = clusters = 0


def random_map(rows, cols, rng):
    """[j, i]: unknown everywhere, then known rectangles, obstacles, unknown holes, single known cells, thin corridors"""
    m = np.full((cols, rows), np.nan, np.float32)

    def rect(value, lo, hi, count):
        for _ in range(count):
            w, h = rng.integers(lo, hi + 1, 2)
            i, j = rng.integers(0, rows), rng.integers(0, cols)
            m[j:j + h, i:i + w] = value
    rect(0.0, 3, max(4, min(rows, cols) // 2), int(rng.integers(1, 10)))
    rect(180.0, 1, 9, int(rng.integers(0, 10)))
    rect(np.nan, 1, 6, int(rng.integers(0, 14)))
    for _ in range(int(rng.integers(0, 40))):
        m[rng.integers(0, cols), rng.integers(0, rows)] = 0.0
    for _ in range(int(rng.integers(0, 4))):
        m[rng.integers(0, cols), :] = 0.0
        m[:, rng.integers(0, rows)] = 0.0
    return m


while time.time() < t_end:
    rows, cols = int(rng.integers(3, 300)), int(rng.integers(3, 300))
    cfg = dict(rows=rows, cols=cols, fuzz_seed=seed, map=maps)
    e = R.Engine(rows * 0.05, cols * 0.05, 0.05)
    assert (e.rows, e.cols) == (rows, cols)
    if rng.random() < 0.4:
        e.upload(R.capi.LAYER_MASTER, np.zeros(rows * cols, np.float32))
        e.move(float(rng.uniform(-0.4, 0.4) * rows * 0.05), float(rng.uniform(-0.4, 0.4) * cols * 0.05))
        moved += 1
    g = e.geometry()
    m = T.serpentine(rows, cols, int(rng.integers(2, 5))) if rng.random() < 0.1 else random_map(rows, cols, rng)
    e.upload(R.capi.LAYER_MASTER, to_buffer(m, rows, cols, g.start_index[0], g.start_index[1]))
    if rng.random() < 0.4:
        cfg["radius"] = float(rng.choice([0.05, 0.15, 0.3]))
        e.astar_robot_radius(cfg["radius"])
        with_radius += 1
    try:
        w, _ = T.check(e, R)
        builds += 1
        cells += w.cells
        clusters += len(w.records)
        cfg["min_size"] = min_size = int(rng.integers(1, 13))
        T.check(e, R, min_size=min_size, want=w)
        builds += 1
        if rng.random() < 0.6:
            if rng.random() < 0.4:
                cfg["table"] = table = rng.integers(0, 3000, int(rng.integers(2, 20))).astype(np.uint16).tolist()
                e.goal_field_clearance_cost(np.array(table, np.uint16))
            free = np.flatnonzero((e.astar_blocked_mask() == 0) & ~np.isnan(e.download(R.capi.LAYER_MASTER)))
            if len(free):                                  # (no free cell: nothing to root a field at)
                cfg["robot"] = robot = int(rng.choice(free))
                e.goal_field(robot)
                T.check(e, R, min_size=int(rng.choice([1, min_size])), rank=True)
                builds += 1
                ranked += 1
    except (AssertionError, R.capi.RnaError) as err:
        print("MISMATCH", cfg, str(err)[:2000])
        sys.exit(1)
    e.close()
    maps += 1

print("fuzz_frontiers ok: %d maps (%d moved, %d with a robot radius), %d builds (%d ranked), %d frontier cells in %d clusters, "
      "every label and record equal" % (maps, moved, with_radius, builds, ranked, cells, clusters))
