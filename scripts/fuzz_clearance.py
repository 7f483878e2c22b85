"""Developer tool: time-boxed random parity run of the clearance field (csrc/clearance.hip) and of the goal field's clearance
cost (csrc/goal_field.hip) against the integer oracles of tests/test_gpu_clearance.py: every cell of the clearance field,
and field / next of a goal field built with a random cost table, over random map shapes (not multiples of the 64-cell tile),
obstacle densities, unknown cells, caps 1..63, robot radii and moved maps.
usage: python scripts/fuzz_clearance.py [seconds] [seed]
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
import test_gpu_clearance as T  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
torch.zeros(1, device="cuda")
rng = np.random.default_rng(seed)
t_end = time.time() + budget
maps = clearances = fields = moved = with_radius = 0

while time.time() < t_end:
    rows, cols = int(rng.integers(3, 300)), int(rng.integers(3, 300))
    density = float(rng.choice([0.0, 0.02, 0.1, 0.3]))
    mseed = int(rng.integers(0, 1 << 30))
    cfg = dict(rows=rows, cols=cols, density=density, mseed=mseed, fuzz_seed=seed, map=maps)
    e = R.Engine(rows * 0.05, cols * 0.05, 0.05)
    assert (e.rows, e.cols) == (rows, cols)
    if rng.random() < 0.4:
        e.upload(R.capi.LAYER_MASTER, np.zeros(rows * cols, np.float32))
        e.move(float(rng.uniform(-0.4, 0.4) * rows * 0.05), float(rng.uniform(-0.4, 0.4) * cols * 0.05))
        moved += 1
    master = R.synth.obstacles_rect(rows, cols, density=density, seed=mseed, side=(1, max(2, min(rows, cols) // 4))).copy()
    if rng.random() < 0.5:
        master[rng.random(rows * cols) < 0.05] = np.nan
    if rng.random() < 0.3:
        master[rng.integers(0, rows * cols, 3)] = 200.0      # a few single cells
    e.upload(R.capi.LAYER_MASTER, master)
    if rng.random() < 0.4:
        cfg["radius"] = float(rng.choice([0.05, 0.15, 0.3, 0.62]))
        e.astar_robot_radius(cfg["radius"])
        with_radius += 1
    try:
        for cap in [int(c) for c in rng.choice([1, 2, 7, 20, 40, 62, 63], 2)]:
            cfg["cap"] = cap
            T.check_clearance(e, cap)
            clearances += 1
        n = int(rng.integers(2, 65))
        table = rng.integers(0, int(rng.choice([1, 50, 3000, 65536])), n).astype(np.uint16)
        cfg["table"] = table.tolist()
        e.goal_field_clearance_cost(table)
        blocked = e.astar_blocked_mask()
        cells = np.flatnonzero(blocked == 0) if (blocked == 0).any() and rng.random() < 0.9 else np.arange(rows * cols)
        cfg["goal"] = goal = int(rng.choice(cells))
        got = T.check_field(e, goal, table)
        if got is not None and rows * cols <= 40000:
            want, want_nx, pen, _ = got
            starts = np.concatenate([rng.integers(0, rows * cols, 30), [goal, -1, rows * cols]]).astype(np.int32)
            T.check_paths(e, want, want_nx, starts, int(rng.choice([8, 64, 4096])))
        fields += 1
    except AssertionError as err:
        print("MISMATCH", cfg, str(err)[:2000])
        sys.exit(1)
    e.close()
    maps += 1

print("fuzz_clearance ok: %d maps (%d moved, %d with a robot radius), %d clearance fields, %d goal fields with a cost table, every cell equal"
      % (maps, moved, with_radius, clearances, fields))
