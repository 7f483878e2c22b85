"""Developer tool: time-boxed random parity run of the line-of-sight shortcut (csrc/shortcut.hip) against the sequential
definition in plain Python (the oracle of tests/test_gpu_shortcut.py): way points, counts, blocked_steps, longest_span and
statuses of every path, over random map shapes (not multiples of the 64-cell tile), obstacle densities, robot radii, moved
maps, max_span (chunk edges among them) and keep_clearance.  Paths come from Engine.astar and from the goal field; a share of
the maps gets obstacles dropped on its finished paths, and a few rows are corrupted by hand.
usage: python scripts/fuzz_shortcut.py [seconds] [seed]
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
import test_gpu_shortcut as T  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
torch.zeros(1, device="cuda")
rng = np.random.default_rng(seed)
t_end = time.time() + budget
maps = moved = with_radius = calls = kept = rows_checked = stale_maps = 0

while time.time() < t_end:
    rows, cols = int(rng.integers(3, 260)), int(rng.integers(3, 260))
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
    e.upload(R.capi.LAYER_MASTER, master)
    if rng.random() < 0.3:
        cfg["radius"] = float(rng.choice([0.05, 0.15, 0.3]))
        e.astar_robot_radius(cfg["radius"])
        with_radius += 1
    try:
        free = np.flatnonzero(e.astar_blocked_mask() == 0)
        if len(free) < 2:
            e.close()
            continue
        n = 32
        max_len = int(rng.choice([16, 64, 130, 1024]))
        cfg["max_len"] = max_len
        if rng.random() < 0.5:
            q = np.zeros(n, R.capi.ASTAR_QUERY_DTYPE)
            q["start"], q["goal"] = rng.choice(free, n), rng.choice(free, n)
            q["start"][0] = -1
            res, paths = e.astar(q, max_len)
            cfg["source"] = "astar"
        else:
            cap = int(rng.choice([3, 7, 20]))
            if rng.random() < 0.6:
                e.goal_field_clearance_cost(rng.integers(0, 4000, cap + 1).astype(np.uint16))
            e.goal_field(int(rng.choice(free)))
            starts = rng.choice(free, n).astype(np.int32)
            starts[0] = rows * cols
            paths, res = e.goal_field_paths(starts, max_len)
            cfg["source"] = "goal_field"
        if rng.random() < 0.3:                               # hand-made damage: status 2, the other rows unaffected
            k = int(rng.integers(0, n))
            paths[k, int(rng.integers(0, max_len))] = int(rng.choice([-1, rows * cols, rng.integers(0, rows * cols)]))
        if rng.random() < 0.3:                               # obstacles land on finished paths
            hit = np.concatenate([paths[k][:res["path_len"][k]] for k in np.flatnonzero(res["status"] == 0)] or [np.zeros(0, np.int32)])
            hit = hit[(hit >= 0) & (hit < rows * cols)]
            if len(hit):
                buf = e.download(R.capi.LAYER_MASTER)
                buf[rng.choice(hit, 4)] = 150.0
                e.upload(R.capi.LAYER_MASTER, buf)
                stale_maps += 1
        keep_ok = False
        if rng.random() < 0.5:
            e.clearance(int(rng.choice([1, 5, 20, 63])))
            keep_ok = True
        ora = T.Oracle(e, keep_ok)
        for _ in range(3):
            keep = bool(keep_ok and rng.random() < 0.6)
            span = int(rng.choice([0, 0, 2, 3, 17, 63, 64, 65, 200]))
            mw = int(rng.choice([2, 5, max(2, max_len)]))
            cfg.update(span=span, keep=keep, max_waypoints=mw)
            T.check(e, paths, res, max_span=span, keep=keep, max_waypoints=mw, oracle=ora)
            calls += 1
            kept += int(keep)
            rows_checked += n
    except AssertionError as err:
        print("MISMATCH", cfg, str(err)[:2000])
        sys.exit(1)
    e.close()
    maps += 1

print("fuzz_shortcut ok: %d maps (%d moved, %d with a robot radius, %d with obstacles dropped on finished paths), %d calls (%d with "
      "keep_clearance), %d paths, every way point and count equal" % (maps, moved, with_radius, stale_maps, calls, kept, rows_checked))
