"""Developer tool: time-boxed random parity run of the view-point information gain (csrc/viewgain.hip) against the integer oracle
of tests/test_gpu_view_gain.py: every record (status, unknown, visible, occupied) of random view cells -- out-of-range indices
and occupied cells among them --, over random maps (shapes that are no multiples of the 64-cell tile, occupied cells at a
random density, unknown discs and rectangles, walls), moved maps, radii 1..127 (the word edges of the window's bitmap rows
more often than the rest) and both flag values.
usage: python scripts/fuzz_view_gain.py [seconds] [seed]
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
import test_gpu_view_gain as T  # noqa: E402
from _gpu import to_buffer  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
torch.zeros(1, device="cuda")
rng = np.random.default_rng(seed)
t_end = time.time() + budget
maps = moved = calls = points = evaluated = rays = 0
EDGES = (1, 2, 15, 16, 31, 32, 47, 48, 63, 64, 95, 96, 126, 127)


def random_map(rows, cols, rng):
    """[j, i]: free with occupied cells at a random density, then walls, unknown discs and rectangles (or the other way round:
    unknown everywhere with known rectangles)"""
    if rng.random() < 0.25:
        m = np.full((cols, rows), np.nan, np.float32)
        for _ in range(int(rng.integers(1, 8))):
            w, h = rng.integers(3, max(4, min(rows, cols) // 2) + 1, 2)
            i, j = rng.integers(0, rows), rng.integers(0, cols)
            m[j:j + h, i:i + w] = 0.0
    else:
        m = np.zeros((cols, rows), np.float32)
    m[rng.random((cols, rows)) < rng.choice([0.0, 0.01, 0.05, 0.3])] = 180.0
    for _ in range(int(rng.integers(0, 4))):
        if rng.random() < 0.5:
            m[rng.integers(0, cols), :] = 180.0
        else:
            m[:, rng.integers(0, rows)] = 180.0
    jj, ii = np.mgrid[0:cols, 0:rows]
    for _ in range(int(rng.integers(0, 8))):
        ci, cj, r = rng.integers(0, rows), rng.integers(0, cols), rng.integers(1, 30)
        m[(ii - ci) ** 2 + (jj - cj) ** 2 <= r * r] = np.nan
    for _ in range(int(rng.integers(0, 6))):
        w, h = rng.integers(1, 12, 2)
        i, j = rng.integers(0, rows), rng.integers(0, cols)
        m[j:j + h, i:i + w] = rng.choice([0.0, np.nan])
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
    e.upload(R.capi.LAYER_MASTER, to_buffer(random_map(rows, cols, rng), rows, cols, g.start_index[0], g.start_index[1]))
    w = T.Want(e, R)
    try:
        for _ in range(int(rng.integers(1, 4))):
            cfg["radius"] = radius = int(rng.choice(EDGES)) if rng.random() < 0.5 else int(rng.integers(1, 128))
            n = int(rng.integers(1, 6 if radius > 64 else 40))
            cfg["cells"] = cells = rng.integers(-2, rows * cols + 2, n).tolist()
            _, clear, _ = T.check(e, R, cells, radius, w)
            calls += 2
            points += 2 * n
            evaluated += 2 * sum(t[0] == 0 for t in clear)
            rays += 2 * 8 * radius * sum(t[0] == 0 for t in clear)
    except (AssertionError, R.capi.RnaError) as err:
        print("MISMATCH", cfg, str(err)[:2000])
        sys.exit(1)
    e.close()
    maps += 1

print("fuzz_view_gain ok: %d maps (%d moved), %d calls, %d view points (%d evaluated, %d rays), every record equal"
      % (maps, moved, calls, points, evaluated, rays))
