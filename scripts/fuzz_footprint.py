"""Developer tool: time-boxed random parity run of the robot radius (csrc/footprint.hip) against the reference's own
CircleIterator (oracle/_ref; the pinned restatement og_circle_cells where it was not built): every byte of the blocked set
and of the neighbour masks, and GlobalPlanner::ifBlocked at 500 positions (inside, on the edges, on cell corners, outside),
over resolutions 0.05 / 0.1 / 0.2 / 0.025 / 0.03 m, map shapes of 20-140 cells a side, origins up to +-2000 m, radii of k
cells, k + 1/2 cells and anything up to 12 cells, maps moved 0-2 times, unknown cells and obstacles on the map's edges.
usage: python scripts/fuzz_footprint.py [seconds] [seed]
Exits non-zero on the first mismatch and prints the configuration that reproduces it."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (initialises the HIP runtime before librna.so loads)
import ros_navigation_amd as R  # noqa: E402
import _oracle as O  # noqa: E402
import test_gpu_footprint as T  # noqa: E402  (the oracle of the footprint's tests: disc lists, blocked set, maps)
from _gpu import map_nbr  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
torch.zeros(1, device="cuda")
rng = np.random.default_rng(seed)
t_end = time.time() + budget
cases = cells = moves = positions = blocked_cells = blocked_positions = 0
by_res = {}


def fail(what, here, *more):
    print("MISMATCH", what, here, *more)
    sys.exit(1)


while time.time() < t_end:
    res = float(rng.choice([0.05, 0.1, 0.2, 0.025, 0.03]))
    rows, cols = int(rng.integers(20, 141)), int(rng.integers(20, 141))
    pos = (float(rng.uniform(-2000.0, 2000.0)), float(rng.uniform(-2000.0, 2000.0)))
    kind = int(rng.integers(0, 3))
    if kind == 0:
        r = float(rng.integers(1, 13)) * res                  # a whole number of cells: ties on the axes
    elif kind == 1:
        r = (float(rng.integers(0, 12)) + 0.5) * res          # k + 1/2 cells: the box corners on cell boundaries
    else:
        r = float(rng.uniform(0.0, 12.0)) * res or res
    mseed = int(rng.integers(0, 1 << 30))
    cfg = dict(res=res, rows=rows, cols=cols, pos=pos, r=r, mseed=mseed, fuzz_seed=seed, case=cases, moves=[])
    e = R.Engine(rows * res, cols * res, res, *pos)
    g = O.make_geom(rows * res, cols * res, res, *pos)
    if (e.rows, e.cols) != (rows, cols) or (g.size[0], g.size[1]) != (rows, cols):
        fail("size", cfg, (e.rows, e.cols), (g.size[0], g.size[1]))
    master = T.sample_map(rows, cols, seed=mseed, occupied=float(rng.choice([0.0, 0.004, 0.02])))
    e.upload(R.capi.LAYER_MASTER, master)
    for k in range(int(rng.integers(0, 3))):
        target = (g.pos[0] + float(rng.uniform(-0.6, 0.6)) * rows * res, g.pos[1] + float(rng.uniform(-0.6, 0.6)) * cols * res)
        ptrs = (C.POINTER(C.c_float) * 1)(O.fptr(master))
        regs = (O.Region * 4)()
        mv = C.c_int(0)
        O.lib().og_move(C.byref(g), ptrs, 1, O.d2(*target), regs, C.byref(mv))
        e.move(*target)
        cfg["moves"].append(target)
        ge = e.geometry()
        if tuple(ge.start_index) != tuple(g.start) or tuple(ge.position) != tuple(g.pos):
            fail("move", cfg, tuple(ge.start_index), tuple(g.start), tuple(ge.position), tuple(g.pos))
        if rng.random() < 0.3:                                # a fresh map over what the move left (buffer order)
            master = T.sample_map(rows, cols, seed=mseed + 1 + k)
            e.upload(R.capi.LAYER_MASTER, master)
        moves += 1
    T._discs.clear()
    e.astar_robot_radius(r)
    want = T.ref_blocked(g, master, r)
    got = e.astar_blocked_mask()
    bad = np.flatnonzero(got != want)
    if bad.size:
        fail("blocked set", cfg, bad[:8], got[bad[:8]], want[bad[:8]])
    if not np.array_equal(e.nbr_mask(), map_nbr(g, want)):
        fail("neighbour masks", cfg)
    # ifBlocked: uniform up to r + a cell outside the map, a fifth on its edges, a fifth on cell corners
    n = 500
    L = np.array([rows * res, cols * res])
    lo, hi = np.array(g.pos) - L / 2, np.array(g.pos) + L / 2
    xy = rng.uniform(lo - r - res, hi + r + res, (n, 2))
    xy[:50, 0] = rng.choice([lo[0], hi[0]], 50)
    xy[50:100, 1] = rng.choice([lo[1], hi[1]], 50)
    xy[100:200] = lo + res * np.stack([rng.integers(0, rows + 1, 100), rng.integers(0, cols + 1, 100)], axis=1)
    rq = r if rng.random() < 0.7 else float(rng.uniform(0.0, 14.0)) * res
    occ = (~np.isnan(master)) & (master > 0)
    want_p = np.zeros(n, np.uint8)
    for k in range(n):
        c = O.circle_cells(g, tuple(xy[k]), rq, reference=T.REFERENCE)
        ok = (c[:, 0] >= 0) & (c[:, 0] < rows) & (c[:, 1] >= 0) & (c[:, 1] < cols)
        want_p[k] = occ[c[ok, 0] + c[ok, 1] * rows].any()
    got_p = e.if_blocked(xy, rq)
    bad = np.flatnonzero(got_p != want_p)
    if bad.size:
        fail("if_blocked", dict(cfg, radius=rq), [tuple(p) for p in xy[bad[:5]]], got_p[bad[:5]], want_p[bad[:5]])
    e.close()
    cases += 1
    cells += rows * cols
    positions += n
    blocked_cells += int(want.sum())
    blocked_positions += int(want_p.sum())
    by_res[res] = by_res.get(res, 0) + 1
print("fuzz ok (%s): %d maps (%d cells, %d blocked; %d moves), %d positions (%d blocked) in %.0f s, seed %d; maps per resolution %s"
      % ("the reference's CircleIterator" if T.REFERENCE else "og_circle_cells", cases, cells, blocked_cells, moves, positions,
         blocked_positions, budget, seed, " ".join("%g:%d" % kv for kv in sorted(by_res.items()))))
