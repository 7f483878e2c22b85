"""Exploration frontiers (csrc/frontier.hip) on one MI355X, on the bench's map (4096 x 4096, config 3) explored along a random
walk: NaN outside the union of --discs discs of 150-400 cells radius whose centres take a random walk from the map's middle.

  (a) frontiers   rna_frontiers_build, count only (cap 0): unranked and ranked, min_size 1 and 8, with the counts it reports
  (b) clearance   the same run's rna_clearance_build(20): the yardstick, a one-pass tile kernel over the same layer
  (c) goal_field  the same run's rna_goal_field_build from the robot's cell (the walk's start)
  (d) floor       64 MiB of master read + 64 MiB of labels written at the HBM rate of DESIGN.md section 3 (8 TB/s)

Every row is the whole call -- launches, kernels and the host's waits for the counts in between -- timed by HIP events on the
engine's stream around it (us_events) and by the host's clock (us_wall): a warm-up, then the median of --reps.
One JSON object on stdout (and into --out).  Usage: python3 scripts/frontier_rows.py [--reps 5] [--seed 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRID, RES = 4096, 0.05
HBM_BYTES_PER_S = 8e12


def explored(master, seed, discs):
    """the known part of the map: a union of discs along a random walk; returns (master with NaN elsewhere, robot cell, known share of the map)"""
    rng = np.random.default_rng(seed)
    n = GRID
    known = np.zeros((n, n), bool)
    ci = cj = n // 2
    for _ in range(discs):
        r = int(rng.integers(150, 401))
        i0, i1, j0, j1 = max(ci - r, 0), min(ci + r + 1, n), max(cj - r, 0), min(cj + r + 1, n)
        jj, ii = np.ogrid[j0:j1, i0:i1]
        known[j0:j1, i0:i1] |= (ii - ci) ** 2 + (jj - cj) ** 2 <= r * r
        ci = int(np.clip(ci + rng.integers(-300, 301), 0, n - 1))
        cj = int(np.clip(cj + rng.integers(-300, 301), 0, n - 1))
    m = master.reshape(n, n).copy()
    m[~known] = np.nan
    free = np.argwhere(known & ~(m > 0))
    centre = free[np.argmin(((free - n // 2) ** 2).sum(axis=1))]          # the free cell nearest the walk's start
    return np.ascontiguousarray(m.reshape(-1)), int(centre[1] + centre[0] * n), float(known.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--discs", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import ros_navigation_amd as R
    n = GRID
    master, robot, known_share = explored(R.synth.obstacles_rect(n, n), args.seed, args.discs)
    e = R.Engine(n * RES, n * RES, RES)
    e.upload(R.capi.LAYER_MASTER, master)
    e.nbr_mask()                                     # masks in place: no row pays for their refresh
    stream = torch.cuda.ExternalStream(e._L.rna_stream(e.h), device=torch.device("cuda", 0))
    out = {"grid": n, "resolution": RES, "reps": args.reps, "seed": args.seed, "discs": args.discs, "known_share": known_share,
           "robot_cell": robot}

    def timed(call):
        call()
        ev, wall = [], []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            t0 = time.perf_counter()
            call()
            wall.append(1e6 * (time.perf_counter() - t0))
            b.record(stream)
            b.synchronize()
            ev.append(1000.0 * a.elapsed_time(b))
        return {"us_events": statistics.median(ev), "us_events_min": min(ev), "us_events_max": max(ev), "us_wall": statistics.median(wall)}

    out["clearance_R20"] = timed(lambda: e._check(e._L.rna_clearance_build(e.h, 20)))
    info = {}
    out["goal_field"] = timed(lambda: info.update(e.goal_field(robot)))
    out["goal_field"].update(rounds=info["rounds"], tile_jobs=info["tile_jobs"], tiles_reached=info["tiles_reached"], reached=info["reached"])
    out["frontiers"] = {}
    for rank in (False, True):
        for min_size in (1, 8):
            got = {}
            row = timed(lambda: got.update(e.frontiers(min_size=min_size, rank=rank, cap=0)[1]))
            row.update(cells=got["cells"], clusters_all=got["clusters_all"], clusters=got["clusters"], largest=got["largest"])
            out["frontiers"]["%s min_size=%d" % ("ranked" if rank else "unranked", min_size)] = row
    recs, got = e.frontiers(min_size=8, rank=True, cap=max(1, got["clusters_all"]))
    reach = recs[recs["cost"] < R.capi.GOAL_FIELD_FAR]
    out["ranked_min_size_8"] = {"records": len(recs), "reachable": len(reach),
                                "cheapest_cost": int(reach["cost"].min()) if len(reach) else None}
    out["floor"] = {"bytes": 2 * n * n * 4, "hbm_bytes_per_s": HBM_BYTES_PER_S, "us": 1e6 * 2 * n * n * 4 / HBM_BYTES_PER_S}
    e.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
