"""View-point information gain (csrc/viewgain.hip) on one MI355X, on the explored bench map of scripts/frontier_rows.py (4096 x
4096, config 3, seed 7: NaN outside a union of discs along a random walk, about a quarter of the map known).

  (a) view_gain   rna_view_gain at the `nearest` cells of the ranked frontiers (min_size 8), at 1 024 frontier cells and at
                  every frontier cell of the map, R = 60 and 127, RNA_VIEW_UNKNOWN_OPAQUE off and on: the host form (upload,
                  kernel, download) and the _device form (the kernel alone), with the byte floor of each case
  (b) frontiers   the same run's rna_frontiers_build (ranked, min_size 8, count only)
  (c) goal_field  the same run's rna_goal_field_build from the robot's cell
  (d) floor       (2R + 1)^2 x 4 B of master per view point at the HBM rate of DESIGN.md section 3 (8 TB/s)

Every row is the whole call timed by HIP events on the engine's stream around it (us_events) and by the host's clock
(us_wall): a warm-up, then the median of --reps.  The ray-to-thread deal is a developer knob of the library read once per
process (RNA_VIEW_GAIN_DEAL), so the script runs itself in a fresh child process once with the library's own choice (by the
flag) and once per forced deal, and reports all three.
One JSON object on stdout (and into --out).  Usage: python3 scripts/view_gain_rows.py [--reps 5] [--seed 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from frontier_rows import GRID, HBM_BYTES_PER_S, RES, explored  # noqa: E402

DEALS = {"by_flag": None, "spread": "1", "adjacent": "0"}   # by_flag: the library's own choice (knob unset)


def one_deal(args):
    import torch
    import ros_navigation_amd as R
    n = GRID
    master, robot, known_share = explored(R.synth.obstacles_rect(n, n), args.seed, args.discs)
    e = R.Engine(n * RES, n * RES, RES)
    e.upload(R.capi.LAYER_MASTER, master)
    e.nbr_mask()                                     # masks in place: no row pays for their refresh
    stream = torch.cuda.ExternalStream(e._L.rna_stream(e.h), device=torch.device("cuda", 0))
    out = {"deal": args.deal, "known_share": known_share, "robot_cell": robot}

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

    info = {}
    out["goal_field"] = timed(lambda: info.update(e.goal_field(robot)))
    out["goal_field"].update(rounds=info["rounds"], tile_jobs=info["tile_jobs"], reached=info["reached"])
    got = {}
    out["frontiers ranked min_size=8"] = timed(lambda: got.update(e.frontiers(min_size=8, rank=True, cap=0)[1]))
    out["frontiers ranked min_size=8"].update(cells=got["cells"], clusters=got["clusters"])
    recs, _ = e.frontiers(min_size=8, rank=True, cap=max(1, got["clusters_all"]))
    every = np.flatnonzero(e.frontier_labels() >= 0).astype(np.int32)
    some = np.random.default_rng(args.seed).permutation(every)[:1024]
    cases = {"nearest of ranked frontiers": recs["nearest"].astype(np.int32), "1024 frontier cells": some, "every frontier cell": every}
    out["view_gain"] = {}
    for name, cells in cases.items():
        d_cells = torch.from_numpy(cells).cuda()
        d_out = torch.zeros(4 * len(cells), dtype=torch.int32, device="cuda")
        for radius in (60, 127):
            floor_us = 1e6 * len(cells) * (2 * radius + 1) ** 2 * 4 / HBM_BYTES_PER_S
            for opaque in (False, True):
                res = {}
                row = {"view_points": int(len(cells)), "radius": radius, "unknown_opaque": int(opaque), "floor_us": floor_us}
                row["host_form"] = timed(lambda: res.update(r=e.view_gain(cells, radius, unknown_opaque=opaque)))
                row["device_form"] = timed(lambda: e.view_gain_device(d_cells.data_ptr(), len(cells), radius, d_out.data_ptr(), opaque))
                r = res["r"]
                dev = d_out.cpu().numpy().view(R.capi.VIEW_GAIN_DTYPE)
                assert dev.tobytes() == r.tobytes()
                ok = r[r["status"] == 0]
                row.update(evaluated=int(len(ok)), mean_unknown=float(ok["unknown"].mean()) if len(ok) else 0.0,
                           mean_visible=float(ok["visible"].mean()) if len(ok) else 0.0,
                           device_over_floor=row["device_form"]["us_events"] / floor_us)
                out["view_gain"]["%s R=%d %s" % (name, radius, "opaque" if opaque else "transparent")] = row
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--discs", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--deal", choices=sorted(DEALS), default=None, help="(internal) measure this deal in this process")
    args = ap.parse_args()
    if args.deal:
        if DEALS[args.deal] is None:
            os.environ.pop("RNA_VIEW_GAIN_DEAL", None)
        else:
            os.environ["RNA_VIEW_GAIN_DEAL"] = DEALS[args.deal]      # before librna.so is loaded
        print(json.dumps(one_deal(args)))
        return
    out = {"grid": GRID, "resolution": RES, "reps": args.reps, "seed": args.seed, "discs": args.discs,
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "deals": {}}
    for deal in DEALS:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--deal", deal, "--reps", str(args.reps), "--seed", str(args.seed),
                              "--discs", str(args.discs)], capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            sys.exit(run.returncode or 1)
        out["deals"][deal] = json.loads(run.stdout.strip().splitlines()[-1])
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
