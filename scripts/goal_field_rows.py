"""The goal distance field (csrc/goal_field.hip) on one MI355X, on the bench's map (4096 x 4096, config 3), for four goals
taken from synth.astar_queries:

  build        host wall time of rna_goal_field_build (its round loop is part of it): a warm-up build, then the median of
               --reps builds; rounds, tile_jobs / tiles_reached (the work inflation) -- for every --widths entry (the tile
               ordering's threshold in cost units through the developer knob RNA_GOAL_FIELD_WIDTH; 0 = plain rounds)
  paths        rna_goal_field_paths_device for 256 and 4096 starts, HIP events on the engine's stream, median of --reps
  comparator   in the same run: rna_astar_batch_device + rna_synchronize on the 256 queries (s_i -> that goal) at pipeline
               depth 1, host wall time, median of --reps -- the batch search this change does not touch
  break_even   starts per goal from which the field wins: build / (comparator per query - path per start)
  floor_mb     what a build has to move at least: 1 B mask read + 4 B field + 1 B next written per cell

One JSON object on stdout (and into --out).  Usage: python3 scripts/goal_field_rows.py [--reps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--widths", default="0,32000,64000,128000,256000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import ros_navigation_amd as R
    n, res = args.grid, 0.05
    e = R.Engine(n * res, n * res, res)
    master = R.synth.obstacles_rect(n, n)
    e.upload(R.capi.LAYER_MASTER, master)
    q = R.synth.astar_queries(4096, master, n, n)
    goals = [int(g) for g in q["goal"][:4]]
    starts = q["start"].astype(np.int32)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(e._L.rna_stream(e.h), device=dev)
    max_len = 16384
    d_starts = torch.from_numpy(starts).to(dev)
    d_paths = torch.zeros(4096 * max_len, dtype=torch.int32, device=dev)
    d_res = torch.zeros(4096 * 6, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    widths = [int(w) for w in args.widths.split(",")]
    default = os.environ.get("RNA_GOAL_FIELD_WIDTH")
    out = {"grid": n, "resolution": res, "reps": args.reps, "floor_mb": 6 * n * n / 1e6, "goals": []}
    e.astar_pipeline_depth(1)
    e.astar_configure(max_queries=256)
    for goal in goals:
        row = {"goal": goal, "build": {}}
        for w in widths + ["default"]:
            if w == "default":
                if default is None:
                    os.environ.pop("RNA_GOAL_FIELD_WIDTH", None)
                else:
                    os.environ["RNA_GOAL_FIELD_WIDTH"] = default
            else:
                os.environ["RNA_GOAL_FIELD_WIDTH"] = str(w)
            info = e.goal_field(goal)   # warm-up
            ms = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                info = e.goal_field(goal)
                ms.append(1000.0 * (time.perf_counter() - t0))
            row["build"][str(w)] = {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "rounds": info["rounds"],
                                    "tile_jobs": info["tile_jobs"], "tiles_reached": info["tiles_reached"],
                                    "jobs_per_tile": info["tile_jobs"] / max(info["tiles_reached"], 1), "reached": info["reached"]}
        # (the field now in place is the default build's)
        row["paths"] = {}
        for k in (256, 4096):
            e.goal_field_paths_device(d_starts.data_ptr(), k, d_paths.data_ptr(), max_len, d_res.data_ptr())
            e.synchronize_map()
            ms = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                e.goal_field_paths_device(d_starts.data_ptr(), k, d_paths.data_ptr(), max_len, d_res.data_ptr())
                b.record(stream)
                b.synchronize()
                ms.append(a.elapsed_time(b))
            r = d_res.cpu().numpy().view(R.capi.ASTAR_RESULT_DTYPE)[:k]
            row["paths"][str(k)] = {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "found": int((r["status"] == 0).sum()),
                                    "mean_path_len": float(r["path_len"][r["status"] == 0].mean())}
        # comparator: the batch search on the same 256 pairs
        qq = np.zeros(256, R.capi.ASTAR_QUERY_DTYPE)
        qq["start"], qq["goal"] = starts[:256], goal
        d_q = torch.from_numpy(qq.view(np.int32).copy()).to(dev)
        torch.cuda.synchronize()
        ms = []
        for it in range(args.reps + 1):
            t0 = time.perf_counter()
            e.astar_device(d_q.data_ptr(), 256, d_paths.data_ptr(), max_len, d_res.data_ptr())
            e.synchronize()
            if it:
                ms.append(1000.0 * (time.perf_counter() - t0))
        r = d_res.cpu().numpy().view(R.capi.ASTAR_RESULT_DTYPE)[:256]
        row["comparator_astar_256"] = {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "found": int((r["status"] == 0).sum())}
        per_query = row["comparator_astar_256"]["ms"] / 256
        per_start = row["paths"]["256"]["ms"] / 256
        row["break_even_starts"] = row["build"]["default"]["ms"] / (per_query - per_start) if per_query > per_start else None
        out["goals"].append(row)
    e.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
