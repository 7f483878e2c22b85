"""The line-of-sight shortcut (csrc/shortcut.hip) on one MI355X, on the bench's map (4096 x 4096, config 3) with the paths of
the bench's 256 queries:

  search     rna_astar_batch_device for the 256 queries (pipeline depth 1), by HIP events on the engine's stream around the
             call and the rna_synchronize that makes its outputs valid -- the comparator
  shortcut   rna_shortcut_paths_device on those paths for max_span 0 and 256, without and with keep_clearance (clearance
             field R = 20 in place, masks in place), by HIP events around the call: a warm-up, then the median of --reps;
             next to each the way points per path and the longest leg, and the ratio to the search

One JSON object on stdout (and into --out, default profiles/shortcut_rows.json).
Usage: python3 scripts/shortcut_rows.py [--reps 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRID, RES, NQ, MAX_LEN, MAX_WP = 4096, 0.05, 256, 16384, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shortcut_rows.json"))
    args = ap.parse_args()
    import torch
    import ros_navigation_amd as R
    n = GRID
    e = R.Engine(n * RES, n * RES, RES)
    master = R.synth.obstacles_rect(n, n)
    e.upload(R.capi.LAYER_MASTER, master)
    e.astar_pipeline_depth(1)
    e.astar_configure(max_queries=NQ)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(e._L.rna_stream(e.h), device=dev)
    q = R.synth.astar_queries(NQ, master, n, n)
    d_q = torch.from_numpy(q.view(np.int32).copy()).to(dev)
    d_paths = torch.zeros(NQ * MAX_LEN, dtype=torch.int32, device=dev)
    d_res = torch.zeros(NQ * 6, dtype=torch.int32, device=dev)
    d_wp = torch.zeros(NQ * MAX_WP, dtype=torch.int32, device=dev)
    d_out = torch.zeros(NQ * 4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def timed(fn, sync=False):
        fn()                                              # warm-up
        e.synchronize()
        us = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            if sync:
                e.synchronize()                           # (the searches run on the pipeline stage's own stream)
            b.record(stream)
            b.synchronize()
            e.synchronize()
            us.append(1000.0 * a.elapsed_time(b))
        return {"us": statistics.median(us), "us_min": min(us), "us_max": max(us)}

    out = {"grid": GRID, "resolution": RES, "queries": NQ, "reps": args.reps}
    out["search"] = timed(lambda: e.astar_device(d_q.data_ptr(), NQ, d_paths.data_ptr(), MAX_LEN, d_res.data_ptr()), sync=True)
    res = d_res.cpu().numpy().view(R.capi.ASTAR_RESULT_DTYPE)
    found = res["status"] == 0
    out["paths"] = {"found": int(found.sum()), "cells_median": float(np.median(res["path_len"][found])), "cells_max": int(res["path_len"][found].max())}
    e.clearance(20)
    out["shortcut"] = {}
    for span in (0, 256):
        for keep in (False, True):
            row = timed(lambda: e.shortcut_paths_device(d_paths.data_ptr(), d_res.data_ptr(), NQ, MAX_LEN, d_wp.data_ptr(), MAX_WP,
                                                        d_out.data_ptr(), max_span=span, keep_clearance=keep))
            sc = d_out.cpu().numpy().view(R.capi.SHORTCUT_RESULT_DTYPE)
            ok = sc["status"] == 0
            row.update({"ok": int(ok.sum()), "waypoints_median": float(np.median(sc["n_waypoints"][ok])),
                        "waypoints_max": int(sc["n_waypoints"][ok].max()), "longest_span_max": int(sc["longest_span"][ok].max()),
                        "blocked_steps": int(sc["blocked_steps"][ok].sum()), "ratio_to_search": row["us"] / out["search"]["us"]})
            out["shortcut"]["max_span=%d keep_clearance=%d" % (span, int(keep))] = row
    e.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
