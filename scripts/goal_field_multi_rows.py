"""The goal field with many sources and owner labels (csrc/goal_field.hip) on one MI355X, on the bench's map (4096 x 4096,
config 3) and on its explored variant of scripts/frontier_rows.py (seed 7):

  (a) single    rna_goal_field_build(goal) -- which now runs the parallel seed, the terminal kernel and the new finalize rule --
                in fresh processes, --rounds times alternating between --parent-lib (a librna.so built from the parent commit,
                next to librna.so) and this tree's library, four goals, a warm-up and --reps builds each: every single build
                time is kept; accepted when this tree's median lies inside the parent's own min-max widened by the 1 %
                box-to-box spread of DESIGN.md section 0
  (b) multi     rna_goal_field_build_multi with 16 sources (robots: the first 16 starts of synth.astar_queries, start costs
                0..15 x 1000) on the bench's map, and with every frontier cell of the explored map as a source
                (Engine.goal_field_from_frontiers, the torch selection included); rounds and tile jobs next to the single-goal
                build's on the same map
  (c) owners    the same two builds with RNA_GOAL_FIELD_OWNERS: the owner pass is the difference of the medians; its rounds, its
                share of the build, and its floor: `next` read once (1 B per cell) and the labels written once (4 B per cell)
                at the HBM rate of DESIGN.md section 3
  (d) today     what a user has without this: 16 single-goal builds, 16 downloads and the host's element-wise minimum (no
                `next` bytes, no owners); the ratio to (b)

Every row is the whole call by the host's clock, read-backs included: a warm-up, then the median of --reps.
One JSON object on stdout (and into --out).
Usage: python3 scripts/goal_field_multi_rows.py [--reps 5] [--rounds 5] [--parent-lib NAME] [--out FILE]"""
import argparse
import ctypes as C
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
GRID, RES = 4096, 0.05
HBM_BYTES_PER_S = 8e12
BOX_SPREAD = 0.01


def single_child(lib_name, reps):
    """single-goal builds through a minimal binding of its own (the parent's library lacks the new symbols)"""
    import torch  # noqa: F401  (one HIP runtime, loaded first)
    from ros_navigation_amd import synth
    L = C.CDLL(os.path.join(ROOT, "ros_navigation_amd", lib_name))
    vp = C.c_void_p
    L.rna_create.argtypes = [C.POINTER(vp), C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int]
    L.rna_layer_upload.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.rna_goal_field_build.argtypes = [vp, C.c_int32, vp]
    L.rna_destroy.argtypes = [vp]
    L.rna_destroy.restype = None
    h = vp()
    assert L.rna_create(C.byref(h), GRID * RES, GRID * RES, RES, 0.0, 0.0, 0) == 0
    master = np.ascontiguousarray(synth.obstacles_rect(GRID, GRID), np.float32)
    assert L.rna_layer_upload(h, 0, master.ctypes.data, master.size) == 0
    q = synth.astar_queries(4096, master, GRID, GRID)
    info = np.zeros(8, np.int32)
    out = {}
    for goal in [int(g) for g in q["goal"][:4]]:
        assert L.rna_goal_field_build(h, goal, info.ctypes.data) == 0   # warm-up
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            assert L.rna_goal_field_build(h, goal, info.ctypes.data) == 0
            ms.append(1000.0 * (time.perf_counter() - t0))
        out[str(goal)] = {"ms": ms, "median": statistics.median(ms), "rounds": int(info[4]), "tile_jobs": int(info[5]), "reached": int(info[2])}
    L.rna_destroy(h)
    print("SINGLE " + json.dumps(out))


def timed(call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append(1000.0 * (time.perf_counter() - t0))
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--discs", type=int, default=200)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child-single", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child_single:
        return single_child(args.child_single, args.reps)
    out = {"grid": GRID, "resolution": RES, "reps": args.reps, "rounds": args.rounds}

    # (a) processes of their own, one at a time, alternating
    libs = (["parent"] if args.parent_lib else []) + ["branch"]
    single = {k: [] for k in libs}
    for _ in range(args.rounds):
        for k in libs:
            name = args.parent_lib if k == "parent" else "librna.so"
            txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-single", name, "--reps", str(args.reps)], check=True,
                                 capture_output=True, text=True, timeout=600).stdout
            single[k].append(json.loads(next(l for l in txt.splitlines() if l.startswith("SINGLE "))[7:]))
    out["single"] = single
    verdict = {}
    for goal in single["branch"][0]:
        b = [t for r in single["branch"] for t in r[goal]["ms"]]
        row = {"branch_median_ms": statistics.median(b), "branch_every_build_ms": [min(b), max(b)]}
        if args.parent_lib:
            p = [t for r in single["parent"] for t in r[goal]["ms"]]
            lo, hi = min(p) * (1.0 - BOX_SPREAD), max(p) * (1.0 + BOX_SPREAD)
            row.update({"parent_median_ms": statistics.median(p), "parent_every_build_ms": [min(p), max(p)],
                        "accepted_range_ms": [lo, hi], "branch_inside": lo <= statistics.median(b) <= hi})
        verdict[goal] = row
    out["single_summary"] = verdict

    import ros_navigation_amd as R
    from frontier_rows import explored
    n = GRID
    bench_map = R.synth.obstacles_rect(n, n)
    q = R.synth.astar_queries(4096, bench_map, n, n)
    robots = q["start"][:16].astype(np.int32)
    busy = (np.arange(16) * 1000).astype(np.int32)
    floor_us = 1e6 * n * n * 5 / HBM_BYTES_PER_S
    out["owner_floor"] = {"bytes": n * n * 5, "hbm_bytes_per_s": HBM_BYTES_PER_S, "us": floor_us}

    def rows_for(e, build, label):
        """(b) and (c) of one source set: build(owners) -> info"""
        res = {}
        for owners in (False, True):
            info = {}
            row = timed(lambda: info.update(build(owners)), args.reps)
            src = e.goal_field_sources_info()
            row.update(rounds=info["rounds"], tile_jobs=info["tile_jobs"], tiles_reached=info["tiles_reached"], reached=info["reached"],
                       sources=src["sources"], blocked_sources=src["blocked_sources"], terminals=src["terminals"],
                       owner_rounds=src["owner_rounds"])
            res["owners" if owners else "plain"] = row
        pass_ms = res["owners"]["ms"] - res["plain"]["ms"]
        res["owner_pass"] = {"ms": pass_ms, "share_of_build": pass_ms / res["owners"]["ms"], "times_floor": 1000.0 * pass_ms / floor_us,
                             "owner_rounds": res["owners"]["owner_rounds"]}
        out[label] = res

    # the bench's map: the single goal, 16 robots, the comparator
    e = R.Engine(n * RES, n * RES, RES)
    e.upload(R.capi.LAYER_MASTER, bench_map)
    e.nbr_mask()                                         # masks in place: no row pays for their refresh
    info = {}
    row = timed(lambda: info.update(e.goal_field(int(robots[0]))), args.reps)
    row.update(rounds=info["rounds"], tile_jobs=info["tile_jobs"], tiles_reached=info["tiles_reached"])
    out["bench_map_single_goal"] = row
    rows_for(e, lambda owners: e.goal_field_multi(robots, busy, owners=owners), "bench_map_16_robots")

    def today():
        best = None
        for c, s in zip(robots, busy):
            e.goal_field(int(c))
            f = e.goal_field_download().astype(np.int64) + int(s)
            best = f if best is None else np.minimum(best, f)
        return best
    out["today_16_builds_16_downloads_host_minimum"] = timed(today, max(1, args.reps // 2))
    out["today_over_multi"] = out["today_16_builds_16_downloads_host_minimum"]["ms"] / out["bench_map_16_robots"]["plain"]["ms"]
    e.close()

    # the explored map: the robot's field, every frontier cell as a source
    master, robot, known_share = explored(bench_map, args.seed, args.discs)
    e = R.Engine(n * RES, n * RES, RES)
    e.upload(R.capi.LAYER_MASTER, master)
    e.nbr_mask()
    info = {}
    row = timed(lambda: info.update(e.goal_field(robot)), args.reps)
    row.update(rounds=info["rounds"], tile_jobs=info["tile_jobs"], tiles_reached=info["tiles_reached"], known_share=known_share)
    out["explored_map_single_goal"] = row
    _, finfo = e.frontiers(cap=0)
    out["explored_map_frontiers"] = {"cells": finfo["cells"], "clusters_all": finfo["clusters_all"]}
    rows_for(e, lambda owners: e.goal_field_from_frontiers(min_size=1, owners=owners)[0], "explored_map_all_frontier_cells")
    e.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
