"""The grid A*'s robot radius (csrc/footprint.hip) on one MI355X, at the bench's size (4096 x 4096, 0.05 m):

  rebuild      a full rebuild of the blocked set and the neighbour masks for R = r / res in {0, 3, 6, 20, 63}: R = 0 is the
               point robot's nbr_mask_tiles_kernel (profile slot nbr_mask), R > 0 footprint_tiles_kernel (slot footprint)
  incremental  the refresh after one bench-sized HIMM batch (64 x 1563 = 100 032 rays) through rna_update_map(compose mode 0):
               r = 0.3 m (compose of the dirty tiles + footprint_tiles_kernel on them and their ring) against r = 0 (the fused
               compose_nbr_tiles_kernel); kernel times of the compose_master / nbr_mask / footprint slots
  astar        bench.py's map and 256-query sets (seeds 2..5) with r = 0.15 m: queries per second of synchronous batches
               (rna_astar_batch, pipeline depth 1) and the share of queries that still find a path; r = 0 alongside

Kernel times come from the engine's profile slots (a pair of hipEvents around every launch, rna_profile_enable), after a
warm-up.  One JSON object on stdout.  Usage: python3 scripts/footprint_rows.py [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def slot_ms(e, names):
    got = e.profile_get()
    return {k: got[k] for k in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--grid", type=int, default=4096)
    args = ap.parse_args()
    import ros_navigation_amd as R
    n, res = args.grid, 0.05
    length = n * res
    e = R.Engine(length, length, res)
    master0 = R.synth.obstacles_rect(n, n, density=0.30, seed=2)
    e.upload(R.capi.LAYER_LASER, master0)
    e.compose_master(1)
    ray_sets = [R.synth.rays(64, 1563, length, length, seed=4 + k) for k in range(4)]
    for rays in ray_sets:
        e.update_map(rays, compose_mode=0)
    out = {"grid": n, "resolution": res, "reps": args.reps, "rebuild_us": {}, "incremental_us": {}, "astar": {}}

    # full rebuilds: setting the radius marks every mask dirty; the download refreshes them (its copy is not in the slot)
    for Rc in (0, 3, 6, 20, 63):
        r = Rc * res
        for _ in range(3):
            e.astar_robot_radius(r)
            e.nbr_mask()
        e.profile(True)
        e.profile_reset()
        for _ in range(args.reps):
            e.astar_robot_radius(r)
            e.nbr_mask()
        s = slot_ms(e, ("nbr_mask", "footprint"))
        e.profile(False)
        slot = "nbr_mask" if Rc == 0 else "footprint"
        ms, launches = s[slot]
        out["rebuild_us"]["R=%d" % Rc] = {"slot": slot, "us": 1000.0 * ms / max(launches, 1), "launches": launches}

    # incremental refresh after one bench-sized batch
    for r in (0.0, 0.3):
        e.astar_robot_radius(r)
        e.nbr_mask()
        for k in range(4):
            e.update_map(ray_sets[k], compose_mode=0)
        e.synchronize()
        e.profile(True)
        e.profile_reset()
        for k in range(args.reps):
            e.update_map(ray_sets[k % 4], compose_mode=0)
        s = slot_ms(e, ("compose_master", "nbr_mask", "footprint"))
        e.profile(False)
        out["incremental_us"]["r=%g" % r] = {k: {"us": 1000.0 * v[0] / max(v[1], 1), "launches": v[1]} for k, v in s.items()}

    # A* on the bench's map and queries
    master = e.download(R.capi.LAYER_MASTER)
    qs = [R.synth.astar_queries(256, master, n, n, seed=2 + k) for k in range(4)]
    e.astar_pipeline_depth(1)
    e.astar_configure(max_queries=256)
    for r in (0.0, 0.15):
        e.astar_robot_radius(r)
        e.astar(qs[0], 32768)   # warm-up (and the mask rebuild)
        found = total = 0
        t0 = time.perf_counter()
        for k in range(8):
            res_, _ = e.astar(qs[k % 4], 32768)
            found += int((res_["status"] == 0).sum())
            total += len(res_)
        dt = time.perf_counter() - t0
        blocked = e.astar_blocked_mask()
        out["astar"]["r=%g" % r] = {"queries_per_s": total / dt, "found_share": found / total, "queries": total,
                                    "blocked_share": float(blocked.mean())}
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
