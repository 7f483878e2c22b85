"""Scan matching (csrc/scanmatch.hip) on one MI355X, on the bench's map (4096 x 4096, config 3: synth.obstacles_rect) with the
scans of a fleet: 256 robots, 1081-beam scans from synth.laser_scans, R = 127, L = 3.

  (a) scan_match   rna_scan_match_device (three enqueues: clear, scores, decode) for (T, n_rot) = (8, 21) and (16, 41), without
                   and with the volume; the host form of the same call for comparison.  The same two rotation counts at T = 0
                   (one candidate: one bitmap read per staged point and thread) show what a call costs apart from the
                   candidates: fill, dilation, staging, launch
  (b) ingestion    the same run's rna_scan_to_rays_device + rna_update_map_device for the same scans (what the matched pose
                   goes into), and the replan loop's 1.57 ms pass (README.md) as a constant
  (c) floors       the window bytes at the HBM rate of DESIGN.md section 3 (8 TB/s): every workgroup's (2H + 1)^2 x 4 B of
                   master, and the same counted once per query (the n_rot workgroups of a query read the same window: L2 hits
                   if the cache holds it -- not measured); the bitmap reads of the scoring loop, read from the code: per
                   workgroup 4 wavefronts x nk x staged points wave-reads, nk = ceil((2T + 1)^2 / 256) candidate slots per
                   thread (the 16-byte reads of the staged points themselves, one per four points, are not counted), at one
                   wave-read per clock per CU and at the LDS table's clocks for the read the compiler emits at L = 3, the
                   12-byte ds_read_b96: 8 per wave-read; 256 CUs, 2.4 GHz

Every row is the whole call timed by HIP events on the engine's stream around it (us_events) and by the host's clock
(us_wall): a warm-up, then the median of --reps.  No hardware counter is collected.
One JSON object on stdout (and into --out).  Usage: python3 scripts/scan_match_rows.py [--reps 5] [--seed 6] [--out FILE]"""
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
CUS, CLOCK_HZ = 256, 2.4e9
LOOP_PASS_US = 1570.0
ROBOTS, BEAMS, RANGE_CELLS, LEVELS = 256, 1081, 127, 3
CONFIGS = ((8, 21), (16, 41), (0, 21), (0, 41))
LDS_CLOCKS_PER_WAVE_READ = 8   # ds_read_b96 (MI355X LDS table); L = 3 reads three of the four interleaved words
YAW_STEP = 0.005


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import ros_navigation_amd as R
    capi = R.capi
    n = GRID
    e = R.Engine(n * RES, n * RES, RES)
    e.upload(capi.LAYER_MASTER, R.synth.obstacles_rect(n, n))
    e.upload(capi.LAYER_LASER, e.download(capi.LAYER_MASTER))
    e.nbr_mask()
    stream = torch.cuda.ExternalStream(e._L.rna_stream(e.h), device=torch.device("cuda", 0))

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

    scans, ranges = R.synth.laser_scans(ROBOTS, BEAMS, n * RES, n * RES, seed=args.seed)
    g = e.geometry()
    out = {"grid": GRID, "resolution": RES, "reps": args.reps, "seed": args.seed, "robots": ROBOTS, "beams": BEAMS,
           "range_cells": RANGE_CELLS, "levels": LEVELS, "yaw_step": YAW_STEP, "hbm_bytes_per_s": HBM_BYTES_PER_S, "cus": CUS,
           "clock_hz": CLOCK_HZ, "loop_pass_us": LOOP_PASS_US, "lds_clocks_per_wave_read": LDS_CLOCKS_PER_WAVE_READ, "scan_match": {}}
    for T, n_rot in CONFIGS:
        queries = np.zeros(ROBOTS, capi.SCAN_MATCH_QUERY_DTYPE)
        pts, rots = [], []
        for k, s in enumerate(scans):                                   # as Engine.scan_match_poses prepares them
            r = ranges[int(s["ranges_offset"]):int(s["ranges_offset"]) + int(s["n_ranges"])].astype(np.float64)
            a = np.float64(s["angle_min"]) + np.arange(len(r)) * np.float64(s["angle_increment"])
            ok = np.isfinite(r) & (r >= s["range_min"]) & (r <= s["range_max"])
            xy = np.stack([r[ok] * np.cos(a[ok]), r[ok] * np.sin(a[ok])], axis=1)
            inside, q, q6, rot = capi.scan_match_prepare(g, xy, float(s["x"]), float(s["y"]), float(s["yaw"]), YAW_STEP, n_rot)
            assert inside
            queries[k] = q
            queries[k]["points_offset"] = sum(len(p) for p in pts)
            pts.append(q6)
            rots.append(rot)
        points, rot = np.concatenate(pts), np.stack(rots)
        S = 2 * T + 1
        d_q = torch.from_numpy(queries.view(np.int32).reshape(-1)).cuda()
        d_p, d_r = torch.from_numpy(points).cuda(), torch.from_numpy(rot).cuda()
        d_out = torch.zeros(8 * ROBOTS, dtype=torch.int32, device="cuda")
        d_vol = torch.zeros(ROBOTS * n_rot * S * S, dtype=torch.int32, device="cuda")
        row = {"max_shift": T, "n_rot": n_rot, "points": int(len(points))}
        res = {}
        row["host_form"] = timed(lambda: res.update(r=e.scan_match(queries, points, rot, RANGE_CELLS, T, LEVELS)))
        row["device_form"] = timed(lambda: e.scan_match_device(d_q.data_ptr(), ROBOTS, d_p.data_ptr(), len(points), d_r.data_ptr(), n_rot,
                                                               RANGE_CELLS, T, LEVELS, d_out.data_ptr(), None))
        dev = d_out.cpu().numpy().view(capi.SCAN_MATCH_DTYPE)
        assert dev.tobytes() == res["r"].tobytes()
        row["device_form_with_volume"] = timed(lambda: e.scan_match_device(d_q.data_ptr(), ROBOTS, d_p.data_ptr(), len(points),
                                                                           d_r.data_ptr(), n_rot, RANGE_CELLS, T, LEVELS, d_out.data_ptr(),
                                                                           d_vol.data_ptr()))
        recs = res["r"]
        H = RANGE_CELLS + 1 + T + (LEVELS - 1)
        window_bytes = (2 * H + 1) ** 2 * 4
        wave_reads = int(recs["n_used"].astype(np.int64).sum()) * n_rot * 4 * -(-(S * S) // 256)
        row.update(matched=int((recs["status"] == 0).sum()), used_points=int(recs["n_used"].sum()),
                   mean_score_over_max=float((recs["score"] / np.maximum(1, recs["score_max"])).mean()),
                   workgroups=ROBOTS * n_rot, window_bytes_per_workgroup=window_bytes,
                   floor_us_window_bytes_every_workgroup=1e6 * ROBOTS * n_rot * window_bytes / HBM_BYTES_PER_S,
                   floor_us_window_bytes_once_per_query=1e6 * ROBOTS * window_bytes / HBM_BYTES_PER_S,
                   lds_wave_reads=wave_reads, floor_us_lds_1_clock_per_wave_read=1e6 * wave_reads / (CUS * CLOCK_HZ),
                   candidate_slots_per_thread=-(-(S * S) // 256),
                   floor_us_lds_table_clocks_per_wave_read=1e6 * LDS_CLOCKS_PER_WAVE_READ * wave_reads / (CUS * CLOCK_HZ))
        row["device_over_lds_floor_table_clocks"] = row["device_form"]["us_events"] / row["floor_us_lds_table_clocks_per_wave_read"]
        row["device_over_window_floor_every_workgroup"] = row["device_form"]["us_events"] / row["floor_us_window_bytes_every_workgroup"]
        row["device_over_loop_pass"] = row["device_form"]["us_events"] / LOOP_PASS_US
        out["scan_match"]["T=%d n_rot=%d" % (T, n_rot)] = row
    # the ingestion the matched poses go into, for the same scans (last: it changes the map)
    rays = e.scan_to_rays(scans, ranges)
    d_scans = torch.from_numpy(scans.view(np.uint8).reshape(-1)).cuda()
    d_ranges = torch.from_numpy(ranges).cuda()
    d_rays = torch.zeros(len(rays) * capi.RAY_DTYPE.itemsize + 64, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")

    def ingest():
        e._check(e._L.rna_scan_to_rays_device(e.h, d_scans.data_ptr(), ROBOTS, d_ranges.data_ptr(), BEAMS, d_rays.data_ptr(), len(rays),
                                              d_n.data_ptr()))
        e.update_map_device(d_rays.data_ptr(), len(rays), 0)

    out["scan_to_rays_device + update_map_device"] = timed(ingest)
    out["scan_to_rays_device + update_map_device"]["rays"] = int(len(rays))
    assert int(d_n.cpu()[0]) == len(rays)
    e.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
