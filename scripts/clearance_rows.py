"""The clearance field (csrc/clearance.hip) and the goal field's clearance cost on one MI355X, on the bench's map
(4096 x 4096, config 3):

  clearance    rna_clearance_build for R = 6, 20 and 63 on the point robot's blocked set, and R = 20 on the blocked set of a
               0.3 m robot (the footprint's bits), masks in place: the whole call, launch + kernel + the wait for it, by HIP
               events on the engine's stream around it (call_us_events) and by the host's clock (call_us_wall), a warm-up,
               then the median of --reps; next to them the footprint kernel's figures for the same R from
               profiles/footprint_rows.json (an earlier session, kernel time by the engine's event brackets).  The kernel's
               own time comes from a profiler trace of `--clearance-only` (rocprofv3 --kernel-trace, a run of its own):
               1 + --reps dispatches per row, in the order of the rows
  goal_field   host wall time of rna_goal_field_build for four goals from synth.astar_queries: with an R = 20
               inflation_cost_table (0.05 m cells, inscribed 0.15 m, inflation radius 1.0 m, factor 3, scale 2000) -- the
               clearance field is in place, as in a replan loop that rebuilds after a goal change -- and once more with a
               map update before every build, so that the build has to refresh the clearance field too
  plain        the table-free build in fresh processes, --rounds times alternating between --parent-lib (a librna.so built
               from the parent commit, next to librna.so) and this tree's library: every single build time is kept, and the
               branch's medians are compared with the spread of the parent's own medians

One JSON object on stdout (and into --out).  Usage: python3 scripts/clearance_rows.py [--reps 5] [--parent-lib NAME] [--out FILE]"""
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
GRID, RES = 4096, 0.05


def plain_child(lib_name, reps):
    """table-free builds through a minimal binding of its own (the parent's library lacks the new symbols)"""
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
    print("PLAIN " + json.dumps(out))


def med(ms):
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child-plain", default=None)
    ap.add_argument("--clearance-only", action="store_true", help="only the clearance builds (for a profiler trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child_plain:
        return plain_child(args.child_plain, args.reps)
    out = {"grid": GRID, "resolution": RES, "reps": args.reps}
    # plain builds first, in processes of their own (one at a time)
    libs = (["parent"] if args.parent_lib else []) + ["branch"]
    plain = {k: [] for k in libs}
    for _ in range(0 if args.clearance_only else args.rounds):
        for k in libs:
            name = args.parent_lib if k == "parent" else "librna.so"
            txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-plain", name, "--reps", str(args.reps)], check=True,
                                 capture_output=True, text=True, timeout=600).stdout
            plain[k].append(json.loads(next(l for l in txt.splitlines() if l.startswith("PLAIN "))[6:]))
    out["plain"] = plain
    verdict = {}
    for goal in (plain["branch"][0] if plain["branch"] else []):
        b = [r[goal]["median"] for r in plain["branch"]]
        row = {"branch_medians_ms": b}
        if args.parent_lib:
            p = [r[goal]["median"] for r in plain["parent"]]
            every = [t for r in plain["parent"] for t in r[goal]["ms"]]
            row.update({"parent_medians_ms": p, "parent_every_build_ms": [min(every), max(every)],
                        "branch_inside_parent_spread": min(every) <= statistics.median(b) <= max(every)})
        verdict[goal] = row
    out["plain_summary"] = verdict

    import torch
    import ros_navigation_amd as R
    n = GRID
    e = R.Engine(n * RES, n * RES, RES)
    master = R.synth.obstacles_rect(n, n)
    e.upload(R.capi.LAYER_MASTER, master)
    e.upload(R.capi.LAYER_LASER, master)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(e._L.rna_stream(e.h), device=dev)
    try:
        fp = json.load(open(os.path.join(ROOT, "profiles", "footprint_rows.json")))["rebuild_us"]
    except OSError:
        fp = {}
    out["clearance"] = {}
    for radius, caps in ((0.0, (6, 20, 63)), (0.3, (20,))):
        e.astar_robot_radius(radius)
        e.nbr_mask()                                     # masks (and the footprint's bits) in place: the build is the kernel alone
        for cap in caps:
            e.clearance(cap)
            ev, wall = [], []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                t0 = time.perf_counter()
                e._check(e._L.rna_clearance_build(e.h, cap))
                wall.append(1e6 * (time.perf_counter() - t0))
                b.record(stream)
                b.synchronize()
                ev.append(1000.0 * a.elapsed_time(b))
            clr = e.clearance_download()
            out["clearance"]["r=%g R=%d" % (radius, cap)] = {
                "call_us_events": statistics.median(ev), "call_us_events_min": min(ev), "call_us_events_max": max(ev),
                "call_us_wall": statistics.median(wall),
                "none_share": float((clr == R.capi.CLEARANCE_NONE).mean()), "blocked_share": float((clr == 0).mean()),
                "footprint_kernel_us_same_R": fp.get("R=%d" % cap, {}).get("us")}
    if args.clearance_only:
        e.close()
        print(json.dumps(out["clearance"], indent=1))
        return
    e.astar_robot_radius(0.0)
    table = R.capi.inflation_cost_table(RES, 0.15, 1.0, 3.0, 2000.0)
    out["table"] = [int(v) for v in table]
    q = R.synth.astar_queries(4096, master, n, n)
    rays = R.synth.rays(8, 200, n * RES, n * RES, seed=4, lmax=4.0, margin=4.5)
    out["goal_field"] = []
    for goal in [int(g) for g in q["goal"][:4]]:
        row = {"goal": goal}
        for name, tab, update in (("plain", [], False), ("cost_R20", table, False), ("cost_R20_after_map_update", table, True)):
            e.goal_field_clearance_cost(tab)
            info = e.goal_field(goal)
            ms = []
            for _ in range(args.reps):
                if update:
                    e.update_map(rays, compose_mode=0)
                    e.synchronize_map()
                t0 = time.perf_counter()
                info = e.goal_field(goal)
                ms.append(1000.0 * (time.perf_counter() - t0))
            row[name] = dict(med(ms), rounds=info["rounds"], tile_jobs=info["tile_jobs"], tiles_reached=info["tiles_reached"],
                             reached=info["reached"], max_cost=info["max_cost"])
        out["goal_field"].append(row)
    e.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
