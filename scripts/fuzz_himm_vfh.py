"""Developer tool: time-boxed random parity run of the map-update and VFH+ kernels against the CPU oracle: random
geometry (size, resolution, map position, moved buffer), random layers, ray batches with end points snapped to cell
centres / cell edges / the map border, then compose + VFH+ steps for poses anywhere (also near and past the border), for half
of the cases at a VFH parameter set drawn from tests/_vfh_cases.py instead of the Steerer's defaults.
Layer contents, chosen speed / turn rate, both histograms and the picked angle must agree bit for bit.
usage: python scripts/fuzz_himm_vfh.py [seconds] [seed]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import ros_navigation_amd as R  # noqa: E402
import _oracle as O  # noqa: E402
import _vfh_cases as V  # noqa: E402
from _gpu import bits, same_f32  # noqa: E402


def gen_rays(rng, n, g, lx, ly, res):
    cx, cy = float(g.pos[0]), float(g.pos[1])
    r = np.zeros(n, O.RAY_DTYPE)
    r["sx"] = rng.uniform(cx - 0.7 * lx, cx + 0.7 * lx, n)
    r["sy"] = rng.uniform(cy - 0.7 * ly, cy + 0.7 * ly, n)
    th, ln = rng.uniform(-np.pi, np.pi, n), rng.uniform(0.0, 8.0, n)
    r["ex"], r["ey"] = r["sx"] + ln * np.cos(th), r["sy"] + ln * np.sin(th)
    # snapped end points: cell centres, cell edges, the map border itself
    k = rng.random(n)
    snap = k < 0.35
    for f, c, L in (("ex", cx, lx), ("ey", cy, ly)):
        v = r[f]
        edge = c - 0.5 * L
        v[snap] = edge + np.round((v[snap] - edge) / res) * res + rng.choice([0.0, 0.5 * res], int(snap.sum()))
        border = (k > 0.35) & (k < 0.45)
        v[border] = rng.choice([c - 0.5 * L, c + 0.5 * L], int(border.sum()))
        r[f] = v
    zero = rng.random(n) < 0.02
    r["ex"][zero], r["ey"][zero] = r["sx"][zero], r["sy"][zero]
    r["clear_end"] = (rng.random(n) >= 0.7).astype(np.int32)
    return r


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    rng = np.random.default_rng(seed)
    t_end = time.time() + budget
    cases = nrays = nposes = 0
    while time.time() < t_end:
        res = float(rng.choice([0.05, 0.05, 0.1, 0.2, 0.025]))
        if os.environ.get("FUZZ_RES"):
            res = float(os.environ["FUZZ_RES"])
        lx, ly = float(rng.uniform(3, 24)), float(rng.uniform(3, 24))
        px, py = (float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5))) if rng.random() < 0.5 else (0.0, 0.0)
        here = dict(res=res, lx=lx, ly=ly, px=px, py=py, fuzz_seed=seed, case=cases)
        e = R.Engine(lx, ly, res, px, py)
        g = O.make_geom(lx, ly, res, px, py)
        init = rng.choice(np.array([np.nan, 0, 10, 50, 150, 160, 170, 180, 7.5, -3, 1e3], np.float32), e.ncell)
        for l in range(3):
            e.upload(l, init)
        ref = init.copy()
        if rng.random() < float(os.environ.get("FUZZ_MOVE", "0.4")):
            target = (px + float(rng.uniform(-3, 3)), py + float(rng.uniform(-3, 3)))
            ptrs = (C.POINTER(C.c_float) * 1)(O.fptr(ref))
            regs = (O.Region * 4)()
            mv = C.c_int(0)
            O.lib().og_move(C.byref(g), ptrs, 1, O.d2(*target), regs, C.byref(mv))
            e.move(*target)
            here["moved"] = target
            if tuple(e.geometry().start_index) != tuple(g.start) or not same_f32(e.download(R.capi.LAYER_LASER), ref):
                print("MISMATCH after move", here)
                sys.exit(1)
        for b in range(int(rng.integers(1, 4))):
            n = int(rng.choice([1, 17, 400, 5000]))
            rays = gen_rays(rng, n, g, lx, ly, res)
            O.himm_update(g, ref, rays)
            e.update_map(rays.view(R.capi.RAY_DTYPE), compose_mode=int(rng.integers(0, 2)))
            nrays += n
            if not same_f32(e.download(R.capi.LAYER_LASER), ref) or not same_f32(e.download(R.capi.LAYER_MASTER), ref):
                dev = e.download(R.capi.LAYER_LASER)
                bad = np.flatnonzero(~((dev == ref) | (np.isnan(dev) & np.isnan(ref))))
                print("MISMATCH himm", here, "batch", b, "n", n, "cells", bad[:5], dev[bad[:5]], ref[bad[:5]], "of", len(bad))
                sys.exit(1)
        np_ = int(rng.integers(1, 40))
        poses = np.zeros(np_, R.capi.POSE_DTYPE)
        cx, cy = float(g.pos[0]), float(g.pos[1])
        poses["x"] = rng.uniform(cx - 0.55 * lx, cx + 0.55 * lx, np_)
        poses["y"] = rng.uniform(cy - 0.55 * ly, cy + 0.55 * ly, np_)
        poses["yaw"] = rng.uniform(-np.pi, np.pi, np_)
        poses["dt"] = 0.2
        poses["current_speed"] = rng.choice([0, 0, 200, 600], np_)
        poses["goal_direction"] = rng.uniform(0, 360, np_)
        poses["goal_distance"] = rng.choice([3000.0, 100.0, 800.0], np_)
        poses["goal_tolerance"] = 250.0
        vp = None                                  # the Steerer's own parameters, or one of the named sets
        if rng.random() < 0.5:
            here["vfh_set"] = str(rng.choice(V.NAMES))
            vp = V.params(here["vfh_set"])
            np_ = min(np_, 12)                     # (an oracle instance of the large sets allocates tens of megabytes)
            poses = poses[:np_]
        e.vfh_init(np_, V.capi_params(R, vp) if vp else None)
        oracles = [O.OracleVfh(vp) for _ in range(np_)]
        for s in range(2):
            out, origin, hist = e.vfh_step(poses)
            for k in range(np_):
                p = poses[k]
                cs, ct = oracles[k].step_pose(g, ref, p["x"], p["y"], p["yaw"], int(p["current_speed"]), p["goal_direction"],
                                              p["goal_distance"], p["goal_tolerance"], float(p["dt"]))
                ok = ((out["chosen_speed"][k], out["chosen_turnrate"][k]) == (cs, ct) and
                      bits(origin[k]).tobytes() == bits(oracles[k].origin_hist()).tobytes() and
                      bits(hist[k]).tobytes() == bits(oracles[k].hist()).tobytes() and
                      np.float32(out["picked_angle"][k]) == np.float32(oracles[k].picked_angle()))
                if not ok:
                    do, dh = bits(origin[k]) != bits(oracles[k].origin_hist()), bits(hist[k]) != bits(oracles[k].hist())
                    print("MISMATCH vfh", here, "step", s, "pose", k, p, "gpu", out[k], "oracle", cs, ct, oracles[k].picked_angle(),
                          "origin sectors", np.flatnonzero(do), origin[k][do], oracles[k].origin_hist()[do],
                          "hist sectors", np.flatnonzero(dh), hist[k][dh], oracles[k].hist()[dh])
                    sys.exit(1)
            poses["x"] += rng.uniform(-0.05, 0.05, np_)
            poses["y"] += rng.uniform(-0.05, 0.05, np_)
            poses["current_speed"] = out["chosen_speed"]
        nposes += np_
        cases += 1
        e.close()
    print("himm/vfh fuzz ok: %d maps, %d rays, %d poses in %.0f s, seed %d" % (cases, nrays, nposes, budget, seed))


if __name__ == "__main__":
    torch.zeros(1, device="cuda")
    main()
