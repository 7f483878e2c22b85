"""Developer tool: time-boxed random parity run of the message-side kernels against the oracle: toOccupancyGrid /
fromOccupancyGrid (random geometry, layer contents incl. NaN / out-of-range / +-inf, data ranges, moved buffers),
LaserScan -> rays (batches of scans that differ in beam count and increment, either side of the 0.017 rad decimation threshold,
at offsets with gaps, ranges at and beyond range_min / range_max, NaN / inf returns; host and device forms), every end point
held to the accepted-value rule of tests/_scan_reference.py.  usage: python scripts/fuzz_msgs.py [seconds] [seed]"""
import ctypes as C
import math
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
import _scan_reference as SR  # noqa: E402
from _gpu import SENTINEL, device_libm_error, scan_device_form  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
torch.zeros(1, device="cuda")
rng = np.random.default_rng(seed)
t_end = time.time() + budget
cases = cells = nrays = inexact = two_valued = device_forms = 0
K, worst = 2, 0.0    # K_device: 1 ulp of margin over the measured error of the device libm, raised where a batch measures more
while time.time() < t_end:
    res = float(rng.choice([0.05, 0.1, 0.2, 0.025]))
    lx, ly = float(rng.uniform(2, 20)), float(rng.uniform(2, 20))
    px, py = float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5))
    here = dict(res=res, lx=lx, ly=ly, px=px, py=py, fuzz_seed=seed, case=cases)
    e = R.Engine(lx, ly, res, px, py)
    g = O.make_geom(lx, ly, res, px, py)
    layer = rng.choice(np.array([np.nan, 0, 10, 50, 99.5, 100, 150, 180, 254.9, 255, 256, -0.5, -3, 1e9, np.inf, -np.inf], np.float32), e.ncell)
    noise = rng.random(e.ncell) < 0.3
    layer[noise] = rng.uniform(-10, 300, int(noise.sum())).astype(np.float32)
    for l in range(3):
        e.upload(l, layer)
    ref = layer.copy()
    if rng.random() < 0.5:
        target = (px + float(rng.uniform(-0.4, 0.4)) * lx, py + float(rng.uniform(-0.4, 0.4)) * ly)
        ptrs = (C.POINTER(C.c_float) * 1)(O.fptr(ref))
        regs = (O.Region * 4)()
        mv = C.c_int(0)
        O.lib().og_move(C.byref(g), ptrs, 1, O.d2(*target), regs, C.byref(mv))
        e.move(*target)
        here["moved"] = target
    for dmin, dmax in ((0.0, 255.0), (-1.0, 100.0), (float(rng.uniform(-5, 50)), float(rng.uniform(60, 300)))):
        want = O.to_occupancy_grid(g, ref, dmin, dmax)
        got = e.to_occupancy_grid(R.capi.LAYER_LASER, dmin, dmax)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            print("MISMATCH to_occupancy", here, dmin, dmax, bad[:5], got[bad[:5]], want[bad[:5]])
            sys.exit(1)
    cells += e.ncell
    if "moved" not in here:
        data = rng.integers(-1, 101, e.ncell).astype(np.int8)
        data[rng.random(e.ncell) < 0.02] = rng.integers(-128, 128, 1).astype(np.int8)[0]
        e.from_occupancy_grid(R.capi.LAYER_RANGE, data)
        got, want = e.download(R.capi.LAYER_RANGE), O.from_occupancy_grid(e.rows, e.cols, data)
        if not (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])):
            print("MISMATCH from_occupancy", here)
            sys.exit(1)
    # laser scans: a batch of scans that differ in beam count and increment, their ranges at offsets with gaps and out of scan
    # order; both pose forms; for half of the cases through the device form with a segment stride of its own
    ns = int(rng.integers(1, 7))
    for form, make in (("planar", R.synth.laser_scans), ("tf", R.synth.laser_scans_tf)):
        parts, at = [], int(rng.integers(0, 9))
        kw = dict(tilt=float(rng.choice([0.05, 0.35, 1.2])), planar=float(rng.choice([0.0, 0.25, 1.0]))) if form == "tf" else {}
        for k in rng.permutation(ns):
            beams = int(rng.choice([0, 1, 2, 37, 181, 257, 361, 1081, 2500]))
            inc = np.float32(rng.choice([0.0005, 0.004, 0.0169, 0.017, 0.0171, 0.05, 1.5 * np.pi / max(beams, 1)]))
            if beams > 400 and not inc < 0.017:
                beams = 400                           # the reference's mpmath calls are what a beam costs
            sc, r = make(1, beams, lx, ly, seed=int(rng.integers(0, 1 << 30)), angle_increment=inc, **kw)
            r[rng.random(len(r)) < 0.05] = np.float32(rng.choice([np.nan, np.inf, 0.0, -1.0]))
            u = rng.random(len(r))
            r[u < 0.05] = sc["range_max"][0]
            r[(u > 0.05) & (u < 0.1)] = sc["range_min"][0]
            sc["ranges_offset"] = at
            parts.append((int(k), sc, r, at))
            at += beams + int(rng.integers(0, 50))
        ranges = np.full(at + 1, 3.25, np.float32)
        for _, _, r, off in parts:
            ranges[off:off + len(r)] = r
        scans = np.concatenate([sc for _, sc, _, _ in sorted(parts, key=lambda p: p[0])])
        here_s = dict(form=form, n_ranges=scans["n_ranges"].tolist(), inc=[float(v) for v in scans["angle_increment"]])
        if rng.random() < 0.5:
            total, stride = int(scans["n_ranges"].sum()) + 1, int(rng.integers(max(1, int(scans["n_ranges"].max())), 8193))
            n, raw = scan_device_form(e, form, scans, ranges, stride, total)
            got = raw[:min(n, total) * 40].view(R.capi.RAY_DTYPE).copy()
            here_s["device_stride"] = stride
            if n > total or not (raw[n * 40:] == SENTINEL).all():
                print("MISMATCH scan_to_rays device form", here, here_s, n)
                sys.exit(1)
            device_forms += 1
        else:
            got = (e.scan_to_rays if form == "planar" else e.scan_to_rays_tf)(scans, ranges)
        # the shared accepted-set rule (tests/_scan_reference.py); K from the device libm's error over this batch's own arguments
        while True:
            libm = SR.Libm(K)
            ref = SR.Batch(form, scans, ranges, libm)
            err = device_libm_error({fn: sorted(a) for fn, a in libm.asked.items()})
            worst = max([worst] + list(err.values()))
            need = math.ceil(max(list(err.values()) + [0.0])) + 1
            if need <= K:
                break
            K = need
        bad = ref.frame_mismatch(got)
        out = ref.outside(got) if bad is None else []
        if K > 4 or bad is not None or len(out):
            print("MISMATCH scan_to_rays", here, here_s, dict(K=K, libm_error=err), bad, len(got), ref.n, out[:5], got[out[:5]])
            sys.exit(1)
        want = (O.scan_to_rays if form == "planar" else O.scan_to_rays_tf)(scans, ranges)
        nrays += ref.n
        inexact += int(((got["ex"] != want["ex"]) | (got["ey"] != want["ey"])).sum())
        two_valued += ref.multi_valued()
    cases += 1
    e.close()
print("msgs fuzz ok: %d maps, %d cells converted, %d rays from scans (%d batches through the device form; every end point an accepted "
      "value with K = %d, device libm within %.3f ulp; %d end points differ from glibc's, %d beams had two accepted values) in %.0f s, seed %d"
      % (cases, cells, nrays, device_forms, K, worst, inexact, two_valued, budget, seed))
