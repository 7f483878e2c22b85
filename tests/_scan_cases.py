"""The laser-ingestion cases tests/test_scan_reference_host.py (CPU: oracle/scan.c against tests/_scan_reference.py) and
tests/test_gpu_scan_ingest.py (the kernels against it) share -- TEST INFRASTRUCTURE ONLY.  Small on purpose: what a case
costs is the mpmath side of the reference, about 19 000 surviving beams over all of them.

A case is (name, form, scans, ranges): `form` is _scan_reference.PLANAR or TF, `scans` the matching descriptor array."""
import math

import numpy as np

import _oracle as O
import _scan_reference as SR
from _scan_reference import PLANAR, TF, decimate

RANGE_MIN, RANGE_MAX = np.float32(0.1), np.float32(6.0)
FILL = np.float32(3.25)      # what lies in the gaps between the scans: a valid range, so a wrong offset shows as rays
FAN = np.float32(1.5 * np.pi)
# n_ranges, angle_increment of the mixed batch, in scan order
MIXED = ((1081, np.float32(FAN / 1081)),            # decimated: the happy path
         (0, np.float32(0.02)),                     # an empty scan between full ones
         (1, np.float32(0.02)),                     # ranges_norm = 0
         (257, np.float32(0.02)),                   # the chunk carry by one beam
         (2, np.float32(0.3)),
         (600, np.float32(0.0169)),                 # every second beam
         (64, np.float32(0.02)),                    # range_min > range_max: nothing survives
         (600, np.float32(0.017)),                  # float32(0.017) > 0.017: not decimated; holds the special range values
         (4000, np.float32(0.0005)),
         (1, np.float32(0.001)),                    # one beam through the decimation
         (8192, np.float32(0.02)),                  # the cap: 32 chunks, one of them without a valid beam
         (300, np.float32(0.02)))                   # every range invalid
EMPTY_CHUNK = 5                                     # of the 8192-beam scan
SPECIAL_SCAN, INVERTED_SCAN, DEAD_SCAN, CAP_SCAN = 7, 6, 11, 10


def _frame(dtype, rng):
    """the descriptor frame and the ranges of the mixed batch: offsets with gaps, not in scan order"""
    scans = np.zeros(len(MIXED), dtype)
    order = rng.permutation(len(MIXED))
    at, offs = 3, {}
    for k in order:
        offs[int(k)] = at
        at += MIXED[k][0] + int(rng.integers(1, 40))
    ranges = np.full(at + 5, FILL, np.float32)
    for k, (n, inc) in enumerate(MIXED):
        scans["angle_min"][k] = np.float32(-0.5 * n * float(inc)) if n * float(inc) < 6.0 else np.float32(-3.0)
        scans["angle_increment"][k] = inc
        scans["angle_max"][k] = np.float32(scans["angle_min"][k] + inc * n)
        scans["range_min"][k], scans["range_max"][k] = RANGE_MIN, RANGE_MAX
        scans["n_ranges"][k], scans["ranges_offset"][k] = n, offs[k]
        r = rng.uniform(0.12, 5.9, n).astype(np.float32)
        junk = np.array([np.nan, np.inf, -np.inf, 0.0, -1.0, 6.0, 0.01], np.float32)
        share = 0.4 if k == CAP_SCAN else 0.12
        if n >= 64:
            bad = rng.random(n) < share
            bad[(np.arange(n) % 64) == (7 * (np.arange(n) // 64)) % 64] = True      # every 64-lane wave of every chunk compacts
            r[bad] = rng.choice(junk, int(bad.sum()))
            live = (np.arange(n) % 64) == (7 * (np.arange(n) // 64) + 13) % 64      # ... and keeps a beam
            r[live] = np.float32(2.5)
        if k == CAP_SCAN:
            r[256 * EMPTY_CHUNK:256 * (EMPTY_CHUNK + 1)] = np.nan
        if k == DEAD_SCAN:
            r[:] = rng.choice(junk, n)
        if k == INVERTED_SCAN:
            scans["range_min"][k], scans["range_max"][k] = np.float32(4.0), np.float32(2.0)
        if k == SPECIAL_SCAN:     # the values at the edges of the filter, as scripts/fuzz_msgs.py plants them
            r[10:20] = [np.nan, np.inf, -np.inf, 0.0, -0.0, -2.0, RANGE_MIN, RANGE_MAX, np.nextafter(RANGE_MAX, np.float32(0)),
                        np.nextafter(RANGE_MIN, np.float32(0))]
            u = rng.random(n)
            r[(u < 0.05) & (np.arange(n) >= 20)] = RANGE_MAX
            r[(u > 0.95) & (np.arange(n) >= 20)] = RANGE_MIN
        if float(inc) < 0.017 and n > 100:
            # the clear_end quirk: +inf / range_max at ORIGINAL indices that are SIMPLIFIED indices of beams with a plain hit
            picked, _ = decimate(n, inc)
            for j, idx in enumerate((3, 5, 10, 11, 40, 41)):
                if idx in picked:
                    continue
                r[picked[idx]] = np.float32(1.5 + 0.25 * j)
                r[idx] = np.inf if j % 2 else RANGE_MAX
        ranges[offs[k]:offs[k] + n] = r
    scans["ranges_offset"][1] = offs[0] + 17        # the empty scan points into another scan's ranges
    return scans, ranges


def _quat(yaw, pitch=0.0, roll=0.0):
    from scipy.spatial.transform import Rotation
    return Rotation.from_euler("ZYX", [yaw, pitch, roll]).as_quat()


def _mixed(form):
    rng = np.random.default_rng(20)
    scans, ranges = _frame(O.SCAN_DTYPE if form == PLANAR else O.SCAN_TF_DTYPE, rng)
    for k in range(len(scans)):
        x, y, yaw = rng.uniform(-8, 8), rng.uniform(-8, 8), rng.uniform(-np.pi, np.pi)
        moving = k % 2 == 0
        dx, dy, dyaw = (rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(-0.2, 0.2)) if moving else (0.0, 0.0, 0.0)
        if form == PLANAR:
            scans[k]["x"], scans[k]["y"], scans[k]["yaw"] = x, y, yaw
            scans[k]["x_end"], scans[k]["y_end"], scans[k]["yaw_end"] = x + dx, y + dy, yaw + dyaw
        else:
            pitch, roll = rng.uniform(-0.35, 0.35, 2)
            scans[k]["t"], scans[k]["t_end"] = (x, y, 0.6), (x + dx, y + dy, 0.6 + dx)
            scans[k]["q"] = _quat(yaw, pitch, roll)
            scans[k]["q_end"] = _quat(yaw + dyaw, pitch + 0.1 * dyaw, roll - 0.1 * dyaw) * (-1.0 if k % 4 == 0 else 1.0)
    return scans, ranges


def _pose_frame(dtype, n_scans, rng, beams=181):
    """n_scans plain scans of 181 beams, 0.02 rad apart (the last one 0.004 rad: decimated), every tenth range invalid"""
    scans = np.zeros(n_scans, dtype)
    ranges = rng.uniform(0.12, 5.9, n_scans * beams).astype(np.float32)
    ranges[::10] = np.inf
    scans["angle_increment"] = np.float32(0.02)
    scans["angle_increment"][-1] = np.float32(0.004)
    scans["angle_min"] = np.float32(-1.8)
    scans["angle_max"] = np.float32(1.8)
    scans["range_min"], scans["range_max"] = RANGE_MIN, RANGE_MAX
    scans["n_ranges"] = beams
    scans["ranges_offset"] = np.arange(n_scans) * beams
    return scans, ranges


def _planar_poses():
    """start and end pose of every scan"""
    return [((1.0, -2.0, 0.7), (1.0, -2.0, 0.7)),                     # resting
            ((1.0, -2.0, 0.7), (1.04, -2.03, 0.85)),                  # moving
            ((0.5, 0.5, 3.1), (0.55, 0.5, -3.1)),                     # across +pi
            ((0.5, 0.5, -3.1), (0.55, 0.5, 3.1)),                     # across -pi
            ((-3.0, 2.0, 0.0), (-3.0, 2.0, math.pi)),                 # difference exactly pi
            ((-3.0, 2.0, 0.0), (-3.0, 2.0, -math.pi)),                # ... and exactly -pi
            ((2.0, 2.0, -1.0), (2.0, 2.1, 6.0)),                      # difference beyond 2 pi
            ((2000.0, -1999.5, 2.0), (2000.04, -1999.5, 2.1)),        # float32 end points lose bits out here
            ((-1234.567, 1999.9, -2.5), (-1234.567, 1999.9, -2.5)),
            ((4.0, 4.0, 1.0), (4.0, 4.02, 1.1))]                      # the decimated one


def _planar_pose_case():
    poses = _planar_poses()
    scans, ranges = _pose_frame(O.SCAN_DTYPE, len(poses), np.random.default_rng(21))
    for k, (a, b) in enumerate(poses):
        scans[k]["x"], scans[k]["y"], scans[k]["yaw"] = a
        scans[k]["x_end"], scans[k]["y_end"], scans[k]["yaw_end"] = b
    return scans, ranges


def planar_as_tf(scans):
    """planar descriptors as full transforms: rotation about z by yaw, the sensor on the ground"""
    tf = np.zeros(len(scans), O.SCAN_TF_DTYPE)
    for f in ("angle_min", "angle_max", "angle_increment", "range_min", "range_max", "n_ranges", "ranges_offset"):
        tf[f] = scans[f]
    for a, b, c, d in (("x", "y", "yaw", ""), ("x_end", "y_end", "yaw_end", "_end")):
        tf["t" + d][:, 0], tf["t" + d][:, 1] = scans[a], scans[b]
        tf["q" + d][:, 2], tf["q" + d][:, 3] = np.sin(scans[c] / 2), np.cos(scans[c] / 2)
    return tf


PLANAR_BOTH_WAYS = (0, 1, 2, 3, 7, 8, 9)     # scans of the planar pose case whose turn is the same rotation in both forms


def _tf_pose_case():
    # (no sensor sits on a map axis: where a coordinate of an end point cancels to 0 exactly, rounding noise of 1e-16 m spans
    # thousands of float32 values, and the rule has nothing to say about such a beam)
    h = math.sqrt(0.5)
    a = _quat(0.4, 0.3, -0.2)
    poses = [((1.0, 2.0, 0.5), a, (1.0, 2.0, 0.5), a),                                        # identical: the theta = 0 branch
             ((1.0, 2.0, 0.5), a, (1.03, 2.0, 0.52), _quat(0.5, 0.32, -0.22)),
             ((1.0, 2.0, 0.5), a, (1.03, 2.0, 0.52), -_quat(0.5, 0.32, -0.22)),              # end quaternion of the other sign
             ((0.7, -1.3, 0.3), (0.0, 0.0, 0.0, 1.0), (0.7, -1.2, 0.3), (0.0, 0.0, 1.0, 0.0)),  # dot product exactly 0
             ((0.7, -1.3, 0.3), (h, 0.0, 0.0, h), (0.7, -1.3, 0.3), (0.0, h, h, 0.0)),        # ... with a tilt
             ((-2.0, 1.0, 0.4), 2.0 * a, (-2.0, 1.05, 0.4), 0.5 * _quat(0.45, 0.3, -0.25)),  # scaled by 2 and by 0.5
             ((-2.0, 1.0, 0.4), 0.5 * a, (-2.0, 1.05, 0.4), -2.0 * _quat(0.45, 0.3, -0.25)),
             ((3.0, -3.0, 1.0), _quat(-2.0, 1.2, 0.0), (3.0, -3.0, 1.0), _quat(-1.9, 1.15, 0.1)),   # tilts up to 1.2 rad
             ((3.0, -3.0, 1.0), _quat(2.5, -0.2, 1.2), (3.02, -3.0, 1.0), _quat(2.6, -0.2, 1.2)),
             ((1500.0, -2000.0, 0.2), _quat(1.0, 0.1, 0.1), (1500.02, -2000.0, 0.2), _quat(1.1, 0.1, 0.1)),
             ((1.0, -2.0, 0.0), _quat(0.7), (1.04, -2.03, 0.0), _quat(0.85)),                # a planar pose as a quaternion
             ((4.0, 4.0, 0.2), _quat(1.0, 0.2, 0.0), (4.0, 4.02, 0.2), _quat(1.1, 0.2, 0.05))]   # the decimated one
    scans, ranges = _pose_frame(O.SCAN_TF_DTYPE, len(poses), np.random.default_rng(22))
    for k, (t0, q0, t1, q1) in enumerate(poses):
        scans[k]["t"], scans[k]["q"], scans[k]["t_end"], scans[k]["q_end"] = t0, q0, t1, q1
    return scans, ranges


def _jitter_case():
    from test_oracle_scan import _jittered_scans
    scans, _, ranges = _jittered_scans(n=6)
    return scans, ranges


_made = None


def cases():
    """every case, built once: a list of (name, form, scans, ranges); nobody writes to the arrays"""
    global _made
    if _made is None:
        _made = [("mixed-planar", PLANAR) + _mixed(PLANAR), ("mixed-tf", TF) + _mixed(TF),
                 ("poses-planar", PLANAR) + _planar_pose_case(), ("poses-tf", TF) + _tf_pose_case(),
                 ("jitter-tf", TF) + _jitter_case()]
        flat = _planar_pose_case()
        _made.append(("poses-planar-as-tf", TF, planar_as_tf(flat[0]), flat[1]))
        for c in _made:
            c[2].flags.writeable = False
            c[3].flags.writeable = False
    return _made


def case(name):
    return next(c for c in cases() if c[0] == name)


_batches = {}


def reference(name, K):
    """(the reference Batch of a case, the Libm that made it), computed once per K"""
    if (name, K) not in _batches:
        _, form, scans, ranges = case(name)
        libm = SR.Libm(K)
        _batches[name, K] = (SR.Batch(form, scans, ranges, libm), libm)
    return _batches[name, K]


def asked_arguments():
    """every argument the cases give to cos / sin / acos (both ends where the argument itself is in doubt): what a libm's error
    is measured over"""
    asked = {"cos": set(), "sin": set(), "acos": set()}
    for name, _, _, _ in cases():
        for fn, args in reference(name, 1)[1].asked.items():
            asked[fn] |= args
    return {fn: np.array(sorted(a)) for fn, a in asked.items()}
