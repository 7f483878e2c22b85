"""An independent statement of laser ingestion (rna_scan_to_rays, rna_scan_to_rays_tf) that says which float32 values an end
point MAY take -- TEST INFRASTRUCTURE ONLY.

Written from the contract in include/rna.h (rna_laser_scan, rna_laser_scan_tf), LaserMapUpdater::simplifyLaserScan /
bufferIncomingMsg of the reference, and the published formulas the header cites: laser_geometry's projectLaser_ and
transformLaserScanToPointCloud_, tf's LinearMath (Quaternion::slerp / angleShortestPath / dot / length2,
Matrix3x3::setRotation, Transform::operator*, Vector3::setInterpolate3).  It shares no code with oracle/scan.c or the kernel.

The acceptance rule.  A value on the way to an end point is kept as the closed interval [lo, hi] of the doubles it can be:
  * IEEE operations (+ - * /, fmod, conversions) are REPLAYED on the end points of the intervals in double, round to nearest, with
    no contraction: rounding is monotone and the exact result of each of these operations over a box of arguments is extreme at
    a corner, so the replayed corners are exactly the least and the largest double the operation can give.
  * a library call (cos, sin, acos) may return any double within K ulp of the true value, which mpmath gives at 220 bits: the
    interval runs from K doubles below the true value's upper neighbour to K doubles above its lower neighbour, over both ends
    of the argument's interval (and +-1 where a turning point of sin / cos lies between them).
  * a float32 rounding maps [lo, hi] to the float32 values from f32(lo) to f32(hi): one value, or two neighbours where a
    rounding boundary lies inside the interval.  The projected point (px, py) is rounded that way first, and every one of its
    up to 2 x 2 candidates is taken through the transform as a BRANCH of its own.
The accepted set of ex (ey) is the union over the branches; a value is accepted iff it is a float32 and lies in one of them.

Defined where the cited code is not: a scan of no beam gives no ray (simplifyLaserScan reads ranges[0] of an empty vector), and a
projected scan of one beam has ratio 0 (laser_geometry divides by size - 1 = 0 there)."""
import math

import mpmath
import numpy as np

mpmath.mp.prec = 220                     # 66 digits
DECIMATE_BELOW = 0.017                   # laser_map_updater.cpp:80,135 -- a double literal, compared with a float
TWO_PI = 2.0 * math.pi
PLANAR, TF = "planar", "tf"
_MP = {"cos": mpmath.cos, "sin": mpmath.sin, "acos": mpmath.acos}
_true = {"cos": {}, "sin": {}, "acos": {}}   # argument -> (lower neighbour, upper neighbour, where the true value lies between, ulp)


def _enclose(name, x):
    """the doubles either side of the true value of name(x), and the true value's place between them in ulps"""
    hit = _true[name].get(x)
    if hit is None:
        v = _MP[name](mpmath.mpf(x))
        d = float(v)
        m = mpmath.mpf(d)
        if m == v:
            lo = hi = d
        elif m < v:
            lo, hi = d, math.nextafter(d, math.inf)
        else:
            lo, hi = math.nextafter(d, -math.inf), d
        u = hi - lo if hi != lo else math.ulp(d)
        hit = _true[name][x] = (lo, hi, float((v - mpmath.mpf(lo)) / u) if hi != lo else 0.0, u)
    return hit


def ulp_error(name, args, got):
    """largest distance, in ulps of the true value, of the doubles `got` = name(args) some library returned"""
    worst = 0.0
    for x, y in zip(np.asarray(args, np.float64).tolist(), np.asarray(got, np.float64).tolist()):
        lo, _, frac, u = _enclose(name, x)
        worst = max(worst, abs((y - lo) / u - frac))
    return worst


def _step(d, k):
    """k doubles up (k > 0) or down from d"""
    for _ in range(abs(k)):
        d = np.nextafter(d, math.copysign(math.inf, k))
    return d


class Iv:
    """the doubles a computed value can be, element-wise: lo <= value <= hi"""
    __slots__ = ("lo", "hi")

    def __init__(self, lo, hi=None):
        self.lo = np.asarray(lo, np.float64)
        self.hi = self.lo if hi is None else np.asarray(hi, np.float64)

    def __add__(a, b):
        b = _iv(b)
        return Iv(a.lo + b.lo, a.hi + b.hi)

    def __sub__(a, b):
        b = _iv(b)
        return Iv(a.lo - b.hi, a.hi - b.lo)

    def __rsub__(a, b):
        return _iv(b) - a

    def __neg__(a):
        return Iv(-a.hi, -a.lo)

    def __mul__(a, b):
        b = _iv(b)
        p = (a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi)
        return Iv(np.minimum.reduce(p), np.maximum.reduce(p))

    __rmul__ = __mul__

    def under(a, c):
        """c / a for a positive number c and an interval that does not hold 0"""
        assert c > 0 and ((a.lo > 0) | (a.hi < 0)).all()
        return Iv(c / a.hi, c / a.lo)


def _iv(x):
    return x if isinstance(x, Iv) else Iv(x)


class Libm:
    """cos / sin / acos that may return any double within K ulp of the true value; keeps the arguments it was asked for"""

    def __init__(self, K):
        self.K = int(K)
        self.asked = {"cos": set(), "sin": set(), "acos": set()}

    def _one(self, name, x):
        self.asked[name].add(x)
        lo, hi, _, _ = _enclose(name, x)
        if name == "acos" and x == 1.0:
            return 0.0, 0.0                       # exact, and the slerp branches on it
        return float(_step(hi, -self.K)), float(_step(lo, self.K))

    def __call__(self, name, a):
        a = _iv(a)
        lo, hi = np.atleast_1d(a.lo).astype(np.float64), np.atleast_1d(a.hi).astype(np.float64)
        lo, hi = np.broadcast_arrays(lo, hi)
        out_lo, out_hi = np.empty(lo.shape), np.empty(lo.shape)
        slope = {"cos": lambda t: -math.sin(t), "sin": math.cos, "acos": lambda t: -1.0}[name]
        for k, (x0, x1) in enumerate(zip(lo.ravel().tolist(), hi.ravel().tolist())):
            l0, h0 = self._one(name, x0)
            if x1 != x0:
                assert 0 < x1 - x0 < 1e-3, (name, x0, x1)
                l1, h1 = self._one(name, x1)
                l0, h0 = min(l0, l1), max(h0, h1)
                if name != "acos" and slope(x0) * slope(x1) <= 0:      # a turning point between the two
                    top = math.cos(x0) if name == "cos" else math.sin(x0)
                    l0, h0 = (l0, 1.0) if top > 0 else (-1.0, h0)
            out_lo.flat[k], out_hi.flat[k] = l0, h0
        return Iv(out_lo.reshape(a.lo.shape), out_hi.reshape(a.lo.shape))


class HostLibm:
    """numpy's own cos / sin / acos as point values: what ONE machine computes, for the deliberately wrong variants"""
    K = None

    def __call__(self, name, a):
        a = _iv(a)
        assert np.array_equal(a.lo, a.hi)
        return Iv(getattr(np, {"acos": "arccos"}.get(name, name))(a.lo))


def f32_ord(v):
    """float32 values as integers in value order (-0 and +0 share 0)"""
    i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7FFFFFFF))


def decimate(n_ranges, angle_increment):
    """simplifyLaserScan: the original index of every beam of the simplified scan, and its angle_increment"""
    inc = np.float32(angle_increment)
    if n_ranges <= 0:
        return [], np.float32(0.0)
    picked, acc, out_inc = [0], np.float32(0.0), np.float32(0.0)   # ranges[0] is pushed before the loop
    for i in range(n_ranges):
        acc = np.float32(acc + inc)
        if float(acc) >= DECIMATE_BELOW:
            out_inc, acc = acc, np.float32(0.0)
            picked.append(i)
    return picked, out_inc


def projected_beams(n_ranges, angle_increment):
    if float(np.float32(angle_increment)) < DECIMATE_BELOW:
        return len(decimate(n_ranges, angle_increment)[0])
    return max(int(n_ranges), 0)


def _dot4(a, b):
    return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]


def _planar_rows(sc, ratio, libm):
    """rows 0 and 1 of the rotation and the translation of every beam: position linearly, yaw along the shortest arc
    (rna.h: dyaw = fmod(yaw_end - yaw, 2 pi) brought into [-pi, pi], yaw_i = yaw + ratio * dyaw)"""
    turn = math.fmod(float(sc["yaw_end"]) - float(sc["yaw"]), TWO_PI)
    if turn > math.pi:
        turn -= TWO_PI
    if turn < -math.pi:
        turn += TWO_PI
    yaw = float(sc["yaw"]) + ratio * turn
    c, s = libm("cos", yaw), libm("sin", yaw)
    rest = 1.0 - ratio
    t = [Iv(rest * float(sc[a]) + ratio * float(sc[b])) for a, b in (("x", "x_end"), ("y", "y_end"))]
    return lambda x, y: ((c * x - s * y) + t[0], (s * x + c * y) + t[1])


def _tf_rows(sc, ratio, libm):
    """tf: Vector3::setInterpolate3, Quaternion::slerp over angleShortestPath, Matrix3x3::setRotation, Transform * point"""
    q0, q1 = [float(v) for v in sc["q"]], [float(v) for v in sc["q_end"]]
    rest = 1.0 - ratio
    t = [Iv(rest * float(sc["t"][k]) + ratio * float(sc["t_end"][k])) for k in (0, 1)]
    both = math.sqrt(_dot4(q0, q0) * _dot4(q1, q1))
    along = _dot4(q0, q1)
    arg = (-along if along < 0 else along) / both
    arg = min(1.0, max(-1.0, arg))                       # tfAcos clamps
    theta = (libm("acos", Iv(arg)) * 2.0) * 0.5          # angleShortestPath(q) / 2: both are exact scalings
    theta = Iv(theta.lo.reshape(()), theta.hi.reshape(()))
    if theta.lo == 0.0 and theta.hi == 0.0:
        q = [Iv(np.full(ratio.shape, v)) for v in q0]
    else:
        assert theta.lo > 0.0
        d = libm("sin", theta).under(1.0)
        s0, s1 = libm("sin", theta * rest), libm("sin", theta * ratio)
        sign = -1.0 if along < 0 else 1.0
        q = [(s0 * q0[k] + s1 * (sign * q1[k])) * d for k in range(4)]
    s = _dot4(q, q).under(2.0)
    xs, ys, zs = q[0] * s, q[1] * s, q[2] * s
    wz = q[3] * zs
    xx, xy, yy, zz = q[0] * xs, q[0] * ys, q[1] * ys, q[2] * zs
    m00, m01, m10, m11 = 1.0 - (yy + zz), xy - wz, xy + wz, 1.0 - (xx + zz)
    # the point's z is 0: the third product of each row adds +-0
    return lambda x, y: ((m00 * x + m01 * y) + t[0], (m10 * x + m11 * y) + t[1])


class ScanRays:
    """the rays of one scan: `beam` (index in the projected scan), `own_range`, sx, sy, clear_end, and for ex / ey the branches
    [n, 4, 2] of accepted float32 values as f32_ord integers (lo, hi); `point_span` = candidates of px / py less one"""

    def accepts(self, which, values):
        values = np.asarray(values, np.float64)
        v32 = values.astype(np.float32)
        o = f32_ord(v32)[:, None]
        br = self.ex if which == "ex" else self.ey
        return (v32.astype(np.float64) == values) & ((br[:, :, 0] <= o) & (o <= br[:, :, 1])).any(axis=1)

    def many_valued(self, which):
        """beams whose accepted set holds more than one value"""
        br = self.ex if which == "ex" else self.ey
        return br[:, :, 1].max(axis=1) > br[:, :, 0].min(axis=1)


def scan_rays(form, sc, ranges, libm, variant=None):
    """One scan (a record of the planar or the tf descriptor array) -> ScanRays.  `variant` states a deliberately WRONG
    projection for the tests of the rule itself: "trig32" takes the beam's cos / sin in float32, "unrounded" leaves the float32
    rounding of the projected point out."""
    n_ranges = int(sc["n_ranges"])
    r = np.asarray(ranges, np.float32)[int(sc["ranges_offset"]):int(sc["ranges_offset"]) + n_ranges]
    assert len(r) == n_ranges
    inc = np.float32(sc["angle_increment"])
    pick = np.arange(n_ranges)
    if float(inc) < DECIMATE_BELOW:
        picked, inc = decimate(n_ranges, inc)
        pick = np.asarray(picked, np.int64)
    seen = r[pick]                                   # the ranges of the scan that is projected
    n = len(seen)
    with np.errstate(invalid="ignore"):
        live = (seen.astype(np.float64) < float(np.float32(sc["range_max"]))) & (seen >= np.float32(sc["range_min"]))
    beam = np.flatnonzero(live)
    out = ScanRays()
    out.beam, out.own_range = beam, seen[beam]
    out.sx = np.full(len(beam), float(sc["x"] if form == PLANAR else sc["t"][0]))
    out.sy = np.full(len(beam), float(sc["y"] if form == PLANAR else sc["t"][1]))
    assert (beam < n_ranges).all()
    listed = r[beam]                                 # msg->ranges[index]: the SIMPLIFIED index in the ORIGINAL ranges
    out.clear_end = (np.isinf(listed) | (listed == np.float32(sc["range_max"]))).astype(np.int32)
    if not len(beam):
        out.ex = out.ey = np.zeros((0, 4, 2), np.int64)
        out.point_span = np.zeros((0, 2), np.int64)
        return out
    angle = float(np.float32(sc["angle_min"])) + beam.astype(np.float64) * float(inc)
    if variant == "trig32":
        c, s = Iv(np.cos(angle.astype(np.float32)).astype(np.float64)), Iv(np.sin(angle.astype(np.float32)).astype(np.float64))
    else:
        c, s = libm("cos", angle), libm("sin", angle)
    reach = seen[beam].astype(np.float64)
    px, py = c * reach, s * reach
    if variant == "unrounded":
        assert np.array_equal(px.lo, px.hi)
        cand_x, cand_y = (px.lo, px.hi), (py.lo, py.hi)
        out.point_span = np.zeros((len(beam), 2), np.int64)
    else:
        cand_x = (px.lo.astype(np.float32), px.hi.astype(np.float32))
        cand_y = (py.lo.astype(np.float32), py.hi.astype(np.float32))
        out.point_span = np.stack([f32_ord(cand_x[1]) - f32_ord(cand_x[0]), f32_ord(cand_y[1]) - f32_ord(cand_y[0])], axis=1)
    ratio = beam.astype(np.float64) * (1.0 / (float(n) - 1.0) if n > 1 else 0.0)
    to_map = (_planar_rows if form == PLANAR else _tf_rows)(sc, ratio, libm)
    out.ex, out.ey = np.empty((len(beam), 4, 2), np.int64), np.empty((len(beam), 4, 2), np.int64)
    for b in range(4):
        gx, gy = to_map(cand_x[b & 1].astype(np.float64), cand_y[b >> 1].astype(np.float64))
        for dst, g in ((out.ex, gx), (out.ey, gy)):
            dst[:, b, 0], dst[:, b, 1] = f32_ord(g.lo.astype(np.float32)), f32_ord(g.hi.astype(np.float32))
    return out


class Batch:
    """scan_rays of every scan of a batch, concatenated in scan order: what one rna_scan_to_rays call has to give"""

    def __init__(self, form, scans, ranges, libm, variant=None):
        self.per_scan = [scan_rays(form, sc, ranges, libm, variant) for sc in scans]
        self.counts = np.array([len(p.beam) for p in self.per_scan], np.int64)
        cat = lambda f, empty: np.concatenate([getattr(p, f) for p in self.per_scan]) if self.per_scan else empty  # noqa: E731
        self.all = ScanRays()
        for f, empty in (("beam", np.zeros(0, np.int64)), ("own_range", np.zeros(0, np.float32)), ("sx", np.zeros(0)), ("sy", np.zeros(0)),
                         ("clear_end", np.zeros(0, np.int32)), ("ex", np.zeros((0, 4, 2), np.int64)), ("ey", np.zeros((0, 4, 2), np.int64)),
                         ("point_span", np.zeros((0, 2), np.int64))):
            setattr(self.all, f, cat(f, empty))
        self.n = int(self.counts.sum())

    def frame_mismatch(self, rays):
        """None if count, order-carrying fields (sx, sy, clear_end, _pad) equal the reference's, else what differs"""
        if len(rays) != self.n:
            return "count %d, reference %d" % (len(rays), self.n)
        for f in ("sx", "sy", "clear_end"):
            if not np.array_equal(rays[f], getattr(self.all, f)):
                return f
        return "_pad" if rays["_pad"].any() else None

    def outside(self, rays):
        """indices of the rays whose ex or ey is not an accepted value"""
        return np.flatnonzero(~(self.all.accepts("ex", rays["ex"]) & self.all.accepts("ey", rays["ey"])))

    def multi_valued(self):
        """beams with more than one accepted value for either coordinate"""
        return int((self.all.many_valued("ex") | self.all.many_valued("ey")).sum())

    def widest(self):
        """the largest number of float32 values one branch accepts, and the largest number of candidates of px / py"""
        if not self.n:
            return 1, 1
        per_branch = max(int((b[:, :, 1] - b[:, :, 0]).max()) for b in (self.all.ex, self.all.ey)) + 1
        return per_branch, int(self.all.point_span.max()) + 1

