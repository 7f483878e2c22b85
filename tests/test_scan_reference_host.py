"""Laser ingestion without a GPU: oracle/scan.c held to the independent reference of tests/_scan_reference.py on the cases of
tests/_scan_cases.py, the cap that keeps the acceptance rule from hiding a failure, and the rule's own teeth.

The rule (see _scan_reference): IEEE operations are replayed, cos / sin / acos may be K ulp off the value mpmath gives, and that
doubt is carried through both float32 roundings; an end point is accepted iff it is one of the float32 values that leaves.
K_host is MEASURED here: the largest error of this machine's math.cos / sin / acos over exactly the arguments the cases ask for,
rounded up, at least 1.
The cap: in every case at most 1 beam in 1000 may have more than one accepted value for either coordinate, and no branch of a
projected point may accept more than two neighbouring float32 values -- for K = 1 .. 4."""
import math

import numpy as np
import pytest

import _oracle as O
import _scan_cases as SC
import _scan_reference as SR

CASES = [c[0] for c in SC.cases()]
batch, asked_arguments = SC.reference, SC.asked_arguments


_k_host = None


def k_host():
    global _k_host
    if _k_host is None:
        args = asked_arguments()
        err = {fn: SR.ulp_error(fn, a, [getattr(math, fn)(x) for x in a.tolist()]) for fn, a in args.items()}
        _k_host = (max(1, math.ceil(max(err.values()))), err, {fn: len(a) for fn, a in args.items()})
    return _k_host


def oracle_rays(form, scans, ranges):
    return (O.scan_to_rays if form == SR.PLANAR else O.scan_to_rays_tf)(scans, ranges)


def test_host_libm_error_is_measured_over_the_arguments_of_the_cases():
    K, err, count = k_host()
    print("host libm, ulp error against mpmath: " + ", ".join("%s %.4f over %d arguments" % (fn, err[fn], count[fn]) for fn in err)
          + "; K_host = %d" % K)
    assert min(count.values()) > 10 and K <= 4


def test_the_cases_hold_what_they_promise():
    """the shapes the kernel branches on are really in the batch: decimated next to undecimated scans, empty and dead scans
    between full ones, a chunk without a valid beam, offsets out of order, the clear_end quirk, the values at the filter's edges"""
    _, _, scans, ranges = SC.case("mixed-planar")
    ref, _ = batch("mixed-planar", 1)
    n, inc, cnt = scans["n_ranges"], scans["angle_increment"], ref.counts
    assert set(n.tolist()) >= {0, 1, 2, 257, 600, 1081, 4000, 8192}
    proj = np.array([SR.projected_beams(int(a), b) for a, b in zip(n, inc)])
    assert (proj[n > 2] < n[n > 2]).any() and (proj == n).any()
    assert proj[5] == 301 and proj[7] == 600 and inc[7] == np.float32(0.017) and inc[5] < 0.017 <= float(inc[7])
    assert cnt[1] == 0 and cnt[SC.INVERTED_SCAN] == 0 and cnt[SC.DEAD_SCAN] == 0 and cnt[2] == 1 and cnt[4] == 2 and cnt[9] == 1
    assert cnt[0] > 0 and cnt[SC.CAP_SCAN] > 3000
    off = scans["ranges_offset"]
    assert (np.diff(off) < 0).any() and len(set((off % 64).tolist())) > 6
    cap = ref.per_scan[SC.CAP_SCAN].beam
    chunks = np.bincount(cap // 256, minlength=32)
    assert chunks[SC.EMPTY_CHUNK] == 0 and (np.delete(chunks, SC.EMPTY_CHUNK) > 0).all()
    waves = np.bincount(cap // 64, minlength=128)
    assert (np.delete(waves, range(4 * SC.EMPTY_CHUNK, 4 * SC.EMPTY_CHUNK + 4)) > 0).all() and (waves < 64).all()
    # a surviving beam's OWN range never sets clear_end (inf and range_max are dropped): every flag comes from the index quirk
    flags = [int(ref.per_scan[k].clear_end.sum()) for k in range(len(scans))]
    assert flags[0] >= 2 and flags[5] >= 2 and flags[8] >= 2 and flags[7] == 0 and flags[SC.CAP_SCAN] == 0
    special = ref.per_scan[SC.SPECIAL_SCAN].beam
    assert [b in special for b in range(10, 20)] == [False] * 6 + [True, False, True, False]
    assert ref.n + batch("mixed-tf", 1)[0].n < 17000
    assert sum(batch(c, 1)[0].n for c in CASES) < 21000


@pytest.mark.parametrize("name", CASES)
def test_oracle_scan_is_pinned_by_the_reference(name):
    """counts, order, origins and clear_end of oracle/scan.c equal the reference's; every ex / ey is an accepted value, K_host"""
    _, form, scans, ranges = SC.case(name)
    ref, _ = batch(name, k_host()[0])
    rays = oracle_rays(form, scans, ranges)
    assert ref.frame_mismatch(rays) is None, ref.frame_mismatch(rays)
    out = ref.outside(rays)
    assert len(out) == 0 and ref.n > 500, (len(out), out[:5], rays[out[:5]])
    per_scan = np.array([len(oracle_rays(form, scans[k:k + 1], ranges)) for k in range(len(scans))])
    assert np.array_equal(per_scan, ref.counts)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_the_cap_holds(K):
    for name in CASES:
        ref, _ = batch(name, K)
        multi, (per_branch, per_point) = ref.multi_valued(), ref.widest()
        print("K = %d, %s: %d beams, %d with more than one accepted value" % (K, name, ref.n, multi))
        assert multi * 1000 <= ref.n, (name, K, multi, ref.n)
        assert per_branch <= 2 and per_point <= 2, (name, K, per_branch, per_point)


def test_planar_poses_through_the_tf_formulation_meet_the_planar_one():
    """the two formulations round differently, but on a planar pose they describe the same point: their accepted sets share a
    value on every beam (scans that turn by exactly +-pi or by more than a turn are left out: the arc is then not the same)"""
    _, _, scans, ranges = SC.case("poses-planar")
    K = k_host()[0]
    beams = 0
    for k in SC.PLANAR_BOTH_WAYS:
        a = SR.scan_rays(SR.PLANAR, scans[k], ranges, SR.Libm(K))
        b = SR.scan_rays(SR.TF, SC.planar_as_tf(scans[k:k + 1])[0], ranges, SR.Libm(K))
        assert np.array_equal(a.beam, b.beam) and np.array_equal(a.clear_end, b.clear_end) and np.array_equal(a.sx, b.sx)
        for which in ("ex", "ey"):
            p, q = getattr(a, which), getattr(b, which)
            meet = (p[:, :, None, 0] <= q[:, None, :, 1]) & (q[:, None, :, 0] <= p[:, :, None, 1])
            assert meet.any(axis=(1, 2)).all(), (k, which, np.flatnonzero(~meet.any(axis=(1, 2)))[:5])
        beams += len(a.beam)
    assert beams > 800


# A wrong projection has to fall outside the accepted sets on a stated share of the beams.  The shares follow from magnitudes:
#  trig32     cos / sin of the beam angle in float32 are off by up to 2^-24 relative (plus the angle's own float32 rounding, up to
#             2^-24 * |angle| absolute), the float32 point has a spacing of 2^-23 relative: the point changes on roughly half of the
#             beams, and the end point with it unless the second rounding swallows it -- at least 1 beam in 5 is asked for
#  unrounded  leaving the point's rounding out moves it by up to half a float32 ulp of itself (ranges 0.1 .. 6 m); the end point,
#             of magnitude up to 8 m in these cases (spacing <= 2^-21 m), then rounds elsewhere on about |shift| / spacing of the
#             beams, some 10 % per coordinate -- at least 1 beam in 25 is asked for
@pytest.mark.parametrize("variant,least", [("trig32", 0.2), ("unrounded", 0.04)])
@pytest.mark.parametrize("name", ["mixed-planar", "mixed-tf"])
def test_a_wrong_projection_falls_outside_the_accepted_sets(name, variant, least):
    _, form, scans, ranges = SC.case(name)
    ref, _ = batch(name, k_host()[0])
    wrong = SR.Batch(form, scans, ranges, SR.HostLibm(), variant)
    right = SR.Batch(form, scans, ranges, SR.HostLibm())
    assert np.array_equal(wrong.counts, ref.counts)

    def as_rays(b):
        rays = np.zeros(b.n, O.RAY_DTYPE)
        rays["sx"], rays["sy"], rays["clear_end"] = b.all.sx, b.all.sy, b.all.clear_end
        for f in ("ex", "ey"):
            br = getattr(b.all, f)
            assert (br == br[:, :1, :1]).all()                       # point values: one branch, one value
            o = br[:, 0, 0]
            rays[f] = np.where(o >= 0, o, -o | 0x80000000).astype(np.uint32).view(np.float32).astype(np.float64)
        return rays
    assert len(ref.outside(as_rays(right))) == 0                     # numpy's libm itself is within K_host: only the variant is wrong
    share = len(ref.outside(as_rays(wrong))) / ref.n
    print("%s, %s: %.1f %% of %d beams outside the accepted sets" % (name, variant, 100 * share, ref.n))
    assert share >= least, (name, variant, share)


def test_a_decimation_threshold_taken_in_float32_is_seen():
    """float32(0.017) > 0.017: a kernel that compared with 0.017f would decimate scan 7 of the mixed batch"""
    _, _, scans, _ = SC.case("mixed-planar")
    inc = scans["angle_increment"][SC.SPECIAL_SCAN]
    assert inc == np.float32(0.017) and not float(inc) < 0.017 and SR.projected_beams(600, inc) == 600
    assert len(SR.decimate(600, inc)[0]) == 601


def test_projected_beams_equal_the_references_decimated_count():
    from ros_navigation_amd import capi
    L = capi.lib()
    seen = 0
    for _, _, scans, _ in SC.cases():
        for n, inc in zip(scans["n_ranges"].tolist(), scans["angle_increment"]):
            assert L.rna_scan_projected_beams(int(n), float(inc)) == SR.projected_beams(n, inc), (n, inc)
            seen += 1
    for n, inc in ((0, 0.001), (-3, 0.5), (8192, 0.0169), (5, -0.1), (7, 0.0), (4000, np.float32(0.017)), (33, 0.000531)):
        assert L.rna_scan_projected_beams(n, float(np.float32(inc))) == SR.projected_beams(n, inc), (n, inc)
    assert seen > 40


def test_interval_replay_gives_exactly_the_extreme_doubles():
    """the replayed corners of + - * and c / x are the least and the largest double the operation can give over the box: every
    double of two short intervals is enumerated"""
    rng = np.random.default_rng(5)
    for _ in range(300):
        a0, b0 = (float(v) for v in rng.normal(size=2) * 10.0 ** rng.integers(-3, 4, 2))
        xs = [float(SR._step(np.float64(a0), k)) for k in range(4)]
        ys = [float(SR._step(np.float64(b0), k)) for k in range(3)]
        a, b = SR.Iv(xs[0], xs[-1]), SR.Iv(ys[0], ys[-1])
        for got, op in ((a + b, lambda x, y: x + y), (a - b, lambda x, y: x - y), (a * b, lambda x, y: x * y), (3.0 - a, lambda x, y: 3.0 - x),
                        (a.under(2.0), lambda x, y: 2.0 / x), (-a, lambda x, y: -x)):
            every = [op(x, y) for x in xs for y in ys]
            assert (float(got.lo), float(got.hi)) == (min(every), max(every))


class _WideLibm(SR.Libm):
    """a libm 2^-31 relative off either way: wide enough that projected points straddle float32 rounding boundaries"""

    def _one(self, name, x):
        lo, hi = super()._one(name, x)
        return lo - abs(lo) * 2.0 ** -31, hi + abs(hi) * 2.0 ** -31


@pytest.mark.parametrize("name", ["poses-planar", "poses-tf"])
def test_a_point_with_two_candidates_is_branched_on(name):
    """none of the cases has a projected point in doubt, so the branches are exercised with a libm far worse than any real one:
    points then have two float32 candidates, every candidate is taken through the transform, and what a narrower libm accepts
    stays accepted"""
    _, form, scans, ranges = SC.case(name)
    narrow, _ = batch(name, 1)
    wide = SR.Batch(form, scans, ranges, _WideLibm(1))
    assert np.array_equal(wide.counts, narrow.counts)
    span = wide.all.point_span
    assert span.max() == 1 and 5 <= (span > 0).any(axis=1).sum() < 0.1 * wide.n
    for which in ("ex", "ey"):
        w, n = getattr(wide.all, which), getattr(narrow.all, which)
        assert (w[:, :, 0].min(axis=1) <= n[:, :, 0].min(axis=1)).all() and (w[:, :, 1].max(axis=1) >= n[:, :, 1].max(axis=1)).all()
    branched = np.flatnonzero(span[:, 0] > 0)
    assert (wide.all.ex[branched, 0, :] != wide.all.ex[branched, 1, :]).any() or (wide.all.ey[branched, 0, :] != wide.all.ey[branched, 1, :]).any()
    assert wide.multi_valued() > narrow.multi_valued()
