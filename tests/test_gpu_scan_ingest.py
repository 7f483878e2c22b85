"""Laser ingestion on the GPU (scan.hip) held to the independent reference of tests/_scan_reference.py on the cases of
tests/_scan_cases.py: mixed batches (decimated next to undecimated scans, empty and dead scans, one beam, the 8192-beam cap,
offsets with gaps and out of order), the values at the edges of the range filter, the clear_end index quirk, planar poses and
full transforms at their branch points.  Counts, order, origins and clear_end are exact; every ex / ey has to be one of the
float32 values the reference accepts with K_device -- no tolerance, no percentage.

K_device is MEASURED: the largest error in ulps of torch.cos / sin / acos on float64 device tensors (the device math library,
not the kernel under test) against mpmath over exactly the arguments the cases ask for, rounded up, plus 1 ulp of margin because
torch ships its own build of that library.  Above 4 it is a finding, not a value to adopt.

The device forms (rna_scan_to_rays_device / _tf_device), which no other test runs: same bytes as the host forms whatever the
segment stride, truncation that leaves the required count and writes nothing past max_rays, n_scans = 0, the RNA_EINVAL rows,
and the chain scans -> rays -> map update without a host round trip."""
import math

import numpy as np
import pytest
import torch

import _oracle as O
import _scan_cases as SC
import _scan_reference as SR
from _gpu import SENTINEL, R, dev, device_libm_error, same_f32, scan_device_form  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu
CASES = [c[0] for c in SC.cases()]
_k_device = None


def k_device():
    global _k_device
    if _k_device is None:
        err = device_libm_error(SC.asked_arguments())
        _k_device = (math.ceil(max(err.values())) + 1, err)
    return _k_device


def host_form(e, form, scans, ranges, **kw):
    return (e.scan_to_rays if form == SR.PLANAR else e.scan_to_rays_tf)(scans, ranges, **kw)


def test_device_libm_error_is_measured_over_the_arguments_of_the_cases():
    K, err = k_device()
    print("device libm (torch, float64), ulp error against mpmath: " + ", ".join("%s %.4f" % (fn, err[fn]) for fn in err)
          + "; K_device = %d" % K)
    assert K <= 4, (K, err)


@pytest.mark.parametrize("name", CASES)
def test_host_forms_give_accepted_values_only(R, name):
    _, form, scans, ranges = SC.case(name)
    K = k_device()[0]
    ref, _ = SC.reference(name, K)
    e = R.Engine(25.6, 25.6, 0.05)
    rays = host_form(e, form, scans, ranges)
    e.close()
    assert ref.frame_mismatch(rays) is None, ref.frame_mismatch(rays)
    out = ref.outside(rays)
    assert len(out) == 0 and ref.n > 500, (K, len(out), out[:5], rays[out[:5]])
    want = (O.scan_to_rays if form == SR.PLANAR else O.scan_to_rays_tf)(scans, ranges)
    print("%s: %d rays, %d end points differ from the oracle's (glibc), %d beams with two accepted values, K_device = %d"
          % (name, len(rays), int(((rays["ex"] != want["ex"]) | (rays["ey"] != want["ey"])).sum()), ref.multi_valued(), K))


@pytest.mark.parametrize("name", ["mixed-planar", "mixed-tf", "poses-tf"])
def test_device_forms_give_the_host_forms_bytes(R, name):
    """the caller's max_beams_per_scan is the segment stride as well as the bound: the largest n_ranges, and a larger one"""
    _, form, scans, ranges = SC.case(name)
    e = R.Engine(25.6, 25.6, 0.05)
    want = host_form(e, form, scans, ranges)
    total = int(scans["n_ranges"].sum())
    largest = int(scans["n_ranges"].max())
    for stride in sorted({largest, 8192, min(8192, largest + 37)}):
        n, raw = scan_device_form(e, form, scans, ranges, stride, total)
        assert n == len(want), (stride, n, len(want))
        assert raw[:n * 40].tobytes() == want.tobytes(), stride
        assert (raw[n * 40:] == SENTINEL).all(), stride
    e.close()


@pytest.mark.parametrize("name", ["mixed-planar", "mixed-tf"])
def test_device_forms_truncate_without_writing_past_max_rays(R, name):
    _, form, scans, ranges = SC.case(name)
    e = R.Engine(25.6, 25.6, 0.05)
    want = host_form(e, form, scans, ranges)
    largest = int(scans["n_ranges"].max())
    # cuts inside the first scan, at a scan's last ray, inside the capped scan, and nothing at all
    ends = np.cumsum(SC.reference(name, 1)[0].counts)
    for max_rays in (0, 100, int(ends[0]), int(ends[SC.CAP_SCAN]) - 1000, len(want) - 1):
        n, raw = scan_device_form(e, form, scans, ranges, largest, max_rays, room=len(want))
        assert n == len(want), (max_rays, n)                                  # the required count
        assert raw[:max_rays * 40].tobytes() == want[:max_rays].tobytes(), max_rays
        assert (raw[max_rays * 40:] == SENTINEL).all(), max_rays
    with pytest.raises(R.RnaError, match="RNA_ECAPACITY"):
        host_form(e, form, scans, ranges, max_rays=100)
    e.close()


def test_device_forms_with_no_scan_and_out_of_contract(R):
    _, form, scans, ranges = SC.case("poses-planar")
    _, _, scans_tf, _ = SC.case("poses-tf")
    e = R.Engine(25.6, 25.6, 0.05)
    for fn, sc in ((e.scan_to_rays_device, scans), (e.scan_to_rays_tf_device, scans_tf)):
        d_scans, d_ranges = dev(sc), dev(ranges)
        d_rays = torch.full((len(ranges) * 40,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_n = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        fn(d_scans.data_ptr(), 0, d_ranges.data_ptr(), 181, d_rays.data_ptr(), len(ranges), d_n.data_ptr())
        fn(None, 0, None, 181, None, 0, d_n.data_ptr())                      # no scan needs no buffer
        e.synchronize()
        assert int(d_n.cpu()[0]) == 0                                         # n_scans = 0 zeroes the count
        d_n.fill_(-7)
        torch.cuda.synchronize()
        for stride, count in ((0, d_n.data_ptr()), (-1, d_n.data_ptr()), (8193, d_n.data_ptr()), (181, None)):
            with pytest.raises(R.RnaError, match="RNA_EINVAL"):
                fn(d_scans.data_ptr(), len(sc), d_ranges.data_ptr(), stride, d_rays.data_ptr(), len(ranges), count)
        for bad in ((None, d_ranges.data_ptr(), d_rays.data_ptr()), (d_scans.data_ptr(), None, d_rays.data_ptr()),
                    (d_scans.data_ptr(), d_ranges.data_ptr(), None)):
            with pytest.raises(R.RnaError, match="RNA_EINVAL"):
                fn(bad[0], len(sc), bad[1], 181, bad[2], len(ranges), d_n.data_ptr())
        with pytest.raises(R.RnaError, match="RNA_EINVAL"):
            fn(d_scans.data_ptr(), -1, d_ranges.data_ptr(), 181, d_rays.data_ptr(), len(ranges), d_n.data_ptr())
        with pytest.raises(R.RnaError, match="RNA_EINVAL"):
            fn(d_scans.data_ptr(), len(sc), d_ranges.data_ptr(), 181, d_rays.data_ptr(), -1, d_n.data_ptr())
        e.synchronize()
        assert int(d_n.cpu()[0]) == -7 and bool((d_rays == SENTINEL).all())    # nothing out of contract was launched
    e.close()


def test_scans_to_map_on_the_device_without_a_round_trip(R):
    """rna_scan_to_rays_device, then rna_update_map_device on the same rays with no synchronize in between, twice on one engine
    (a staging buffer that is reused shows the second time): the master layer equals the oracle's HIMM fed with the host form's
    rays.  rna_himm_update_device on the range layer gives rna_himm_update's bytes."""
    _, form, scans, ranges = SC.case("mixed-planar")
    _, _, scans2, ranges2 = SC.case("poses-planar")
    e = R.Engine(32.0, 32.0, 0.05)
    g = O.make_geom(32.0, 32.0, 0.05)
    ref = np.full(e.ncell, np.nan, np.float32)
    for sc, rg in ((scans, ranges), (scans2[:7], ranges2), (scans, ranges)):
        want = host_form(e, form, sc, rg)
        assert len(want) > 1000
        d_scans, d_ranges = dev(sc), dev(rg)
        d_rays = torch.full((len(want) * 40,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        e.scan_to_rays_device(d_scans.data_ptr(), len(sc), d_ranges.data_ptr(), int(sc["n_ranges"].max()), d_rays.data_ptr(), len(want),
                              d_n.data_ptr())
        e.update_map_device(d_rays.data_ptr(), len(want), compose_mode=1)
        O.himm_update(g, ref, want.view(O.RAY_DTYPE))
        assert same_f32(e.download(R.capi.LAYER_MASTER), ref)
        assert int(d_n.cpu()[0]) == len(want) and d_rays.cpu().numpy().tobytes() == want.tobytes()
    # the range layer: device pointer against host pointer
    a, b = R.Engine(32.0, 32.0, 0.05), R.Engine(32.0, 32.0, 0.05)
    for _ in range(2):
        a.himm_update(R.capi.LAYER_RANGE, want)
        b.himm_update_device(R.capi.LAYER_RANGE, d_rays.data_ptr(), len(want))
        assert same_f32(a.download(R.capi.LAYER_RANGE), b.download(R.capi.LAYER_RANGE))
    for x in (e, a, b):
        x.close()

