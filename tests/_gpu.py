"""Helpers the GPU tests (and the fuzzers of scripts/) share: the engine fixture, device buffers through the HIP runtime,
the change between buffer order and map order of a moved map, bitwise float comparison, engine construction and the
constants of include/rna.h that more than one test module names (test infrastructure; tests/test_support_host.py checks the
ones a wrong answer of which would let a parity test compare in the wrong space).

Feature oracles and map generators stay in the test module of their feature."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O

NONE = 0xFFFF                        # RNA_CLEARANCE_NONE
UNREACHED = 0x7fffffff               # RNA_GOAL_FIELD_UNREACHED
# the neighbours of a cell in the contract's order, and the cost of the step to each
NB_DI = (-1, 0, 1, -1, 1, -1, 0, 1)
NB_DJ = (-1, -1, -1, 0, 0, 1, 1, 1)
NB_W = (1414, 1000, 1414, 1000, 1000, 1414, 1000, 1414)
TABLE = np.array([0, 5000, 4000, 3000, 2000, 1200, 600, 300], np.uint16)   # a clearance cost, R = 7


def load():
    import ros_navigation_amd as R
    R.capi.lib()  # fails loudly when librna.so is missing -- there is no fallback
    return R


@pytest.fixture(scope="module")
def R():
    """the package with librna.so loaded; a test module takes it with `from _gpu import R  # noqa: F401`"""
    return load()


class Hip:
    """device buffers for the *_device entry points, through the HIP runtime librna.so itself links"""

    def __init__(self):
        self.h = C.CDLL("libamdhip64.so")
        self.h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.h.hipFree.argtypes = [C.c_void_p]
        self.h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]

    def alloc(self, nbytes, zero=False):
        p = C.c_void_p()
        assert self.h.hipMalloc(C.byref(p), nbytes) == 0
        if zero:
            assert self.h.hipMemset(p, 0, nbytes) == 0
        return p.value

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        assert self.h.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p

    def download(self, p, dtype, count):
        out = np.empty(count, dtype)
        assert self.h.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
        return out

    def free(self, p):
        self.h.hipFree(p)


# ---- buffer order <-> map order: map cell (i, j) sits at buffer ((i + s0) % rows, (j + s1) % cols) ----
def to_map(a, rows, cols, s0, s1):
    """buffer order -> map order, as a [j, i] array"""
    return np.roll(np.roll(a.reshape(cols, rows), -s1, axis=0), -s0, axis=1)


def to_buffer(a, rows, cols, s0, s1):
    return np.ascontiguousarray(np.roll(np.roll(a.reshape(cols, rows), s1, axis=0), s0, axis=1).reshape(-1))


def blocked_of(master):
    return ((~np.isnan(master)) & (master > 0)).astype(np.uint8)


def map_nbr(g, blocked):
    """og_astar_nbr_mask of a blocked set, taken in MAP space (a moved map's neighbours wrap round the buffer, not the edge)"""
    rows, cols, s0, s1 = g.size[0], g.size[1], g.start[0], g.start[1]
    b = np.ascontiguousarray(to_map(blocked, rows, cols, s0, s1).reshape(-1))
    nbr = np.zeros(rows * cols, np.uint8)
    u8 = C.POINTER(C.c_uint8)
    O.lib().og_astar_nbr_mask(b.ctypes.data_as(u8), rows, cols, nbr.ctypes.data_as(u8))
    return to_buffer(nbr, rows, cols, s0, s1)


# ---- floats, bit for bit ----
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_f32(a, b):
    """bitwise equality, all NaNs treated as equal"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


# ---- engines ----
def make_engine(R, rows, cols, master=None, pos=(0.0, 0.0), res=0.05):
    e = R.Engine(rows * res, cols * res, res, *pos)
    assert (e.rows, e.cols) == (rows, cols)
    if master is not None:
        e.upload(R.capi.LAYER_MASTER, master)
    return e


def make_engine_and_geom(R, rows, cols, master, pos=(0.0, 0.0), res=0.05):
    """the engine and the oracle's geometry of the same map"""
    e = R.Engine(rows * res, cols * res, res, *pos)
    g = O.make_geom(rows * res, cols * res, res, *pos)
    assert (e.rows, e.cols) == (rows, cols) == (g.size[0], g.size[1])
    e.upload(R.capi.LAYER_MASTER, master)
    return e, g


def centre(g, lin):
    """position of buffer cell `lin`, asked of the ORACLE (og_position_from_index)"""
    p = O.d2(0.0, 0.0)
    O.lib().og_position_from_index(C.byref(g), O.i2(lin % g.size[0], lin // g.size[0]), p)
    return p[0], p[1]


def engine_centre(e, lin):
    """position of buffer cell `lin`, asked of the ENGINE (rna_get_position): another source of truth than centre()"""
    return e.get_position(lin % e.rows, lin // e.rows)


# ---- laser ingestion on device buffers ----
SENTINEL = 0xA5


def dev(a):
    """a numpy array's bytes as a torch device tensor"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def scan_device_form(e, form, scans, ranges, stride, max_rays, room=None):
    """rna_scan_to_rays_device (form "planar") / rna_scan_to_rays_tf_device ("tf") on torch tensors, the count between two
    guard words: (the count the call left on the device, the whole rays buffer as bytes -- `room` rays and 64 bytes more, SENTINEL
    where nothing was written)"""
    import torch
    d_scans, d_ranges = dev(scans), dev(ranges)
    d_rays = torch.full(((max_rays if room is None else room) * O.RAY_DTYPE.itemsize + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_n = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    fn = e.scan_to_rays_device if form == "planar" else e.scan_to_rays_tf_device
    fn(d_scans.data_ptr(), len(scans), d_ranges.data_ptr(), stride, d_rays.data_ptr(), max_rays, d_n[1:].data_ptr())
    e.synchronize()
    n = d_n.cpu().numpy()
    assert n[0] == -7 and n[2] == -7
    return int(n[1]), d_rays.cpu().numpy()


def device_libm_error(asked):
    """largest error in ulps of torch.cos / sin / acos on float64 device tensors (the device math library, not a kernel of this
    project) against mpmath, over the arguments `asked` = {name: set or array of doubles}"""
    import torch
    import _scan_reference as SR
    return {fn: SR.ulp_error(fn, sorted(a), getattr(torch, fn)(torch.from_numpy(np.array(sorted(a), np.float64)).cuda()).cpu().numpy())
            for fn, a in asked.items() if len(a)}


def check_scan_rays(form, scans, ranges, rays, what=""):
    """the accepted-value rule of tests/_scan_reference.py on the rays a scan entry point gave: count, order, origins and clear_end
    equal the reference's, every ex / ey one of the float32 values it accepts with K_device = the device libm's error over THIS
    batch's arguments, rounded up, plus 1 (above 4: a finding, not a value to adopt).  Returns (the reference Batch, K_device)."""
    import math
    import _scan_reference as SR
    K = 2
    while True:
        libm = SR.Libm(K)
        ref = SR.Batch(form, scans, ranges, libm)
        err = device_libm_error(libm.asked)
        need = math.ceil(max(err.values(), default=0.0)) + 1
        assert need <= 4, (what, err)
        if need <= K:
            break
        K = need
    assert ref.frame_mismatch(rays) is None, (what, ref.frame_mismatch(rays))
    out = ref.outside(rays)
    assert len(out) == 0, (what, K, len(out), out[:5], rays[out[:5]])
    return ref, K
