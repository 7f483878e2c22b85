"""CPU: the VFH+ tables and the device-block layout of csrc/vfh_tables.hpp (build_tables, VfhLayout), built by
tests/cpp/vfh_tables_dump.cpp without a GPU, for every parameter set of tests/_vfh_cases.py.

Tables: against the tables of an oracle instance of the same parameters (oracle/vfh.c), bit for bit.  The per-speed blocked
circles (bcr, in_circle), which the oracle evaluates per step and keeps no table of, against this file's restatement of
oracle/vfh.c build_masked_polar_histogram in float32 with libm's hypotf -- the engine's k_hypotf restates glibc's.

ONE cell differs from the oracle's table by design: the base magnitude of the centre cell (CX, CY) of an odd window.  It is a
front cell with direction -1; the reference reads laser_ranges[-2] for it, the oracle skips it when it computes the cell
magnitudes (calculate_cells_mag: `Cell_Direction < 0`) and keeps the formula's value in Cell_Base_Mag, the engine's kernel has
no such test and the table holds 0 there instead, with range index 0.

Layout: the sub-arrays of either block are disjoint, inside the block, 256-byte aligned and no smaller than the seventeen
allocations rna_vfh_init made before there was a layout."""
import ctypes as C
import ctypes.util
import functools
import subprocess

import numpy as np
import pytest

import _build as B
import _oracle as O
import _vfh_cases as V
from test_gpu_vfh_params import REFUSED

N_ROBOTS = (1, 2, 3, 7, 26, 1024)
TABLE = ("cell_dist", "cell_base_mag", "cell_dir", "range_idx", "memb", "in_circle", "min_turning_radius", "bcr")
STATE = ("last_binary", "hist", "origin", "picked", "last_picked", "blocked_radius", "last_chosen_speed", "max_speed_picked")
DTYPE = dict(cell_dist=np.float32, cell_base_mag=np.float32, cell_dir=np.float32, range_idx=np.int32, memb=np.uint32,
             in_circle=np.uint32, min_turning_radius=np.int32, bcr=np.float32)


def dump(p, n_robots=()):
    """the program's answer for parameter record p: None when refused, else (dims, {n_robots: (table_bytes, state_bytes,
    {name: (offset, bytes)})}, the table block)"""
    args = [repr(getattr(p, f)) for f, _ in O.VfhParams._fields_]
    assert len(args) == 20
    out = subprocess.run([B.cpp("vfh_tables_dump")] + args + [str(n) for n in n_robots], capture_output=True, timeout=120)
    if out.returncode == 2:
        assert out.stdout == b"refused\n"
        return None
    assert out.returncode == 0, out.stderr[-2000:]
    at = out.stdout.index(b"\nblock ") + 1
    end = out.stdout.index(b"\n", at) + 1
    block = out.stdout[end:]
    assert len(block) == int(out.stdout[at:end].split()[1])
    lines = out.stdout[:at].decode().splitlines()
    assert lines[0].split()[0] == "dims"
    dims = dict(zip("W H T CX CY YH NQ NQF NW max_speed".split(), map(int, lines[0].split()[1:])))
    layouts = {}
    for k in range(1, len(lines), 17):
        head = lines[k].split()
        assert head[0] == "layout" and len(head) == 4
        spans = {l.split()[0]: (int(l.split()[1]), int(l.split()[2])) for l in lines[k + 1:k + 17]}
        assert tuple(spans) == TABLE + STATE
        layouts[int(head[1])] = (int(head[2]), int(head[3]), spans)
    return dims, layouts, block


@functools.lru_cache(maxsize=None)
def dumped(name):
    return dump(V.params(name), N_ROBOTS)


def tables_of(name):
    """(dims, {name: the sub-array of the table block as numpy})"""
    dims, layouts, block = dumped(name)
    table_bytes, _, spans = layouts[0]
    assert len(block) == table_bytes
    return dims, {k: np.frombuffer(block, DTYPE[k], spans[k][1] // 4, spans[k][0]) for k in TABLE}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cell_bits(words, NQ):
    """rows of 32-bit words -> rows of NQ booleans, bit q & 31 of word q >> 5"""
    w = np.ascontiguousarray(words, "<u4")
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :NQ].astype(bool)


@pytest.mark.parametrize("name", V.SETS)
def test_tables_equal_the_oracles(name):
    p = V.params(name)
    d, t = tables_of(name)
    L = O.lib()
    v = O.OracleVfh(p)
    W, H, T, YH, NQ, NW = d["W"], d["H"], d["T"], d["YH"], d["NQ"], d["NW"]
    assert (W, H, T) == (p.window_diameter, V.hist_size(p), L.og_vfh_num_tables(v.h)) and H == v.H and T == V.num_tables(p)
    assert (d["CX"], d["CY"], YH, NQ, d["NQF"], NW, d["max_speed"]) == (W // 2, W // 2, (W + 1) // 2, ((W + 1) // 2 + 1) * W, (W + 1) // 2 * W,
                                                                        (NQ + 31) // 32, p.max_speed)
    # q = y W + x of the engine is x W + y of the oracle
    y, x = np.divmod(np.arange(NQ), W)
    assert y.max() == YH
    centre = np.zeros(NQ, bool)
    if W % 2:
        centre[d["CY"] * W + d["CX"]] = True          # the one cell that differs by design (module docstring)
    for key, fn in (("cell_dist", L.og_vfh_cell_dist), ("cell_base_mag", L.og_vfh_cell_base_mag), ("cell_dir", L.og_vfh_cell_direction)):
        want = np.ctypeslib.as_array(fn(v.h), (W * W,))[x * W + y]
        same = bits(t[key]) == bits(want)
        if key == "cell_base_mag":
            assert np.array_equal(same, ~centre), (key, np.flatnonzero(same == centre)[:5])
            assert np.all(bits(t[key][centre]) == 0) and np.all(want[centre] > 0)
        else:
            assert same.all(), (key, np.flatnonzero(~same)[:5])
    assert np.all(t["cell_dir"][centre] == -1.0) and np.all(t["cell_dir"][~centre & (y < YH)] >= 0)
    # the range bin of the front cells
    front = y < YH
    want_ri = np.where(centre, 0, np.rint(t["cell_dir"].astype(np.float64) * 2.0)).astype(np.int32)
    assert np.array_equal(t["range_idx"][front], want_ri[front])
    assert want_ri[front].min() >= 0 and want_ri[front].max() <= 360
    # sector membership: bit q of row (t, i) <=> sector i is in the oracle's list of cell (x, y) in table t
    assert len(t["memb"]) == T * H * NW + 16 and not t["memb"][T * H * NW:].any()
    got = cell_bits(t["memb"][:T * H * NW].reshape(T * H, NW), NQ).reshape(T, H, NQ)
    want = np.zeros((T, H, NQ), bool)
    for tb in range(T):
        for q in range(NQ):
            cnt = L.og_vfh_cell_sector_count(v.h, tb, int(x[q]), int(y[q]))
            lst = L.og_vfh_cell_sector_list(v.h, tb, int(x[q]), int(y[q]))
            want[tb, lst[:cnt], q] = True
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # Min_Turning_Radius
    mtr = np.array([L.og_vfh_min_turning_radius(v.h, s) for s in range(p.max_speed + 1)], np.int32)
    assert np.array_equal(t["min_turning_radius"], mtr)


def safety_dist(p, speed):
    """oracle/vfh.c get_safety_dist, operation by operation"""
    sd0, sd1 = np.float32(p.safety_dist_0ms), np.float32(p.safety_dist_1ms)
    val = int(np.float32(sd0 + np.float32(int(float(np.float32(np.float32(speed) * np.float32(sd1 - sd0))) / 1000.0))))
    return max(val, 0)


@pytest.mark.parametrize("name", V.SETS)
def test_blocked_circles_equal_the_oracles_test_with_libm_hypotf(name):
    """oracle/vfh.c build_masked_polar_histogram: Blocked_Circle_Radius = Min_Turning_Radius + ROBOT_RADIUS + safety distance, and a
    front cell lies in the right / left circle when hypotf(centre_x -+ x, centre_y - y) * CELL_WIDTH is below it"""
    p = V.params(name)
    d, t = tables_of(name)
    W, YH, NQ, NW, CX, CY = d["W"], d["YH"], d["NQ"], d["NW"], d["CX"], d["CY"]
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.hypotf.restype = C.c_float
    libm.hypotf.argtypes = [C.c_float, C.c_float]
    f32 = np.float32
    cw = f32(p.cell_size)
    assert len(t["bcr"]) == p.max_speed + 1 and len(t["in_circle"]) == (p.max_speed + 1) * 2 * NW
    circles = cell_bits(t["in_circle"].reshape(-1, NW), NQ).reshape(p.max_speed + 1, 2, NQ)
    assert not circles[:, :, YH * W:].any()           # only front cells are asked
    for s in sorted({0, 1, p.max_speed // 2, p.max_speed}):
        mtr = int(t["min_turning_radius"][s])         # (equal to the oracle's: test_tables_equal_the_oracles)
        radius = f32(f32(f32(mtr) + f32(p.robot_radius)) + f32(safety_dist(p, s)))
        assert bits(t["bcr"][s]) == bits(radius), s
        cxr, cxl, cy = f32(f32(CX) + f32(f32(mtr) / cw)), f32(f32(CX) - f32(f32(mtr) / cw)), f32(CY)
        for yy in range(YH):
            for xx in range(W):
                q = yy * W + xx
                dr = f32(f32(libm.hypotf(f32(cxr - f32(xx)), f32(cy - f32(yy)))) * cw)
                dl = f32(f32(libm.hypotf(f32(cxl - f32(xx)), f32(cy - f32(yy)))) * cw)
                assert (circles[s, 0, q], circles[s, 1, q]) == (dr < radius, dl < radius), (s, xx, yy)


def test_refused_parameters():
    """what rna_vfh_init refuses in tests/test_gpu_vfh_params.py, and the set they are variations of"""
    assert dump(V.params("sa8")) is not None
    for bad in REFUSED:
        p = V.params("sa8")
        for f, val in bad.items():
            setattr(p, f, val)
        assert dump(p) is None, bad


@pytest.mark.parametrize("name", V.SETS)
def test_layout_of_the_device_blocks(name):
    d, layouts, _ = dumped(name)
    speeds = d["max_speed"] + 1
    assert set(layouts) == {0} | set(N_ROBOTS)
    for n in N_ROBOTS:
        table_bytes, state_bytes, spans = layouts[n]
        # the allocations of the code before the layout, in bytes; memb with the sixteen words the kernel reads past a row's end
        was = dict(cell_dist=d["NQ"] * 4, cell_base_mag=d["NQ"] * 4, cell_dir=d["NQ"] * 4, range_idx=d["NQ"] * 4,
                   memb=(d["T"] * d["H"] * d["NW"] + 16) * 4, in_circle=speeds * 2 * d["NW"] * 4, min_turning_radius=speeds * 4, bcr=speeds * 4,
                   last_binary=n * d["H"] * 4, hist=n * d["H"] * 4, origin=n * d["H"] * 4, picked=n * 4, last_picked=n * 4,
                   blocked_radius=n * 4, last_chosen_speed=n * 4, max_speed_picked=n * 4)
        for names, total in ((TABLE, table_bytes), (STATE, state_bytes)):
            at = sorted((spans[k][0], spans[k][1], k) for k in names)
            for (off, size, k), nxt in zip(at, at[1:] + [(total, 0, "the block's end")]):
                assert off % 256 == 0 and size >= was[k] > 0, (n, k)
                assert off + size <= nxt[0], (n, k, nxt[2])
        assert {k: spans[k] for k in TABLE} == {k: layouts[0][2][k] for k in TABLE} and table_bytes == layouts[0][0]
