"""Information gain of view points on the GPU (rna_view_gain, csrc/viewgain.hip) against an oracle written here in plain numpy /
Python from the definition of include/rna.h: un-rotate master to map space, walk the line to each of the 8R ring cells (the
lines come from the oracle's og_line_cells_index, pinned to the reference's compiled LineIterator), stop before a cell outside
the map or outside the disc and after an opaque one, count the union.  Integers only: every record is compared for equality.

The oracle is vectorised over the rays of a view point (Want.record); a cell-by-cell walk of the same definition
(walk_record) checks it.  The maps are small (130 x 70: 3 x 2 ragged tiles) with few view points at R = 127 and many at
small R; one 300 x 280 map holds an R = 127 window wholly inside."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as O
from _gpu import Hip, R, engine_centre, make_engine, to_buffer, to_map  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu

RES = 0.05
RNA_ECAPACITY = -4
ROWS, COLS = 130, 70
RADII = (1, 15, 16, 31, 32, 63, 64, 127)       # the word edges of 2R + 1: 3, 31 | 33, 63 | 65, 127 | 129, 255 bits per bitmap row


# ---- the lines ----
_rings = {}


def ring_lines(radius):
    """[8R, R, 2]: the offsets c_1 .. c_R from the view cell of the line to each ring cell, from line((0, 0), offset).  That a
    line depends on the offset alone is asserted first, on view cells off the origin and on both sides of it."""
    if radius not in _rings:
        Rr = radius
        ring = [(a, b) for a in range(-Rr, Rr + 1) for b in range(-Rr, Rr + 1) if max(abs(a), abs(b)) == Rr]
        assert len(ring) == 8 * Rr and len(set(ring)) == 8 * Rr
        lines = np.stack([O.line_cells_index((0, 0), off)[1:] for off in ring])
        assert lines.shape == (8 * Rr, Rr, 2) and all(tuple(lines[k, -1]) == ring[k] for k in range(8 * Rr))
        step = max(1, (8 * Rr) // 61)
        for v in ((129, 69), (5, 64), (77, 3), (0, 0), (-40, 211)):
            for k in range(0, 8 * Rr, step):
                off = ring[k]
                assert np.array_equal(O.line_cells_index(v, (v[0] + off[0], v[1] + off[1]))[1:], lines[k] + np.array(v)), (v, off)
        _rings[radius] = lines
    return _rings[radius]


# ---- the oracle ----
class Want:
    """the definition's answer for the engine's present master layer and geometry"""

    def __init__(self, e, R):
        g = e.geometry()
        self.rows, self.cols, self.s0, self.s1 = e.rows, e.cols, g.start_index[0], g.start_index[1]
        m = to_map(e.download(R.capi.LAYER_MASTER), self.rows, self.cols, self.s0, self.s1)      # [j, i]
        self.unknown = np.isnan(m)
        self.occupied = ~self.unknown & (m > 0)

    def view_cell(self, c):
        """map-space (i, j) of buffer linear index c"""
        return (c % self.rows - self.s0) % self.rows, (c // self.rows - self.s1) % self.cols

    def buffer_cell(self, i, j):
        return ((j + self.s1) % self.cols) * self.rows + (i + self.s0) % self.rows

    def seen(self, vi, vj, radius, opaque):
        rows, cols = self.rows, self.cols
        L = ring_lines(radius)
        a, b = L[..., 0], L[..., 1]
        i, j = vi + a, vj + b
        inside = (i >= 0) & (i < rows) & (j >= 0) & (j < cols) & (a * a + b * b <= radius * radius)
        ic, jc = np.clip(i, 0, rows - 1), np.clip(j, 0, cols - 1)
        stop = (self.occupied | self.unknown) if opaque else self.occupied
        behind = np.zeros_like(inside)                       # an opaque cell among c_1 .. c_(t - 1)
        behind[:, 1:] = np.logical_or.accumulate(stop[jc, ic] & inside, axis=1)[:, :-1]
        ok = np.logical_and.accumulate(inside, axis=1) & ~behind
        s = np.zeros((cols, rows), bool)
        s[vj, vi] = True
        s[jc[ok], ic[ok]] = True
        return s

    def record(self, c, radius, opaque):
        """(status, unknown, visible, occupied)"""
        if c < 0 or c >= self.rows * self.cols:
            return (1, 0, 0, 0)
        vi, vj = self.view_cell(c)
        if self.occupied[vj, vi]:
            return (2, 0, 0, 0)
        s = self.seen(vi, vj, radius, opaque)
        return (0, int((s & self.unknown).sum()), int(s.sum()), int((s & self.occupied).sum()))

    def walk_record(self, c, radius, opaque):
        """the same, cell by cell as the definition's text reads"""
        if c < 0 or c >= self.rows * self.cols:
            return (1, 0, 0, 0)
        vi, vj = self.view_cell(c)
        if self.occupied[vj, vi]:
            return (2, 0, 0, 0)
        seen = {(vi, vj)}
        for a in range(-radius, radius + 1):
            for b in range(-radius, radius + 1):
                if max(abs(a), abs(b)) != radius:
                    continue
                for ci, cj in O.line_cells_index((vi, vj), (vi + a, vj + b))[1:]:
                    ci, cj = int(ci), int(cj)
                    if not (0 <= ci < self.rows and 0 <= cj < self.cols) or (ci - vi) ** 2 + (cj - vj) ** 2 > radius * radius:
                        break
                    seen.add((ci, cj))
                    if self.occupied[cj, ci] or (opaque and self.unknown[cj, ci]):
                        break
        return (0, sum(bool(self.unknown[j, i]) for i, j in seen), len(seen), sum(bool(self.occupied[j, i]) for i, j in seen))


def as_tuples(recs):
    return [tuple(int(r[f]) for f in ("status", "unknown", "visible", "occupied")) for r in recs]


def check(e, R, cells, radius, want=None):
    """both flag values compared with the oracle; gain(opaque) <= gain(transparent) per view point"""
    w = want if want is not None else Want(e, R)
    cells = [int(c) for c in cells]
    got = {}
    for opaque in (False, True):
        got[opaque] = as_tuples(e.view_gain(cells, radius, unknown_opaque=opaque))
        expect = [w.record(c, radius, opaque) for c in cells]
        assert got[opaque] == expect, [(c, g, x) for c, g, x in zip(cells, got[opaque], expect) if g != x][:5]
    for t, o in zip(got[False], got[True]):
        assert o[0] == t[0] and o[1] <= t[1] and o[2] <= t[2] and o[3] <= t[3]
    return w, got[False], got[True]


# ---- the maps ([j, i] arrays) ----
def door_map(rows=ROWS, cols=COLS):
    """known free on the left, a wall along i = 60 with a one-cell door at j = 35, everything behind it unknown"""
    m = np.full((cols, rows), np.nan, np.float32)
    m[:, :60] = 0.0
    m[:, 60] = 180.0
    m[35, 60] = 0.0
    return m


def random_map(rows, cols, density, seed, discs=6):
    rng = np.random.default_rng(seed)
    m = np.where(rng.random((cols, rows)) < density, np.float32(180.0), np.float32(0.0)).astype(np.float32)
    jj, ii = np.mgrid[0:cols, 0:rows]
    for _ in range(discs):
        ci, cj, r = rng.integers(0, rows), rng.integers(0, cols), rng.integers(3, 25)
        m[(ii - ci) ** 2 + (jj - cj) ** 2 <= r * r] = np.nan
    return m


def view_cells(w, rows=ROWS, cols=COLS):
    """map-space view cells: the four corners, a cell on each edge, beside the door map's wall, inside its unknown space, an
    occupied cell if the map has one; as buffer indices, plus the two indices just outside the range"""
    at = [(0, 0), (rows - 1, 0), (0, cols - 1), (rows - 1, cols - 1), (40, 0), (40, cols - 1), (0, 30), (rows - 1, 30),
          (59, 34), (59, 35), (61, 35), (100, 50), (64, 33)]
    occ = np.argwhere(w.occupied)
    if len(occ):
        at.append((int(occ[len(occ) // 2][1]), int(occ[len(occ) // 2][0])))
    return [w.buffer_cell(i, j) for i, j in at] + [-1, rows * cols]


# ---- 1. every radius at a word edge x every map content x every kind of view cell x both flags ----
@pytest.mark.parametrize("radius", RADII)
def test_radii_contents_and_view_cells(R, radius):
    rows, cols = ROWS, COLS
    e = make_engine(R, rows, cols)
    disc_in_map = lambda vi, vj: sum(1 for a in range(-radius, radius + 1) for b in range(-radius, radius + 1)  # noqa: E731
                                     if a * a + b * b <= radius * radius and 0 <= vi + a < rows and 0 <= vj + b < cols)
    # all unknown: the gain is the in-map disc; rays that stop at unknown cells see the view cell's neighbours only
    e.upload(R.capi.LAYER_MASTER, np.full(rows * cols, np.nan, np.float32))
    w = Want(e, R)
    cells = view_cells(w)
    _, clear, opaque = check(e, R, cells, radius, w)
    for c, t, o in zip(cells, clear, opaque):
        if t[0] == 0:
            vi, vj = w.view_cell(c)
            assert t == (0, disc_in_map(vi, vj), disc_in_map(vi, vj), 0)
            near = sum(1 for a in (-1, 0, 1) for b in (-1, 0, 1)
                       if a * a + b * b <= radius * radius and 0 <= vi + a < rows and 0 <= vj + b < cols)
            assert o == (0, near, near, 0)
    assert [t[0] for t in clear[-2:]] == [1, 1] and all(t[0] == 0 for t in clear[:-2])      # an unknown view cell is evaluated
    if radius == 127:                                                                      # the window overhangs all four sides at once
        vi, vj = w.view_cell(cells[12])
        assert vi - radius < 0 and vj - radius < 0 and vi + radius >= rows and vj + radius >= cols
        assert clear[12][2] == rows * cols - sum(1 for i in range(rows) for j in range(cols)
                                                 if (i - vi) ** 2 + (j - vj) ** 2 > radius * radius)
    # all free: the same set, nothing to gain
    e.upload(R.capi.LAYER_MASTER, np.zeros(rows * cols, np.float32))
    w = Want(e, R)
    _, free_clear, free_opaque = check(e, R, cells, radius, w)
    assert free_clear == free_opaque == [(t[0], 0, t[2], 0) for t in clear]
    # half unknown behind a wall with a one-cell door
    e.upload(R.capi.LAYER_MASTER, door_map().reshape(-1))
    w = Want(e, R)
    cells = view_cells(w)
    _, clear, opaque = check(e, R, cells, radius, w)
    by_cell = dict(zip(cells, clear))
    closed, in_door, beyond = (by_cell[w.buffer_cell(i, j)] for i, j in ((59, 34), (59, 35), (61, 35)))
    assert closed[0] == in_door[0] == beyond[0] == 0 and clear[-3][0] == 2                 # (the occupied cell is on the wall)
    assert closed[3] > 0 and beyond[1] > 0
    if radius >= 15:
        assert in_door[1] > closed[1]                                                      # through the door, not through the wall
    # random occupied cells with random unknown discs
    for density, seed in ((0.05, 11), (0.30, 12)):
        e.upload(R.capi.LAYER_MASTER, random_map(rows, cols, density, seed).reshape(-1))
        w = Want(e, R)
        extra = np.random.default_rng(seed).integers(0, rows * cols, 4 if radius > 64 else 40).tolist()
        _, clear, _ = check(e, R, view_cells(w) + extra, radius, w)
        assert {t[0] for t in clear} == {0, 1, 2} and (radius < 15 or any(t[1] > 0 and t[3] > 0 for t in clear))
    e.close()


def test_the_vectorised_oracle_is_the_walk(R):
    e = make_engine(R, ROWS, COLS, random_map(ROWS, COLS, 0.05, 3).reshape(-1))
    w = Want(e, R)
    for radius in (1, 7, 33):
        for c in view_cells(w)[:6] + [64 + 33 * ROWS, 3 + 66 * ROWS]:
            for opaque in (False, True):
                assert w.record(c, radius, opaque) == w.walk_record(c, radius, opaque), (c, radius, opaque)
    e.close()


# ---- 2. a moved map: windows across the buffer's wrap in i and in j ----
def test_moved_map(R):
    rows, cols = ROWS, COLS
    e = make_engine(R, rows, cols, np.zeros(rows * cols, np.float32), pos=(1.25, -2.5))
    assert e.move(1.25 + 37 * RES, -2.5 - 22 * RES)
    g = e.geometry()
    s0, s1 = g.start_index[0], g.start_index[1]
    assert s0 != 0 and s1 != 0
    si, sj = rows - s0, cols - s1                                            # the seams lie before map column si and map row sj
    m = random_map(rows, cols, 0.08, 21)
    m[sj - 8:sj + 6, si - 6:si + 6] = 0.0                                    # view cells round the crossing of the seams
    m[sj + 3, si - 9:si + 9] = 180.0
    m[sj - 12:sj - 8, si - 4:si + 4] = np.nan
    e.upload(R.capi.LAYER_MASTER, to_buffer(m, rows, cols, s0, s1))
    w = Want(e, R)
    assert np.array_equal(w.unknown, np.isnan(m))
    at = [(si, sj), (si - 1, sj - 1), (si - 1, sj), (si, sj - 1), (si + 2, sj - 2), (si - 2, sj + 2), (0, 0), (rows - 1, cols - 1)]
    cells = [w.buffer_cell(i, j) for i, j in at]
    assert cells[0] == 0                                                     # map cell (si, sj) is buffer cell 0
    for radius in (3, 20, 64, 127):
        _, clear, _ = check(e, R, cells, radius, w)
        assert all(t[0] == 0 for t in clear)
        for (i, j), t in zip(at[:6], clear):                                 # the windows straddle both seams and see across them
            assert i - radius < si <= i + radius and j - radius < sj <= j + radius
        assert clear[0][3] > 0 and (radius < 20 or clear[0][1] > 0)
    e.close()


# ---- 3. the largest window wholly inside a map ----
def test_large_window_inside_the_map(R):
    rows, cols, radius = 300, 280, 127
    e = make_engine(R, rows, cols, random_map(rows, cols, 0.05, 31, discs=20).reshape(-1))
    w = Want(e, R)
    at = [(150, 140), (127, 127), (rows - 128, cols - 128), (160, 150)]
    assert all(i - radius >= 0 and j - radius >= 0 and i + radius < rows and j + radius < cols for i, j in at)
    at = [(i, j) for i, j in at if not w.occupied[j, i]]
    assert len(at) >= 3
    _, clear, opaque = check(e, R, [w.buffer_cell(i, j) for i, j in at], radius, w)
    assert all(t[0] == 0 and t[1] > 0 and t[3] > 0 for t in clear)
    e.upload(R.capi.LAYER_MASTER, np.zeros(rows * cols, np.float32))
    full = e.view_gain([w.buffer_cell(150, 140)], radius)[0]
    assert tuple(full) == (0, 0, sum(1 for a in range(-radius, radius + 1) for b in range(-radius, radius + 1)
                                     if a * a + b * b <= radius * radius), 0)
    e.close()


# ---- 4. batch sizes, duplicates, the _device form, the capacity rule ----
def test_batches_and_device_form(R):
    hip = Hip()
    rows, cols = ROWS, COLS
    e = make_engine(R, rows, cols, random_map(rows, cols, 0.05, 41).reshape(-1))
    w = Want(e, R)
    L, h = e._L, e.h
    assert len(e.view_gain([], 9)) == 0 and L.rna_view_gain(h, None, 0, 9, 0, None) == 0         # n == 0
    assert L.rna_view_gain_device(h, None, 0, 9, 1, None) == 0
    one = np.zeros(1, R.capi.VIEW_GAIN_DTYPE)
    cell = np.array([5], np.int32)
    assert L.rna_view_gain(h, cell.ctypes.data, 1, 128, 0, one.ctypes.data) == RNA_ECAPACITY and not one.view(np.uint8).any()
    with pytest.raises(R.capi.RnaError, match="RNA_ECAPACITY"):
        e.view_gain([5], 128)
    check(e, R, [w.buffer_cell(64, 33)], 127, w)                                                # n == 1
    rng = np.random.default_rng(5)
    base = rng.integers(-1, rows * cols + 1, 200)
    cells = np.concatenate([base, base, base[::-1]]).astype(np.int32)                           # n == 600, every cell three times
    for radius in (9, 16):
        _, clear, opaque = check(e, R, cells, radius, w)
        assert clear[:200] == clear[200:400] == clear[400:][::-1]
        d_cells, d_out = hip.upload(cells), hip.alloc(16 * len(cells))
        for flag, host in ((False, clear), (True, opaque)):
            e.view_gain_device(d_cells, len(cells), radius, d_out, unknown_opaque=flag)
            e.synchronize()
            dev = hip.download(d_out, R.capi.VIEW_GAIN_DTYPE, len(cells))
            assert dev.tobytes() == e.view_gain(cells, radius, unknown_opaque=flag).tobytes() and as_tuples(dev) == host
        hip.free(d_cells)
        hip.free(d_out)
    e.close()


# ---- 5. at the frontiers; the raw layer decides, not the robot radius ----
def test_frontier_view_gain_and_robot_radius(R):
    rows, cols = ROWS, COLS
    m = random_map(rows, cols, 0.03, 51)
    m[30:40, 20:110] = 0.0
    e = make_engine(R, rows, cols, m.reshape(-1))
    robot = 25 + 35 * rows
    assert e.goal_field(robot)["status"] == 0
    recs, info = e.frontiers(min_size=2, rank=True)
    assert len(recs) >= 1
    w = Want(e, R)
    got = e.frontier_view_gain(recs, 24)
    assert got.tobytes() == e.view_gain(recs["nearest"], 24).tobytes()
    assert as_tuples(got) == [w.record(int(c), 24, False) for c in recs["nearest"]]
    assert all(g[0] == 0 and g[1] > 0 for g in as_tuples(got))                                   # a frontier cell sees unknown cells
    pess = e.frontier_view_gain(recs, 24, unknown_opaque=True)
    assert as_tuples(pess) == [w.record(int(c), 24, True) for c in recs["nearest"]]
    cells = view_cells(w)
    before = e.view_gain(cells, 24).tobytes()
    e.astar_robot_radius(0.3)
    e.nbr_mask()
    assert e.view_gain(cells, 24).tobytes() == before
    check(e, R, cells, 24, w)
    e.close()


# ---- 6. not a snapshot: the next call sees what a map update changed ----
def test_sees_a_map_update(R):
    rows, cols = ROWS, COLS
    m = np.full((cols, rows), np.nan, np.float32)
    m[20:50, 20:70] = 0.0
    master = m.reshape(-1)
    e = make_engine(R, rows, cols, master)
    e.upload(R.capi.LAYER_LASER, master)
    e.compose_master(1)
    cells = [60 + 35 * rows, 30 + 30 * rows]
    _, old, _ = check(e, R, cells, 40)
    rs = np.zeros(1, R.capi.RAY_DTYPE)
    rs["sx"][0], rs["sy"][0] = engine_centre(e, 60 + 35 * rows)                     # from the known space out into the unknown
    rs["ex"][0], rs["ey"][0] = engine_centre(e, 90 + 35 * rows)
    e.update_map(rs, compose_mode=0)
    got = as_tuples(e.view_gain(cells, 40))                                         # (no download in between)
    w, new, _ = check(e, R, cells, 40)
    assert got == new and new != old
    assert w.unknown.sum() < np.isnan(master).sum() and new[0][1] < old[0][1]       # the ray made unknown cells known
    e.close()


# ---- 7. the fuzzer, briefly ----
def test_fuzzer_runs(R):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, os.path.join(root, "scripts", "fuzz_view_gain.py"), "5", "3"], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0 and "fuzz_view_gain ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
