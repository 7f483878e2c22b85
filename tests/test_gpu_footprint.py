"""GPU: the grid A* planning for a robot of radius r (rna_astar_set_robot_radius, csrc/footprint.hip) against the
reference's own GlobalPlanner::ifBlocked predicate.  The inflated reference: cell c is blocked iff some cell that the
reference's compiled CircleIterator (oracle/_ref/libref_gridmap.so; the pinned restatement og_circle_cells where that
library was not built) visits around getPosition(c) with radius r holds a master value that is not NaN and > 0.  The
A* reference is og_astar_query_on_map on a stand-in master holding 1.0 where that set is blocked and 0.0 elsewhere."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
from _gpu import Hip, R, centre, make_engine_and_geom, map_nbr  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu

REFERENCE = O.ref_gridmap() is not None
_discs = {}


def geom_key(g):
    return (tuple(g.len), tuple(g.pos), g.res, tuple(g.size), tuple(g.start))


def disc_lists(g, r):
    """per buffer cell, the in-map buffer cells CircleIterator(map, centre, r) visits: (offsets, linear indices)"""
    key = (geom_key(g), r)
    if key not in _discs:
        rows, cols = g.size[0], g.size[1]
        offs, idx = [0], []
        for lin in range(rows * cols):
            c = O.circle_cells(g, centre(g, lin), r, reference=REFERENCE)
            ok = (c[:, 0] >= 0) & (c[:, 0] < rows) & (c[:, 1] >= 0) & (c[:, 1] < cols)
            idx.append(c[ok, 0] + c[ok, 1] * rows)
            offs.append(offs[-1] + int(ok.sum()))
        _discs[key] = (np.array(offs), np.concatenate(idx).astype(np.int64))
    return _discs[key]


def ref_blocked(g, master, r):
    occ = (~np.isnan(master)) & (master > 0)
    offs, idx = disc_lists(g, r)
    hit = np.concatenate([[0], np.cumsum(occ[idx])])
    return (hit[offs[1:]] - hit[offs[:-1]] > 0).astype(np.uint8)


def sample_map(rows, cols, seed, occupied=0.004, edge=True):
    """sparse obstacles (single cells and small blocks), unknown (NaN) cells, and obstacles on every map edge"""
    rng = np.random.default_rng(seed)
    m = np.zeros((cols, rows), np.float32)
    m[rng.random((cols, rows)) < occupied] = 100.0
    for _ in range(3):
        i, j = rng.integers(0, rows - 4), rng.integers(0, cols - 4)
        m[j:j + 3, i:i + 4] = 180.0
    m[rng.random((cols, rows)) < 0.08] = np.nan
    if edge:
        m[0, rng.integers(0, rows)] = 50.0
        m[-1, rng.integers(0, rows)] = 50.0
        m[rng.integers(0, cols), 0] = 50.0
        m[rng.integers(0, cols), -1] = 50.0
        m[-1, -1] = 7.0
    return m.reshape(-1)


def move_both(R, e, g, master, target):
    ref = master.copy()
    ptrs = (C.POINTER(C.c_float) * 1)(O.fptr(ref))
    regs = (O.Region * 4)()
    mv = C.c_int(0)
    O.lib().og_move(C.byref(g), ptrs, 1, O.d2(*target), regs, C.byref(mv))
    assert e.move(*target) and tuple(e.geometry().start_index) == tuple(g.start) != (0, 0)
    return ref


def check_masks(e, g, master, r):
    want = ref_blocked(g, master, r)
    got = e.astar_blocked_mask()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, ("r=%g" % r, bad[:10], got[bad[:10]], want[bad[:10]])
    assert np.array_equal(e.nbr_mask(), map_nbr(g, want)), "r=%g" % r
    return want


SPLIT, INSIDE = "split", "inside"
LO3, HI3 = float(np.nextafter(0.3, 0.0)), float(np.nextafter(0.3, 1.0))
# rows, cols, res, position, radii, the map.  A radius given as (r, SPLIT) is a whole number R of cells (or one ulp off it) at a
# resolution whose arithmetic rounds: the reference must put offset (R, 0) inside the disc in some interior cells and outside
# in others, or the case would not tell a per-cell tie from a fixed stencil.  (r, INSIDE): res and r are exact in binary,
# every tie is an equality and (R, 0) is inside in every interior cell.  Both are asked of the reference's lists alone.
# The map: sample_map, or far_wall() of it for the 63-cell radius, under which sample_map leaves no cell of 70 x 45 free.
CASES = [
    (96, 80, 0.05, (1.25, -2.5), (0.05, 0.1, 0.25, 0.3, 0.33, 63 * 0.05), None),
    (257, 131, 0.05, (1000.3, -517.9), (0.05, 0.25, 0.3, 0.33), None),
    (257, 131, 0.05, (1.25, -2.5), (0.1,), None),
    (96, 80, 0.05, (1000.3, -517.9), (0.3, 63 * 0.05), None),
    # off 0.05 m.  0.1: ties (5, 0) / (4, 3), (3, 0), (10, 0) / (8, 6); 0.25 m = 2.5 cells; 6.3 m = 63 cells, the largest R
    (70, 45, 0.1, (1.25, -2.5), ((0.5, SPLIT), (0.3, SPLIT), (1.0, SPLIT), 0.25), None),
    (70, 45, 0.1, (1.25, -2.5), ((6.3, SPLIT),), "far wall"),
    (130, 67, 0.025, (1.25, -2.5), ((0.125, SPLIT), (0.25, SPLIT)), None),
    # (1.4 m and not 1.0 m: at x = 1000 the reference puts (5, 0) inside in all 2100 interior cells, (7, 0) in 1395 of 1736)
    (70, 45, 0.2, (1000.3, -517.9), ((0.6, SPLIT), (1.4, SPLIT)), None),
    (130, 67, 0.03, (1.25, -2.5), ((0.15, SPLIT), (0.3, SPLIT)), None),
    (70, 45, 0.07, (1000.3, -517.9), ((0.35, SPLIT),), None),
    (70, 45, 0.25, (1.25, -2.5), ((1.25, INSIDE),), None),
    (70, 45, 1.0, (0.5, 0.5), ((5.0, INSIDE),), None),
    # below a cell, k + 1/2 cells (the box corners p +- r lie on cell boundaries), one ulp either side of six cells
    (70, 45, 0.05, (1.25, -2.5), (1e-9, 0.025, 0.075, 0.125, (LO3, SPLIT), (HI3, SPLIT)), None),
    # every cell an edge cell: the plan is made for coordinates of 6e12 m, eta = 2^-48 * 6e12 = 0.021 m, 16 eta >= res, so
    # make_plan sets band = 1 << 30 and every cell asks box_is_plain.  (Cell centres lie on a grid of 2^-11 m there.)
    (70, 45, 0.05, (3.0e12, -1.0e12), ((0.3, SPLIT), 0.25), None),
]


def offset_R0_inside(g, r):
    """From the reference's disc lists alone: for every interior cell (at least R = round(r / res) cells from every edge of
    the map), whether the cell R rows on, offset (R, 0), is in its disc.  No cell of a 70 x 45 map is 63 cells from every
    edge: there the cells whose offset (R, 0) is in the map stand in."""
    rows, cols = g.size[0], g.size[1]
    R = int(round(r / g.res))
    offs, idx = disc_lists(g, r)
    cell = np.repeat(np.arange(rows * cols), np.diff(offs))
    inside = np.zeros(rows * cols, bool)
    inside[cell[idx == (cell % rows + R) % rows + cell // rows * rows]] = True
    lin = np.arange(rows * cols)
    i, j = (lin % rows - g.start[0]) % rows, (lin // rows - g.start[1]) % cols        # map space
    interior = (i >= R) & (i < rows - R) & (j >= R) & (j < cols - R)
    if not interior.any():
        interior = i < rows - R
    assert interior.any()
    return inside[interior]


def check_expectation(g, r, expect):
    inside = offset_R0_inside(g, r)
    if expect == SPLIT:
        assert 0 < inside.sum() < inside.size, ("the reference decides offset (R, 0) alike in every cell", r, int(inside.sum()))
    else:
        assert inside.all(), ("an exact tie outside the reference's disc", r, int(inside.sum()), inside.size)


def far_wall(master, rows, cols):
    """sample_map with its obstacles kept in rows 0-1 only and a wall along row 2, gaps where the cell is unknown: whether
    cell (2 + R, j) is blocked is then the reference's decision on offset (-R, 0) in that cell (the next offsets, (-R, +-1),
    are a cell outside), and the cells beyond are free"""
    m = master.reshape(cols, rows).copy()
    m[:, 2:][m[:, 2:] > 0] = 0.0
    m[:, 2][~np.isnan(m[:, 2])] = 100.0
    return m.reshape(-1)


def case_id(k, c):
    """(the four cases at 0.05 m keep the names they had before the resolution became a parameter)"""
    return "%d-%d-pos%d-radii%d" % (c[0], c[1], k, k) if k < 4 else "%d-%d-res%g-pos%d%s" % (c[0], c[1], c[2], k, "-far-wall" if c[5] else "")


@pytest.mark.parametrize("rows,cols,res,pos,radii,wall", CASES, ids=[case_id(k, c) for k, c in enumerate(CASES)])
def test_blocked_set_matches_reference_predicate(R, rows, cols, res, pos, radii, wall):
    master = sample_map(rows, cols, seed=rows + cols)
    if wall:
        master = far_wall(master, rows, cols)
    e, g = make_engine_and_geom(R, rows, cols, master, pos, res=res)
    for r in radii:
        r, expect = r if isinstance(r, tuple) else (r, None)
        if expect:
            check_expectation(g, r, expect)
        assert e.astar_robot_radius(r) == r
        blocked = check_masks(e, g, master, r)
        if (res, r) != (0.05, 63 * 0.05):           # (the two first cases of 63 cells: every cell blocked, kept as they were)
            assert 0 < blocked.sum() < blocked.size, r
    e.close()


@pytest.mark.parametrize("rows,cols,res,target,radii", [(96, 80, 0.05, (2.33, -1.61), (0.3, 0.25, 63 * 0.05)),
                                                        (70, 45, 0.1, (2.33, -1.64), ((0.5, SPLIT), (0.3, SPLIT)))])
def test_blocked_set_on_a_moved_map(R, rows, cols, res, target, radii):
    """(the second target is 10.8 and 8.6 cells of 0.1 m from (1.25, -2.5): no multiple of the resolution on either axis)"""
    master = sample_map(rows, cols, seed=5)
    e, g = make_engine_and_geom(R, rows, cols, master, (1.25, -2.5), res=res)
    first = radii[0][0] if isinstance(radii[0], tuple) else radii[0]
    e.astar_robot_radius(first)
    check_masks(e, g, master, first)
    ref = move_both(R, e, g, master, target)
    for r in radii:
        r, expect = r if isinstance(r, tuple) else (r, None)
        if expect:
            check_expectation(g, r, expect)
        e.astar_robot_radius(r)
        blocked = check_masks(e, g, ref, r)
        assert r == 63 * 0.05 or 0 < blocked.sum() < blocked.size, r
    e.close()


def test_far_move_remakes_the_stencil_plan_and_the_way_back_keeps_it(R):
    """footprint_refresh makes its plan for twice the geometry's coordinate magnitude and re-makes it when a move exceeds
    that (mag > e->fp.mag).  (1.25, -2.5) -> (40000.7, -25000.3) -> (1.4, -2.6), which is three and two cells from where it
    began so that the buffer stays a moved one.  The second comparison runs under a plan re-made for the far origin, the
    third under that same plan, made for some ten thousand times the magnitude the geometry then has (wider margins).  A
    move that far leaves only NaN, so a fresh map is written on both sides, in buffer order."""
    rows, cols, r = 70, 45, 0.3
    near, far, back = (1.25, -2.5), (40000.7, -25000.3), (1.4, -2.6)
    master = sample_map(rows, cols, seed=31)
    e, g = make_engine_and_geom(R, rows, cols, master, near)
    assert e.astar_robot_radius(r) == r
    check_masks(e, g, master, r)
    for k, target in enumerate((far, back)):
        left = move_both(R, e, g, master, target)
        assert np.isnan(left).all() and np.isnan(e.download(R.capi.LAYER_MASTER)).all()
        assert tuple(g.pos) == tuple(e.geometry().position) and abs(g.pos[0] - target[0]) < 0.05
        master = sample_map(rows, cols, seed=32 + k)          # buffer order, the same bytes on both sides
        e.upload(R.capi.LAYER_MASTER, master)
        blocked = check_masks(e, g, master, r)
        assert 0 < blocked.sum() < blocked.size
        check_expectation(g, r, SPLIT)
    e.close()


def check_search(e, g, blocked, q, res, paths, settled, moved):
    stand_in = blocked.astype(np.float32)
    found = 0
    for k in range(len(q)):
        ores, opath = O.astar_query_on_map(g, stand_in, q["start"][k], q["goal"][k])
        if moved:
            assert res["status"][k] == (0 if ores.status == 0 else 1), k
        else:
            assert res["status"][k] == ores.status, k
        if ores.status == 0:
            assert res["path_len"][k] == ores.path_len and res["cost"][k] == ores.cost, k
            assert np.array_equal(paths[k][:ores.path_len], opath), k
            if settled is not None:
                assert settled[k] == ores.settled, k
            found += 1
    return found


def queries(rng, blocked, n, want_band):
    """random free cells plus starts / goals inside the inflated band (blocked for the robot, free for a point)"""
    free = np.flatnonzero(blocked == 0)
    q = np.zeros(n, np.dtype([("start", "<i4"), ("goal", "<i4")]))
    q["start"], q["goal"] = rng.choice(free, n), rng.choice(free, n)
    band = np.flatnonzero(want_band)
    if band.size:
        q["start"][:8] = rng.choice(band, 8)
        q["goal"][8:16] = rng.choice(band, 8)
    q["goal"][16] = q["start"][16]
    return q


SEARCHES = [(96, 80, 0.05, (1.25, -2.5), 0.3, False), (257, 131, 0.05, (1000.3, -517.9), 0.25, False),
            (257, 131, 0.05, (1.25, -2.5), 0.3, True), (130, 67, 0.1, (1.25, -2.5), 0.5, True)]


@pytest.mark.parametrize("rows,cols,res,pos,r,moved", SEARCHES,   # (the ids of the cases at 0.05 m: as they were without `res`)
                         ids=["%d-%d-%spos%d-%s-%s" % (c[0], c[1], "" if k < 3 else "res%g-" % c[2], k, c[4], c[5]) for k, c in enumerate(SEARCHES)])
def test_search_matches_oracle(R, rows, cols, res, pos, r, moved):
    master = sample_map(rows, cols, seed=7 + rows, occupied=0.002)
    e, g = make_engine_and_geom(R, rows, cols, master, pos, res=res)
    if moved:
        master = move_both(R, e, g, master, (pos[0] + 3.37, pos[1] - 1.12))
    e.astar_robot_radius(r)
    e.astar_configure(max_queries=96)
    blocked = check_masks(e, g, master, r)
    point = (~np.isnan(master)) & (master > 0)
    q = queries(np.random.default_rng(rows), blocked, 96, (blocked == 1) & ~point)
    res, paths = e.astar(q, 8192)
    settled = e.astar_settled(len(q))
    found = check_search(e, g, blocked, q, res, paths, settled, moved)
    assert found >= 32
    assert (res["status"][:16] != 0).all()          # a start or goal inside the inflated band answers as a blocked one
    e.close()


def rays(rng, n, half, cx=0.0, cy=0.0, hit=0.7):
    r = np.zeros(n, O.RAY_DTYPE)
    ox, oy = rng.uniform(-half, half, n) + cx, rng.uniform(-half, half, n) + cy
    th, ln = rng.uniform(-np.pi, np.pi, n), rng.uniform(0.0, half, n)
    r["sx"], r["sy"] = ox, oy
    r["ex"], r["ey"] = ox + ln * np.cos(th), oy + ln * np.sin(th)
    r["clear_end"] = (rng.random(n) >= hit).astype(np.int32)
    return r


def test_pipelined_batches_keep_their_snapshot_across_updates_and_radius_changes(R):
    """depth-4 pipeline, rna_update_map (compose mode 0: the incremental refresh) between batches and a radius change
    after the fourth: every batch answers for the map AND the radius of its launch.  (Few marking rays and a second radius
    of 0.25 m keep the free space connected: 44-64 of the 64 queries of each batch have a path, and 39-60 of them answer
    differently under the other radius.)"""
    hip = Hip()
    rows = cols = 128
    master = sample_map(rows, cols, seed=11, occupied=0.002, edge=False)
    e, g = make_engine_and_geom(R, rows, cols, master, (0.0, 0.0))
    e.upload(R.capi.LAYER_LASER, master)
    e.compose_master(1)
    e.astar_robot_radius(0.15)
    e.astar_pipeline_depth(4)
    e.astar_configure(max_queries=64)
    rng = np.random.default_rng(2)
    ref, nq, max_len = master.copy(), 64, 4096
    issued = []
    for b in range(6):
        rs = rays(rng, 200, 2.5, hit=0.15)
        O.himm_update(g, ref, rs)
        e.update_map(rs.view(R.capi.RAY_DTYPE), compose_mode=0)
        if b == 3:
            e.astar_robot_radius(0.25)
        r = e.astar_robot_radius()
        blocked = ref_blocked(g, ref, r)
        q = queries(rng, blocked, nq, np.zeros(0))
        d_q, d_paths, d_res = hip.upload(q), hip.alloc(nq * max_len * 4), hip.alloc(nq * 24)
        e.astar_device(d_q, nq, d_paths, max_len, d_res)
        issued.append((blocked, q, d_q, d_paths, d_res))
    e.synchronize()
    for blocked, q, d_q, d_paths, d_res in issued:
        res = hip.download(d_res, R.capi.ASTAR_RESULT_DTYPE, nq)
        paths = hip.download(d_paths, np.int32, nq * max_len).reshape(nq, max_len)
        assert check_search(e, g, blocked, q, res, paths, None, False) >= nq // 4
        for p in (d_q, d_paths, d_res):
            hip.h.hipFree(p)
    assert np.array_equal(e.astar_blocked_mask(), ref_blocked(g, ref, 0.25))
    e.close()


def test_incremental_refresh_equals_full_rebuild(R):
    rows, cols = 200, 150
    master = sample_map(rows, cols, seed=3, occupied=0.002)
    e, g = make_engine_and_geom(R, rows, cols, master, (0.4, -0.3))
    e.upload(R.capi.LAYER_LASER, master)
    e.compose_master(1)
    e.astar_robot_radius(0.3)
    e.nbr_mask()                                      # the full build; the updates below refresh dirty tiles + ring
    rng = np.random.default_rng(9)
    ref = master.copy()
    for _ in range(4):
        rs = rays(rng, 400, 4.0, 0.4, -0.3)
        O.himm_update(g, ref, rs)
        e.update_map(rs.view(R.capi.RAY_DTYPE), compose_mode=0)
    inc_blocked, inc_nbr = e.astar_blocked_mask(), e.nbr_mask()
    e.astar_robot_radius(0.3)                         # the same radius again: a full rebuild of the same master
    assert np.array_equal(inc_blocked, e.astar_blocked_mask())
    assert np.array_equal(inc_nbr, e.nbr_mask())
    assert np.array_equal(inc_blocked, ref_blocked(g, ref, 0.3))
    e.close()


# rna_if_blocked_batch[_device]: rows, cols, res, moved to, radii (a whole number of cells, k + 1/2 cells, and one larger
# than the margin by which the positions go outside: 0.6 m, which is 6 cells at 0.1 m)
IF_BLOCKED = [(96, 80, 0.05, None, (0.1, 0.3, 0.125, 1.0)), (70, 45, 0.1, None, (0.5, 0.25, 1.0)),
              (96, 80, 0.05, (2.33, -1.61), (0.3, 0.125, 1.0))]
_if_blocked_want = {}


def if_blocked_setup(R, case):
    """the engine, the oracle's geometry, the master and the 10 000 positions of a case of IF_BLOCKED: uniform up to the
    margin outside the map, 1000 on its x edges, 1000 on its y edges, 1000 on cell corners, from that geometry's bounds"""
    rows, cols, res, target, radii = IF_BLOCKED[case]
    master = sample_map(rows, cols, seed=21)
    e, g = make_engine_and_geom(R, rows, cols, master, (1.25, -2.5), res=res)
    if target:
        master = move_both(R, e, g, master, target)
    rng = np.random.default_rng(4)
    L = np.array([rows * res, cols * res])
    lo, hi = np.array(g.pos) - L / 2, np.array(g.pos) + L / 2
    margin = max(0.6, 6 * res)
    xy = rng.uniform(lo - margin, hi + margin, (10000, 2))
    xy[:1000, 0] = rng.choice([lo[0], hi[0]], 1000)                      # on the map's edges
    xy[1000:2000, 1] = rng.choice([lo[1], hi[1]], 1000)
    xy[2000:3000] = lo + res * rng.integers(0, rows + 1, (1000, 2))     # on cell corners
    assert max(radii) > margin
    return e, g, master, xy, radii


def if_blocked_want(case, g, master, xy, r):
    """the reference's answer at every position, computed once for the host and the device-pointer test"""
    if (case, r) not in _if_blocked_want:
        rows, cols = g.size[0], g.size[1]
        occ = (~np.isnan(master)) & (master > 0)
        want = np.zeros(len(xy), np.uint8)
        for k in range(len(xy)):
            c = O.circle_cells(g, tuple(xy[k]), r, reference=REFERENCE)
            ok = (c[:, 0] >= 0) & (c[:, 0] < rows) & (c[:, 1] >= 0) & (c[:, 1] < cols)
            want[k] = occ[c[ok, 0] + c[ok, 1] * rows].any()
        want.flags.writeable = False
        _if_blocked_want[(case, r)] = want
    return _if_blocked_want[(case, r)]


@pytest.mark.parametrize("case", range(len(IF_BLOCKED)))
def test_if_blocked_matches_reference_predicate(R, case):
    e, g, master, xy, radii = if_blocked_setup(R, case)
    for r in radii:
        got = e.if_blocked(xy, r)
        want = if_blocked_want(case, g, master, xy, r)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (r, xy[bad[:5]], got[bad[:5]])
        if r == 0.3:
            og = np.array([O.lib().og_if_blocked(C.byref(g), O.fptr(master), O.d2(*p)) for p in xy], np.uint8)
            assert np.array_equal(got, og)
        assert 0 < got.sum() < len(xy)
    with pytest.raises(R.capi.RnaError):
        e.if_blocked(xy[:4], -0.1)
    e.close()


@pytest.mark.parametrize("case", range(len(IF_BLOCKED)))
def test_if_blocked_device_pointers_answer_as_the_host_entry(R, case):
    """rna_if_blocked_batch_device on positions and an output buffer of the caller's: the same bytes as the host entry and
    as the reference.  (The output buffer starts as 0xEE: every byte must have been written.)"""
    hip = Hip()
    e, g, master, xy, radii = if_blocked_setup(R, case)
    d_xy, d_out = hip.upload(xy), hip.alloc(len(xy))
    for r in radii:
        assert hip.h.hipMemset(d_out, 0xEE, len(xy)) == 0
        e.if_blocked_device(d_xy, len(xy), r, d_out)
        e.synchronize()
        got = hip.download(d_out, np.uint8, len(xy))
        assert got.tobytes() == e.if_blocked(xy, r).tobytes()
        assert got.tobytes() == if_blocked_want(case, g, master, xy, r).tobytes(), r
    with pytest.raises(R.capi.RnaError):
        e.if_blocked_device(d_xy, 4, -0.1, d_out)
    hip.free(d_xy)
    hip.free(d_out)
    e.close()


def test_radius_range_is_checked(R):
    e = R.Engine(3.2, 3.2, 0.05)
    for bad in (-0.01, float("nan"), float("inf"), 64 * 0.05):
        with pytest.raises(R.capi.RnaError):
            e.astar_robot_radius(bad)
    assert e.astar_robot_radius() == 0.0
    assert e.astar_robot_radius(63 * 0.05) == 63 * 0.05
    e.close()


def test_radius_zero_is_untouched_and_clones_copy_the_radius(R):
    """r = 0.3 and back to 0 gives the masks of a fresh engine (the point-robot kernels); rna_clone and
    rna_create_submap carry the radius"""
    n = 512
    master = R.synth.obstacles_rect(n, n, density=0.30, seed=2)
    a = R.Engine(n * 0.05, n * 0.05, 0.05)
    b = R.Engine(n * 0.05, n * 0.05, 0.05)
    for e in (a, b):
        e.upload(R.capi.LAYER_LASER, master)
        e.compose_master(1)
    b.astar_robot_radius(0.3)
    inflated = b.nbr_mask()
    assert not np.array_equal(inflated, a.nbr_mask())
    b.astar_robot_radius(0.0)
    assert np.array_equal(a.nbr_mask(), b.nbr_mask())
    blocked, nbr = O.astar_masks(master, n, n)
    assert np.array_equal(b.astar_blocked_mask(), blocked) and np.array_equal(b.nbr_mask(), nbr)
    q = R.synth.astar_queries(64, master, n, n, seed=5)
    ra, pa = a.astar(q, 8192)
    rb, pb = b.astar(q, 8192)
    assert np.array_equal(ra[["status", "path_len", "cost"]], rb[["status", "path_len", "cost"]]) and np.array_equal(pa, pb)
    b.astar_robot_radius(0.3)
    h = C.c_void_p()
    assert b._L.rna_clone(b.h, C.byref(h)) == 0
    r = C.c_double(0.0)
    assert b._L.rna_astar_get_robot_radius(h, C.byref(r)) == 0 and r.value == 0.3
    out = np.empty(n * n, np.uint8)
    assert b._L.rna_astar_download_nbr_mask(h, out.ctypes.data, out.size) == 0
    assert np.array_equal(out, inflated)
    b._L.rna_destroy(h)
    sub = b.submap_engine(0.0, 0.0, 6.0, 6.0)
    assert sub.astar_robot_radius() == 0.3
    sub.close()
    a.close()
    b.close()
