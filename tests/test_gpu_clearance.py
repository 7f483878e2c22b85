"""GPU: the clearance field (rna_clearance_*, csrc/clearance.hip) and the goal field's clearance cost
(rna_goal_field_set_clearance_cost, csrc/goal_field.hip), every cell compared for equality.

Both oracles are written here, integers only:
  clearance   from the blocked bytes the engine reports (rna_astar_download_blocked), un-rotated to map space: g = distance
              along i to the nearest blocked cell (two running scans), then min over |dj| <= R of dj^2 + g[j + dj]^2, capped.
              Cross-checked once against the plain all-pairs definition.
  field       heapq Dijkstra from the goal over the neighbour masks the engine reports, with
              field[c] = pen[c] + min over the neighbours n that c's mask allows of field[n] + w(n, c);
              next[c] = the first neighbour in the contract's order with field[n] + w + pen[c] == field[c]; paths follow next.
Shapes: 130 x 70 cells = 3 x 2 tiles with ragged edges; 200 x 136 for R = 63, where the halo spans a whole neighbouring tile."""
import ctypes as C
import heapq

import numpy as np
import pytest

import _oracle as O
from _gpu import (NB_DI, NB_DJ, NB_W, NONE, TABLE, UNREACHED, Hip, R, engine_centre, make_engine, to_buffer,  # noqa: F401  (R: the fixture)
                  to_map)

pytestmark = pytest.mark.gpu

RES = 0.05


# ---- the clearance oracle ----
def clearance_oracle(blocked, cap):
    """blocked: [j, i] array in map space -> uint16 [j, i]"""
    cols, rows = blocked.shape
    big = 1 << 20
    g = np.full((cols, rows), big, np.int64)
    run = np.full(cols, big, np.int64)
    for i in range(rows):                       # nearest blocked cell at or below i
        run = np.where(blocked[:, i] != 0, 0, run + 1)
        g[:, i] = run
    run = np.full(cols, big, np.int64)
    for i in range(rows - 1, -1, -1):           # ... at or above i
        run = np.where(blocked[:, i] != 0, 0, run + 1)
        g[:, i] = np.minimum(g[:, i], run)
    g = np.minimum(g, big)
    best = np.full((cols, rows), np.iinfo(np.int64).max, np.int64)
    for dj in range(-cap, cap + 1):
        lo, hi = max(0, -dj), min(cols, cols - dj)      # rows j with 0 <= j + dj < cols
        if lo < hi:
            best[lo:hi] = np.minimum(best[lo:hi], dj * dj + g[lo + dj:hi + dj] ** 2)
    return np.where(best <= cap * cap, best, NONE).astype(np.uint16)


def clearance_all_pairs(blocked, cap):
    cols, rows = blocked.shape
    out = np.full((cols, rows), NONE, np.uint16)
    obst = [(i, j) for j in range(cols) for i in range(rows) if blocked[j, i]]
    for j in range(cols):
        for i in range(rows):
            d = min([(i - a) ** 2 + (j - b) ** 2 for a, b in obst] or [1 << 30])
            if d <= cap * cap:
                out[j, i] = d
    return out


def test_the_clearance_oracle_is_the_all_pairs_definition():
    rng = np.random.default_rng(5)
    blocked = (rng.random((17, 20)) < 0.02).astype(np.uint8)
    blocked[3, 0] = blocked[16, 19] = 1
    assert blocked.sum() >= 4
    for cap in (1, 3, 7, 20):
        assert np.array_equal(clearance_oracle(blocked, cap), clearance_all_pairs(blocked, cap))
    empty = np.zeros((17, 20), np.uint8)
    assert (clearance_oracle(empty, 7) == NONE).all() and np.array_equal(clearance_all_pairs(empty, 7), clearance_oracle(empty, 7))


def check_clearance(e, cap):
    """build with `cap`, compare every cell with the oracle over the engine's own blocked set; returns the field [j, i] in map space"""
    g = e.geometry()
    s0, s1 = g.start_index[0], g.start_index[1]
    got = e.clearance(cap)
    assert e.clearance_info() == (cap, False) and e.clearance_ptr()
    blocked = to_map(e.astar_blocked_mask(), e.rows, e.cols, s0, s1)
    assert e.clearance_info() == (cap, False)
    want = clearance_oracle(blocked, cap)
    got = to_map(got, e.rows, e.cols, s0, s1)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (cap, bad[:10], [(int(got[j, i]), int(want[j, i])) for j, i in bad[:10]])
    assert (got[blocked != 0] == 0).all()
    return got


def obstacle_map(rows, cols, cap, seed, rects=6):
    """random rectangles, and single cells 1, cap and cap + 1 cells either side of the tile border at 64 and of the map edge"""
    rng = np.random.default_rng(seed)
    m = np.zeros((cols, rows), np.float32)
    m[rng.random((cols, rows)) < 0.3] = np.nan              # unknown cells do not block
    for _ in range(rects):
        w, h = rng.integers(1, 12, 2)
        i, j = rng.integers(0, rows - w), rng.integers(0, cols - h)
        m[j:j + h, i:i + w] = 180.0
    for d in (1, cap, cap + 1):
        along = [64 - d, 63 + d, d, rows - 1 - d]
        across = [64 - d, 63 + d, d, cols - 1 - d]
        for k, i in enumerate(along):
            j = int(rng.integers(0, cols))
            if 0 <= i < rows:
                m[j, i] = 200.0 + k
        for k, j in enumerate(across):
            i = int(rng.integers(0, rows))
            if 0 <= j < cols:
                m[j, i] = 200.0 + k
    m[0, 0] = 255.0
    m[cols - 1, rows - 1] = 255.0
    return m


def shape_for(cap):
    return (200, 136) if cap == 63 else (130, 70)


# ---- 1. clearance for R in {1, 7, 20, 63} ----
@pytest.mark.parametrize("cap", [1, 7, 20, 63])
def test_clearance_matches_the_oracle(R, cap):
    rows, cols = shape_for(cap)
    e = make_engine(R, rows, cols)
    assert e.clearance_info() == (0, False) and e.clearance_ptr() is None
    buf = np.zeros(rows * cols, np.uint16)
    assert e._L.rna_clearance_download(e.h, buf.ctypes.data, buf.size) == -5          # RNA_ESTATE before a build
    for seed, rects in ((1, 6), (2, 0), (3, 25)):
        e.upload(R.capi.LAYER_MASTER, obstacle_map(rows, cols, cap, seed + 10 * cap, rects))
        assert e.clearance_info() == ((0, False) if seed == 1 else (cap, True))        # an upload can change the masks
        got = check_clearance(e, cap)
        assert ((got > 0) & (got != NONE)).any()
    e.upload(R.capi.LAYER_MASTER, np.full(rows * cols, np.nan, np.float32))           # an empty map: every cell reads NONE
    assert (check_clearance(e, cap) == NONE).all()
    e.upload(R.capi.LAYER_MASTER, np.full(rows * cols, 180.0, np.float32))            # a fully blocked one: every cell 0
    assert (check_clearance(e, cap) == 0).all()
    assert e._L.rna_clearance_build(e.h, 0) == -1 and e._L.rna_clearance_build(e.h, 64) == -1
    assert e._L.rna_clearance_download(e.h, buf.ctypes.data, buf.size - 1) == -1
    assert e.clearance_info() == (cap, False)                                         # refused calls leave the field alone
    e.close()


# ---- 2. robot radius: the inflated set ----
def test_clearance_uses_the_robot_radius(R):
    rows, cols = 130, 70
    master = obstacle_map(rows, cols, 7, 77)
    e = make_engine(R, rows, cols, master)
    plain = check_clearance(e, 7)
    n_plain = int(e.astar_blocked_mask().sum())
    e.astar_robot_radius(0.15)
    assert e.clearance_info() == (7, True)
    assert int(e.astar_blocked_mask().sum()) > n_plain
    for cap in (7, 20):
        inflated = check_clearance(e, cap)
    assert not np.array_equal(plain, check_clearance(e, 7))
    assert (inflated == 0).sum() > n_plain
    e.close()


# ---- 3. a moved map: an obstacle and its neighbourhood across the buffer seam ----
def test_clearance_on_a_moved_map(R):
    rows, cols = 130, 70
    e = make_engine(R, rows, cols, np.zeros(rows * cols, np.float32), pos=(1.25, -2.5))
    assert e.move(1.25 + 37 * RES, -2.5 - 22 * RES)
    g = e.geometry()
    s0, s1 = g.start_index[0], g.start_index[1]
    assert s0 % 64 != 0 and s1 % 64 != 0 and s0 != 0 and s1 != 0
    # map cell (i, j) sits at buffer ((i + s0) % rows, (j + s1) % cols): the seam lies between map rows - s0 - 1 | rows - s0
    si, sj = rows - s0, cols - s1
    m = np.zeros((cols, rows), np.float32)
    m[3, 5] = m[cols - 2, rows - 7] = m[1, rows - 1] = 180.0
    m[sj - 2:sj + 2, si - 2:si + 2] = 180.0            # a block across both seams
    m[sj + 9, si - 1] = 180.0                          # single cells just either side of them
    m[sj - 1, si + 9] = 180.0
    e.upload(R.capi.LAYER_MASTER, to_buffer(m, rows, cols, s0, s1))
    for cap in (7, 20):
        got = check_clearance(e, cap)
        assert got[sj + 9, si] == 1 and got[sj + 9, si - 2] == 1 and got[sj, si + 9] == 1 and got[sj - 2, si + 9] == 1
    e.close()


# ---- 4. stale after a HIMM batch, a rebuild equals a fresh engine's ----
def test_clearance_stale_after_a_map_update_and_rebuild(R):
    rows, cols = 130, 70
    m = np.zeros((cols, rows), np.float32)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 180.0
    master = m.reshape(-1)
    e = make_engine(R, rows, cols, master)
    e.upload(R.capi.LAYER_LASER, master)
    e.compose_master(1)
    old = check_clearance(e, 20)
    assert old[35, 65] == NONE
    cell = 65 + 35 * rows
    rs = np.zeros(1, R.capi.RAY_DTYPE)
    rs["sx"][0], rs["sy"][0] = engine_centre(e, cell + 6 * rows)
    rs["ex"][0], rs["ey"][0] = engine_centre(e, cell)
    e.update_map(rs, compose_mode=0)
    assert e.clearance_info() == (20, True)
    assert np.array_equal(to_map(e.clearance_download(), rows, cols, 0, 0), old)      # a snapshot until it is rebuilt
    now = e.download(R.capi.LAYER_MASTER)
    assert now[cell] > 0
    new = check_clearance(e, 20)
    assert new[35, 65] == 0 and new[35, 60] == 25 and not np.array_equal(new, old)
    fresh = make_engine(R, rows, cols, now)
    assert np.array_equal(fresh.clearance(20), e.clearance_download())
    fresh.close()
    e.close()


# ---- the field oracle ----
def pen_of(clr, table):
    """cost per cell from the squared clearance: entry k for k^2 <= clr < (k + 1)^2, k = 1 .. len(table) - 1"""
    cap = len(table) - 1
    by_d2 = np.zeros(cap * cap + 1, np.int64)
    for k in range(1, cap + 1):
        by_d2[k * k:min((k + 1) * (k + 1), cap * cap + 1)] = int(table[k])
    c = clr.astype(np.int64)
    return np.where(c <= cap * cap, by_d2[np.minimum(c, cap * cap)], 0)


def field_oracle(nbr, pen, goal):
    """nbr, pen: [j, i] arrays in map space; goal = (i, j).  Returns (field, next) as [j, i] arrays."""
    cols, rows = nbr.shape
    field = np.full((cols, rows), UNREACHED, np.int64)
    nxt = np.full((cols, rows), 255, np.uint8)
    field[goal[1], goal[0]] = 0
    heap = [(0, goal[0], goal[1])]
    nb, pn = nbr.tolist(), pen.tolist()
    dist = field.tolist()
    while heap:
        d, i, j = heapq.heappop(heap)
        if d != dist[j][i]:
            continue
        for k in range(8):                       # the cells c that may step to (i, j): c = (i, j) + offset k, its direction back is 7 - k
            a, b = i + NB_DI[k], j + NB_DJ[k]
            if a < 0 or b < 0 or a >= rows or b >= cols or not (nb[b][a] >> (7 - k)) & 1:
                continue
            nd = d + NB_W[k] + pn[b][a]
            if nd < dist[b][a]:
                dist[b][a] = nd
                heapq.heappush(heap, (nd, a, b))
    field = np.array(dist, np.int64)
    assert field[field != UNREACHED].max() < (1 << 30)
    field[goal[1], goal[0]] = 0
    # next: the first neighbour in the contract's order that explains the cell's value
    pad = np.full((cols + 2, rows + 2), UNREACHED, np.int64)
    pad[1:-1, 1:-1] = field
    for k in range(7, -1, -1):
        fn = pad[1 + NB_DJ[k]:1 + NB_DJ[k] + cols, 1 + NB_DI[k]:1 + NB_DI[k] + rows]
        hit = (((nbr >> k) & 1) != 0) & (fn != UNREACHED) & (field != UNREACHED) & (fn + NB_W[k] + pen == field)
        nxt[hit] = k
    nxt[goal[1], goal[0]] = 8
    assert ((nxt != 255) == (field != UNREACHED)).all()
    return field, nxt


def walk(nxt, field, start, rows, cols, s0, s1, max_len):
    """(status, path_len, cost, path as buffer cells) of buffer cell `start` by the `next` bytes [j, i] in map space"""
    if start < 0 or start >= rows * cols:
        return 2, 0, UNREACHED, []
    i, j = (start % rows - s0) % rows, (start // rows - s1) % cols
    if field[j, i] == UNREACHED:
        return 1, 0, UNREACHED, []
    cost, out = int(field[j, i]), []
    while True:
        out.append((i + s0) % rows + ((j + s1) % cols) * rows)
        k = int(nxt[j, i])
        if k == 8:
            break
        i, j = i + NB_DI[k], j + NB_DJ[k]
    return (3 if len(out) > max_len else 0), len(out), cost, out


def check_field(e, goal, table):
    """builds the field of buffer cell `goal` with the engine's present table and compares field, next and the totals"""
    rows, cols = e.rows, e.cols
    g = e.geometry()
    s0, s1 = g.start_index[0], g.start_index[1]
    info = e.goal_field(goal)
    nbr = to_map(e.nbr_mask(), rows, cols, s0, s1)
    if len(table):
        cap = len(table) - 1
        assert e.clearance_info() == (cap, False)
        clr = to_map(e.clearance_download(), rows, cols, s0, s1)
        assert np.array_equal(clr, clearance_oracle(to_map(e.astar_blocked_mask(), rows, cols, s0, s1), cap))
        pen = pen_of(clr, table)
    else:
        pen = np.zeros((cols, rows), np.int64)
    blocked = to_map(e.astar_blocked_mask(), rows, cols, s0, s1)
    gi, gj = (goal % rows - s0) % rows, (goal // rows - s1) % cols
    field, nx = e.goal_field_download(want_next=True)
    field, nx = to_map(field, rows, cols, s0, s1), to_map(nx, rows, cols, s0, s1)
    if blocked[gj, gi]:
        assert info["status"] == 2 and (field == UNREACHED).all() and (nx == 255).all()
        return None
    want, want_nx = field_oracle(nbr, pen, (gi, gj))
    bad = np.argwhere(field != want)
    assert bad.size == 0, (bad[:10], [(int(field[j, i]), int(want[j, i])) for j, i in bad[:10]])
    bad = np.argwhere(nx != want_nx)
    assert bad.size == 0, (bad[:10], [(int(nx[j, i]), int(want_nx[j, i])) for j, i in bad[:10]])
    reached = want != UNREACHED
    assert (info["goal"], info["status"], info["stale"]) == (goal, 0, 0)
    assert info["reached"] == int(reached.sum()) and info["max_cost"] == int(want[reached].max())
    return want, want_nx, pen, blocked


def check_paths(e, want, want_nx, starts, max_len):
    rows, cols = e.rows, e.cols
    g = e.geometry()
    s0, s1 = g.start_index[0], g.start_index[1]
    paths, res = e.goal_field_paths(starts, max_len)
    seen = set()
    for k, s in enumerate(starts):
        status, n, cost, p = walk(want_nx, want, int(s), rows, cols, s0, s1, max_len)
        r = res[k]
        assert (r["status"], r["path_len"], r["cost"]) == (status, n, cost), (k, s, r, status, n, cost)
        assert (r["expanded"], r["rounds"], r["buckets"]) == (0, 0, 0)
        if status == 0:
            assert np.array_equal(paths[k][:n], p), k
            assert cost == want[(p[0] // rows - s1) % cols, (p[0] % rows - s0) % rows]      # cost == field[start]
        seen.add(status)
    return seen


# ---- 5. a field with a table: 6 maps x 2 goals ----
@pytest.mark.parametrize("seed", range(6))
def test_field_with_a_clearance_cost(R, seed):
    rows, cols = 130, 70
    m = obstacle_map(rows, cols, 7, 100 + seed, rects=4 + 3 * seed)
    m[63:66, 63:66] = 0.0                                   # the goal on the tile corner (64, 64) and its ring are free
    m[62, 64] = 180.0                                       # ... two cells from an obstacle
    e = make_engine(R, rows, cols, m)
    e.goal_field_clearance_cost(TABLE)
    assert np.array_equal(e.goal_field_clearance_cost(), TABLE)
    rng = np.random.default_rng(seed)
    clr = to_map(e.clearance(7), rows, cols, 0, 0)
    band = np.argwhere((clr >= 1) & (clr <= 4))             # inside the penalised band, right next to an obstacle
    bj, bi = band[rng.integers(len(band))]
    for goal in (int(bi + bj * rows), 64 + 64 * rows):
        want, want_nx, pen, blocked = check_field(e, goal, TABLE)
        assert pen[goal // rows, goal % rows] > 0 and want[goal // rows, goal % rows] == 0       # the goal's own cost is not counted
        assert (pen[blocked == 0] > 0).any() and (want != UNREACHED).sum() > rows * cols // 4
        free = np.flatnonzero((want != UNREACHED).reshape(-1))
        lens = e.goal_field_paths(free[::max(1, len(free) // 61)][:59].astype(np.int32), 1)[1]["path_len"]
        starts = np.concatenate([free[::max(1, len(free) // 61)][:59], [goal, np.flatnonzero(blocked.reshape(-1))[3], -1, rows * cols,
                                                                       free[-1]]]).astype(np.int32)
        assert len(starts) == 64
        seen = check_paths(e, want, want_nx, starts, int(np.median(lens)))
        assert seen == {0, 1, 2, 3}
        assert check_paths(e, want, want_nx, starts, 4096) == {0, 1, 2}
    e.close()


# ---- 6. an all-zero table is the table-free build, byte for byte ----
def test_zero_table_equals_the_plain_field(R):
    rows, cols = 130, 70
    e = make_engine(R, rows, cols, obstacle_map(rows, cols, 7, 61, rects=12))
    goal = int(np.flatnonzero(e.astar_blocked_mask() == 0)[777])
    plain_info = e.goal_field(goal)
    plain = e.goal_field_download(want_next=True)
    assert e.clearance_info() == (0, False)                 # no table: no clearance field is built
    check_field(e, goal, [])
    e.goal_field_clearance_cost(np.zeros(8, np.uint16))
    info = e.goal_field(goal)
    zero = e.goal_field_download(want_next=True)
    assert e.clearance_info() == (7, False)
    assert plain[0].tobytes() == zero[0].tobytes() and plain[1].tobytes() == zero[1].tobytes()
    assert (info["reached"], info["max_cost"]) == (plain_info["reached"], plain_info["max_cost"])
    e.close()


# ---- 7. a corridor: the plain path hugs the wall, the penalised one does not ----
def plain_length(path, rows):
    p = np.asarray(path)
    di, dj = np.abs(np.diff(p % rows)), np.abs(np.diff(p // rows))
    return int(np.where((di + dj) == 2, 1414, 1000).sum())


def test_penalised_path_keeps_its_distance(R):
    rows, cols = 130, 70
    m = np.zeros((cols, rows), np.float32)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 180.0
    m[35, 0:100] = 180.0                                     # a wall along j = 35 with its tip at i = 99: the way round is a U-turn
    e = make_engine(R, rows, cols, m)
    start, goal = 10 + 30 * rows, 10 + 40 * rows
    e.goal_field(goal)
    paths, res = e.goal_field_paths(np.array([start], np.int32), 1024)
    assert res["status"][0] == 0
    plain = paths[0][:res["path_len"][0]].copy()
    e.goal_field_clearance_cost(TABLE)
    want, want_nx, pen, blocked = check_field(e, goal, TABLE)
    paths, res = e.goal_field_paths(np.array([start], np.int32), 1024)
    assert res["status"][0] == 0
    wide = paths[0][:res["path_len"][0]].copy()
    clr = e.clearance(20)                                    # (another cap than the table's: the next build makes its own again)
    assert int(clr[plain].min()) == 1                        # round the tip at one cell
    assert int(clr[wide].min()) > int(clr[plain].min())
    assert plain_length(wide, rows) > plain_length(plain, rows)
    assert res["cost"][0] == plain_length(wide, rows) + int(pen.reshape(-1)[wide[:-1]].sum())       # every cell but the goal pays
    assert e.clearance_info() == (20, False)
    check_field(e, goal, TABLE)
    assert e.clearance_info() == (7, False)
    e.close()


# ---- 8. setting the table marks the field stale; clearing it and rebuilding gives the plain field ----
def test_table_changes_mark_the_field_stale(R):
    rows, cols = 130, 70
    e = make_engine(R, rows, cols, obstacle_map(rows, cols, 7, 88, rects=10))
    goal = int(np.flatnonzero(e.astar_blocked_mask() == 0)[1234])
    assert len(e.goal_field_clearance_cost()) == 0
    e.goal_field_clearance_cost(TABLE)                       # (before any field: nothing to mark)
    assert e.goal_field_info()["goal"] == -1 and e.goal_field_info()["stale"] == 0
    e.goal_field_clearance_cost([])
    e.goal_field(goal)
    plain = e.goal_field_download(want_next=True)
    e.goal_field_clearance_cost(TABLE)
    assert e.goal_field_info()["stale"] == 1 and e.clearance_info() == (0, False)
    assert e.goal_field_download().tobytes() == plain[0].tobytes()       # a snapshot until it is rebuilt
    check_field(e, goal, TABLE)
    assert e.goal_field_info()["stale"] == 0
    assert e.goal_field_download().tobytes() != plain[0].tobytes()
    e.goal_field_clearance_cost([])
    assert e.goal_field_info()["stale"] == 1 and e.clearance_info() == (7, False)     # the masks did not change
    e.goal_field(goal)
    again = e.goal_field_download(want_next=True)
    assert again[0].tobytes() == plain[0].tobytes() and again[1].tobytes() == plain[1].tobytes()
    L, h = e._L, e.h
    t = np.zeros(65, np.uint16)
    assert L.rna_goal_field_set_clearance_cost(h, t.ctypes.data, 1) == -1 and L.rna_goal_field_set_clearance_cost(h, t.ctypes.data, 65) == -1
    assert L.rna_goal_field_set_clearance_cost(h, None, 8) == -1 and e.goal_field_info()["stale"] == 0
    e.close()


# ---- 9. with one pipelined batch in flight ----
def test_coexists_with_a_pipelined_batch(R):
    hip = Hip()
    rows, cols = 192, 160
    master = R.synth.obstacles_rect(rows, cols, density=0.2, seed=2)
    e = make_engine(R, rows, cols, master)
    blocked, nbr = O.astar_masks(master, rows, cols)
    e.astar_pipeline_depth(4)
    e.astar_configure(max_queries=32)
    e.goal_field_clearance_cost(TABLE)
    nq, max_len = 32, 2048
    q = R.synth.astar_queries(nq, master, rows, cols, seed=21)
    d_q, d_paths, d_res = hip.upload(q), hip.alloc(nq * max_len * 4), hip.alloc(nq * 24)
    e.astar_device(d_q, nq, d_paths, max_len, d_res)
    goal = int(q["goal"][0])
    want, want_nx, pen, _ = check_field(e, goal, TABLE)                 # built while the batch is in flight
    assert check_paths(e, want, want_nx, q["start"].astype(np.int32), max_len) >= {0}
    e.synchronize()
    res = hip.download(d_res, R.capi.ASTAR_RESULT_DTYPE, nq)
    sp = hip.download(d_paths, np.int32, nq * max_len).reshape(nq, max_len)
    for k in range(nq):                                                 # the batch search does not use the table
        ores, opath, _ = O.astar_query(nbr, rows, cols, q["start"][k], q["goal"][k])
        assert (res["status"][k], res["path_len"][k], res["cost"][k]) == (ores.status, ores.path_len, ores.cost), k
        assert np.array_equal(sp[k][:ores.path_len], opath), k
    for p in (d_q, d_paths, d_res):
        hip.h.hipFree(p)
    e.close()


# ---- 10. a clone carries the table (not the fields) ----
def test_clone_and_submap_carry_the_table(R):
    rows, cols = 130, 70
    e = make_engine(R, rows, cols, obstacle_map(rows, cols, 7, 9, rects=8))
    e.goal_field_clearance_cost(TABLE)
    goal = int(np.flatnonzero(e.astar_blocked_mask() == 0)[900])
    e.goal_field(goal)
    h = C.c_void_p()
    assert e._L.rna_clone(e.h, C.byref(h)) == 0
    c = R.Engine.__new__(R.Engine)
    c._L, c.h, c.device, c.rows, c.cols, c.ncell, c.resolution, c.hist_size = e._L, h, e.device, rows, cols, rows * cols, e.resolution, None
    assert np.array_equal(c.goal_field_clearance_cost(), TABLE)
    assert c.goal_field_info()["goal"] == -1 and c.clearance_info() == (0, False) and c.clearance_ptr() is None
    c.goal_field(goal)
    assert c.goal_field_download().tobytes() == e.goal_field_download().tobytes()
    assert np.array_equal(c.clearance_download(), e.clearance_download())
    c.close()
    sub = e.submap_engine(0.0, 0.0, 2.0, 2.0)
    assert sub is not None and np.array_equal(sub.goal_field_clearance_cost(), TABLE) and sub.clearance_info() == (0, False)
    sub.close()
    e.close()
