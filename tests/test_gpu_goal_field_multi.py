"""GPU: the goal distance field with many sources, start costs and owner labels (rna_goal_field_build_multi,
csrc/goal_field.hip), every cell of field, next and owner compared for equality.

The oracle is written here from the definitions of include/rna.h, integers only: a heapq Dijkstra from a virtual super-source
(source k enters at its start cost seed[k]) over the neighbour masks and the blocked set the ENGINE reports, un-rotated to map
space, with field[c] = min(seed terms of c, pen[c] + min over the neighbours n that c's mask allows of field[n] + w(n, c));
pen from the downloaded clearance field and the table; a sum at or beyond 2^30 is FAR and FAR floods on; next = 8 on
terminals (a source whose seed IS the field value, ties to the terminal), else the first neighbour in the contract's order
with field[n] + w + pen[c] == field[c]; owner = the smallest such source of the terminal the walk along next ends at.

Maps are 130 x 70 cells (3 x 2 ragged 64 x 64 tiles) unless a test says otherwise; what a map is there for is asserted on
the ORACLE's answer, so a map that stops exercising it fails loudly."""
import heapq
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as O
from _gpu import (NB_DI, NB_DJ, NB_W, NONE, TABLE, UNREACHED, Hip, R, blocked_of, engine_centre, make_engine,  # noqa: F401  (R: the fixture)
                  to_buffer, to_map)

pytestmark = pytest.mark.gpu

FAR = 0x7ffffffe
LIMIT = 1 << 30
RES = 0.05
ROWS, COLS = 130, 70
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle ----
class Want:
    """the definitions' answer for the engine's present masks, blocked set and (with a table) clearance field; every array
    in BUFFER order"""

    def __init__(self, e, goals, seed=None, table=None):
        rows, cols = e.rows, e.cols
        n = rows * cols
        g = e.geometry()
        s0, s1 = g.start_index[0], g.start_index[1]
        jj, ii = np.mgrid[0:cols, 0:rows]
        buf = (((jj + s1) % cols) * rows + (ii + s0) % rows).reshape(-1)          # buffer index of map cell j * rows + i
        self.buf = buf
        nbr = e.nbr_mask()[buf].tolist()
        blocked = e.astar_blocked_mask()[buf]
        pen = np.zeros(n, np.int64)
        if table is not None and len(table):
            clr = e.clearance_download()[buf].astype(np.int64)
            cap = len(table) - 1
            k = np.floor(np.sqrt(clr)).astype(np.int64)
            k = np.where(k * k > clr, k - 1, k)
            k = np.where((k + 1) * (k + 1) <= clr, k + 1, k)
            pen = np.where((clr <= cap * cap) & (k >= 1), np.asarray(table, np.int64)[np.minimum(k, cap)], 0)
        self.pen_m = pen
        pen = pen.tolist()
        goals = [int(c) for c in np.asarray(goals).reshape(-1)]
        seed = [0] * len(goals) if seed is None else [int(s) for s in np.asarray(seed).reshape(-1)]
        to_m = lambda b: ((b // rows - s1) % cols) * rows + (b % rows - s0) % rows   # noqa: E731
        best = {}                                                                   # map cell -> (least seed, its smallest k)
        self.blocked_sources = 0
        for k, (b, s) in enumerate(zip(goals, seed)):
            m = to_m(b)
            if blocked[m]:
                self.blocked_sources += 1
            elif m not in best or s < best[m][0]:
                best[m] = (s, k)
        dist = [UNREACHED] * n
        heap = []
        for m, (s, _) in best.items():
            dist[m] = s
            heap.append((s, m))
        heapq.heapify(heap)
        far_from = []
        while heap:
            d, c = heapq.heappop(heap)
            if d != dist[c]:
                continue
            ci, cj = c % rows, c // rows
            for k in range(8):                                                      # the cells t whose k-th neighbour is c
                ti, tj = ci - NB_DI[k], cj - NB_DJ[k]
                if not (0 <= ti < rows and 0 <= tj < cols):
                    continue
                t = tj * rows + ti
                if not (nbr[t] >> k) & 1:
                    continue
                nd = d + NB_W[k] + pen[t]
                if nd >= LIMIT:
                    far_from.append(t)
                elif nd < dist[t]:
                    dist[t] = nd
                    heapq.heappush(heap, (nd, t))
        far = set()
        queue = [t for t in far_from if dist[t] == UNREACHED]
        far.update(queue)
        while queue:
            c = queue.pop()
            ci, cj = c % rows, c // rows
            for k in range(8):
                ti, tj = ci - NB_DI[k], cj - NB_DJ[k]
                if 0 <= ti < rows and 0 <= tj < cols:
                    t = tj * rows + ti
                    if (nbr[t] >> k) & 1 and dist[t] == UNREACHED and t not in far:
                        far.add(t)
                        queue.append(t)
        nxt = [255] * n
        owner = [-1] * n
        step = [0] * n
        for c in sorted((c for c in range(n) if dist[c] < LIMIT), key=lambda c: dist[c]):
            if c in best and best[c][0] == dist[c]:
                nxt[c], owner[c], step[c] = 8, best[c][1], c
                continue
            ci, cj = c % rows, c // rows
            for k in range(8):
                if (nbr[c] >> k) & 1:
                    t = (cj + NB_DJ[k]) * rows + ci + NB_DI[k]
                    if dist[t] < LIMIT and dist[t] + NB_W[k] + pen[c] == dist[c]:
                        nxt[c], owner[c], step[c] = k, owner[t], t
                        break
            assert nxt[c] < 8, c
        for c in far:
            dist[c], nxt[c] = FAR, 254
        self.rows, self.cols, self.s0, self.s1 = rows, cols, s0, s1
        self.goals, self.seed = goals, seed
        self.field_m, self.next_m, self.owner_m, self.step_m = dist, nxt, owner, step
        self.field = np.empty(n, np.int32); self.field[buf] = np.array(dist, np.int64).astype(np.int32)
        self.next = np.empty(n, np.uint8); self.next[buf] = np.array(nxt, np.uint8)
        self.owner = np.empty(n, np.int32); self.owner[buf] = np.array(owner, np.int32)
        self.pen = np.empty(n, np.int64); self.pen[buf] = self.pen_m
        self.terminals = nxt.count(8)
        fin = self.field[self.field < LIMIT]
        self.reached, self.max_cost = int(fin.size), int(fin.max()) if fin.size else 0
        self.to_m = to_m

    def walk(self, b):
        """the buffer cells of the walk along next from buffer cell b (a reached one)"""
        c = self.to_m(int(b))
        out = [int(self.buf[c])]
        while self.next_m[c] != 8:
            c = self.step_m[c]
            out.append(int(self.buf[c]))
        return out

    def walk_m(self, c):
        out = [c]
        while self.next_m[c] != 8:
            c = self.step_m[c]
            out.append(c)
        return out


def downloads(e, owners=True):
    field, nx = e.goal_field_download(want_next=True)
    return field, nx, (e.goal_field_owners() if owners else None)


def first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return bad[:8], got[bad[:8]], want[bad[:8]]


def check(e, goals, seed=None, table=None, owners=True, device=None):
    """one build compared with the oracle: field, next and owner of every cell, the two info records"""
    goals = np.asarray(goals, np.int32)
    if device is not None:
        d_g = device.upload(goals)
        d_s = None if seed is None else device.upload(np.asarray(seed, np.int32))
        info = e.goal_field_multi_device(d_g, d_s, len(goals), owners=owners)
        device.free(d_g)
        if d_s:
            device.free(d_s)
    else:
        info = e.goal_field_multi(goals, seed, owners=owners)
    w = Want(e, goals, seed, table)
    field, nx, own = downloads(e, owners)
    assert np.array_equal(field, w.field), first_bad(field, w.field)
    assert np.array_equal(nx, w.next), first_bad(nx, w.next)
    status = 2 if w.blocked_sources == len(goals) else 0
    assert (info["goal"], info["status"], info["reached"], info["max_cost"], info["stale"]) == (int(goals[0]), status, w.reached, w.max_cost, 0)
    assert e.goal_field_info() == info
    src = e.goal_field_sources_info()
    assert (src["sources"], src["blocked_sources"], src["terminals"], src["owners"]) == (len(goals), w.blocked_sources, w.terminals, int(owners))
    if owners:
        assert np.array_equal(own, w.owner), first_bad(own, w.owner)
        assert e.goal_field_owners_ptr()
        assert src["owner_rounds"] <= math.ceil(math.log2(e.rows * e.cols)) + 1 and (src["owner_rounds"] >= 1) == (status == 0)
    return w, info


# ---- the maps (flat, buffer order of an unmoved map = map order) ----
def random_map(R, density, seed, rows=ROWS, cols=COLS):
    return R.synth.obstacles_rect(rows, cols, density=density, seed=seed, side=(2, 12)).copy()


def door_map(rows=ROWS, cols=COLS):
    m = np.zeros((cols, rows), np.float32)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 180.0
    m[:, 66] = 180.0                                                             # a wall just behind the tile border at 64 ...
    m[30:33, 66] = 0.0                                                           # ... with a door
    return m.reshape(-1)


def three_maps(R):
    return [random_map(R, 0.1, 11), random_map(R, 0.3, 12), door_map()]


def free_cells(e):
    return np.flatnonzero(e.astar_blocked_mask() == 0)


def cell(i, j, rows=ROWS):
    return i + j * rows


# ---- 1. one source with start cost 0 is rna_goal_field_build ----
@pytest.mark.parametrize("which", range(3))
def test_one_source_seed_zero_is_the_single_goal_build(R, which):
    master = three_maps(R)[which]
    m = master.reshape(COLS, ROWS)
    m[40:48, 100:108] = 180.0
    m[42:46, 102:106] = 0.0                                                      # an enclosed pocket
    e = make_engine(R, ROWS, COLS, master)
    free = free_cells(e)
    rng = np.random.default_rng(which)
    blocked_goal = int(np.flatnonzero(e.astar_blocked_mask())[17])
    for goal in (int(rng.choice(free)), cell(103, 43), blocked_goal):
        a = e.goal_field(goal)
        fa, na = e.goal_field_download(want_next=True)
        src = e.goal_field_sources_info()
        assert (src["sources"], src["owners"], src["terminals"]) == (1, 0, int(a["status"] == 0))
        for seed in (None, [0]):
            b = e.goal_field_multi([goal], seed)
            fb, nb = e.goal_field_download(want_next=True)
            assert np.array_equal(fa, fb) and np.array_equal(na, nb)
            for key in ("goal", "status", "reached", "max_cost", "tiles_reached"):
                assert a[key] == b[key], (key, a, b)
        assert a["status"] == (2 if goal == blocked_goal else 0)
        if goal == cell(103, 43):
            assert a["reached"] == 16
    e.close()


# ---- 2. random free sources ----
@pytest.mark.parametrize("n", [2, 5, 64, 1000])
@pytest.mark.parametrize("which", range(3))
def test_random_sources(R, which, n):
    e = make_engine(R, ROWS, COLS, three_maps(R)[which])
    rng = np.random.default_rng(100 * which + n)
    goals = rng.choice(free_cells(e), n)
    seed = None if which == 0 else rng.integers(0, 20000, n)
    w, info = check(e, goals, seed)
    assert w.blocked_sources == 0 and 1 <= w.terminals <= n and len(set(w.owner[w.owner >= 0].tolist())) == w.terminals
    e.close()


# ---- 3. where the sources lie ----
def test_source_placement(R):
    e = make_engine(R, ROWS, COLS, np.zeros(ROWS * COLS, np.float32))
    w, _ = check(e, [cell(10, 10), cell(40, 30)])                                # two sources in one tile
    assert w.terminals == 2 and (w.owner >= 0).all()
    w, _ = check(e, [cell(70, 20), cell(71, 20)])                                # two adjacent cells
    assert w.terminals == 2
    # a source on a tile corner whose in-tile neighbours are all blocked: its start cost has to reach the other tiles
    m = np.zeros((COLS, ROWS), np.float32)
    m[64, 65] = m[65, 64] = m[65, 65] = 180.0
    e.upload(R.capi.LAYER_MASTER, m.reshape(-1))
    w, info = check(e, [cell(64, 64), cell(5, 5)], [0, 50000])
    assert info["reached"] == ROWS * COLS - 3 and (w.owner == 0).sum() > 2000 and w.next[cell(63, 63)] == 7
    # a source in each of two components, a third component without one
    m = np.zeros((COLS, ROWS), np.float32)
    m[:, 40] = m[:, 90] = 180.0
    e.upload(R.capi.LAYER_MASTER, m.reshape(-1))
    w, info = check(e, [cell(10, 35), cell(120, 35)], [300, 0])
    middle = np.array([cell(i, j) for j in range(COLS) for i in range(41, 90)])
    assert (w.field[middle] == UNREACHED).all() and (w.owner[middle] == -1).all()
    assert (w.owner == 0).sum() == 40 * COLS and (w.owner == 1).sum() == 39 * COLS
    e.close()


# ---- 4. start costs ----
def test_seeds(R):
    e = make_engine(R, ROWS, COLS, np.zeros(ROWS * COLS, np.float32))
    a, b = cell(20, 20), cell(23, 20)
    w, _ = check(e, [a, b], [0, 5000])                                           # undercut by the arrival through a neighbour
    assert w.field[b] == 3000 and w.next[b] != 8 and w.owner[b] == 0 and w.terminals == 1 and (w.owner == 0).all()
    w, _ = check(e, [a, b], [0, 3000])                                           # exactly the arrival cost: a terminal
    assert w.field[b] == 3000 and w.next[b] == 8 and w.owner[b] == 1 and w.terminals == 2
    w, _ = check(e, [a, a, a, a], [700, 300, 500, 300])                          # three different seeds, the least one twice
    assert w.field[a] == 300 and w.terminals == 1 and (w.owner == 1).all()
    # 2^30 - 1: the source itself is exact, whatever it reaches lies beyond the 30-bit range
    m = np.zeros((COLS, ROWS), np.float32)
    m[:, 64] = 180.0
    e.upload(R.capi.LAYER_MASTER, m.reshape(-1))
    c = cell(100, 30)
    w, info = check(e, [cell(10, 10), c], [0, LIMIT - 1])
    right = np.array([cell(i, j) for j in range(COLS) for i in range(65, ROWS) if cell(i, j) != c])
    assert w.field[c] == LIMIT - 1 and w.next[c] == 8 and w.owner[c] == 1
    assert (w.field[right] == FAR).all() and (w.next[right] == 254).all() and (w.owner[right] == -1).all()
    assert info["reached"] == 64 * COLS + 1 and info["max_cost"] == LIMIT - 1
    # an empty map: the head start moves the border between the two regions by a known number of cells
    e.upload(R.capi.LAYER_MASTER, np.full(ROWS * COLS, np.nan, np.float32))
    i, j = np.meshgrid(np.arange(ROWS), np.arange(COLS))

    def octile(ci, cj):
        dx, dy = np.abs(i - ci), np.abs(j - cj)
        return (1000 * np.maximum(dx, dy) + 414 * np.minimum(dx, dy)).reshape(-1)

    for head, last_of_a in ((0, 59), (9000, 64), (41000, 80)):                   # row 35: 1000 (i - 20) against head + 1000 (100 - i)
        w, _ = check(e, [cell(20, 35), cell(100, 35)], [0, head])
        da, db = octile(20, 35), head + octile(100, 35)
        assert np.array_equal(w.field, np.minimum(da, db))
        assert (w.owner[da < db] == 0).all() and (w.owner[db < da] == 1).all()
        row = w.owner[cell(0, 35):cell(ROWS, 35)]
        first_of_b = last_of_a + (1 if head else 2)                              # (head 0: cell 60 is a tie, the canonical step decides)
        assert (row[:last_of_a + 1] == 0).all() and (row[first_of_b:] == 1).all()
    e.close()


# ---- 5. blocked sources ----
def test_blocked_sources(R):
    master = random_map(R, 0.2, 5)
    e = make_engine(R, ROWS, COLS, master)
    rng = np.random.default_rng(5)
    free, walls = free_cells(e), np.flatnonzero(e.astar_blocked_mask())
    goals = np.concatenate([rng.choice(free, 5), rng.choice(walls, 3)])
    rng.shuffle(goals)
    w, info = check(e, goals, rng.integers(0, 9000, 8))
    assert w.blocked_sources == 3 and info["status"] == 0
    w, info = check(e, rng.choice(walls, 6))                                     # every source blocked
    assert info["status"] == 2 and info["reached"] == 0 and (w.field == UNREACHED).all()
    assert (e.goal_field_owners() == -1).all() and (e.goal_field_download(want_next=True)[1] == 255).all()
    paths, res = e.goal_field_paths(free[:8].astype(np.int32), 32)
    assert (res["status"] == 1).all()
    # with a robot radius a source inside the inflated region counts as blocked
    e.astar_robot_radius(0.15)
    band = np.flatnonzero((e.astar_blocked_mask() == 1) & (blocked_of(master) == 0))
    assert band.size > 100
    w, info = check(e, [int(band[7]), int(free_cells(e)[50]), int(band[90])])
    assert w.blocked_sources == 2 and w.terminals == 1
    e.close()


# ---- 6. with a clearance cost ----
@pytest.mark.parametrize("which", [0, 2])
def test_clearance_cost(R, which):
    e = make_engine(R, ROWS, COLS, three_maps(R)[which])
    e.goal_field_clearance_cost(TABLE)
    clr = e.clearance(len(TABLE) - 1)
    blocked = e.astar_blocked_mask()
    rng = np.random.default_rng(which)
    near = np.flatnonzero((blocked == 0) & (clr > 0) & (clr <= 9))               # within three cells of an obstacle
    goals = np.concatenate([rng.choice(near, 3), rng.choice(free_cells(e), 3)])
    seed = np.concatenate([[0, 0, 0], rng.integers(0, 6000, 3)])                 # (start cost 0: those three are terminals)
    w, _ = check(e, goals, seed, table=TABLE)
    term = [k for k, c in enumerate(goals) if w.next[c] == 8]
    assert any(w.pen[goals[k]] > 0 and w.field[goals[k]] == seed[k] for k in term)    # its own cost is not charged on the seed term
    assert (w.pen > 0).sum() > 500
    e.close()


# ---- 7. a moved map ----
def test_moved_map(R):
    e = make_engine(R, ROWS, COLS, np.zeros(ROWS * COLS, np.float32), pos=(1.25, -2.5))
    assert e.move(1.25 + 37 * RES, -2.5 - 22 * RES)
    g = e.geometry()
    s0, s1 = g.start_index[0], g.start_index[1]
    assert s0 % 64 != 0 and s1 % 64 != 0
    si, sj = ROWS - s0, COLS - s1                                                # the seams lie before map column si and map row sj
    m = np.zeros((COLS, ROWS), np.float32)
    rng = np.random.default_rng(9)
    for _ in range(14):
        a, b = rng.integers(2, ROWS - 8), rng.integers(2, COLS - 8)
        m[b:b + rng.integers(1, 7), a:a + rng.integers(1, 7)] = 180.0
    m[sj - 8:sj + 8, si - 8:si + 8] = 0.0
    # one source at the seams' crossing, one in the middle of each of the four quarters the seams cut the map into
    srcs = [(si - 4, sj - 4), (si // 2, sj // 2), ((si + ROWS) // 2, sj // 2), (si // 2, (sj + COLS) // 2), ((si + ROWS) // 2, (sj + COLS) // 2)]
    for i, j in srcs:
        m[j - 1:j + 2, i - 1:i + 2] = 0.0
    e.upload(R.capi.LAYER_MASTER, to_buffer(m, ROWS, COLS, s0, s1))
    buf = lambda i, j: (i + s0) % ROWS + ((j + s1) % COLS) * ROWS                # noqa: E731
    assert {i >= si for i, _ in srcs} == {False, True} and {j >= sj for _, j in srcs} == {False, True}
    w, _ = check(e, [buf(i, j) for i, j in srcs], [0, 2000, 1000, 0, 500])
    mine = np.flatnonzero(np.array(w.owner_m) == 0)                              # map cells of the source at the seams' crossing
    assert {int(c % ROWS) >= si for c in mine} == {False, True} and {int(c // ROWS) >= sj for c in mine} == {False, True}
    assert w.terminals == 5
    e.close()


# ---- 8. long chains of exits ----
def test_serpentine(R):
    rows, cols = 200, 136
    m = np.zeros((cols, rows), np.float32)
    for k, j in enumerate(range(2, cols, 4)):
        m[j, :] = 180.0
        m[j, rows - 1 if k % 2 == 0 else 0] = 0.0
    e = make_engine(R, rows, cols, m.reshape(-1))
    # one source at the head of the corridor, one in the middle of the third lap with a head start against it just below the
    # cost of getting there: it is a terminal, and every walk from behind it ends there after some thirty laps
    goals, seed = [cell(0, 0, rows), cell(100, 8, rows)], [0, 450000]
    w = Want(e, goals, seed)
    far = int(np.argmax(np.where(np.array(w.field_m) < LIMIT, w.field_m, -1)))
    tiles = [(c % rows >> 6, c // rows >> 6) for c in w.walk_m(far)]
    runs = [t for k, t in enumerate(tiles) if k == 0 or t != tiles[k - 1]]
    assert len(runs) - 1 >= 64 and len(set(runs)) < len(runs)                   # crosses 64 tile borders, re-enters a tile it has left
    assert w.terminals == 2 and min((w.owner == 0).sum(), (w.owner == 1).sum()) > 500
    w2, _ = check(e, goals, seed)
    src = e.goal_field_sources_info()
    assert 2 <= src["owner_rounds"] <= math.ceil(math.log2(rows * cols)) + 1
    e.close()


# ---- 9. paths ----
def test_paths(R):
    hip = Hip()
    e = make_engine(R, ROWS, COLS, random_map(R, 0.2, 21))
    rng = np.random.default_rng(21)
    free, walls = free_cells(e), np.flatnonzero(e.astar_blocked_mask())
    goals, seed = rng.choice(free, 6), rng.integers(0, 4000, 6)
    w, _ = check(e, goals, seed)
    term = sorted({int(c) for c in goals if w.next[c] == 8})
    starts = np.concatenate([rng.choice(free, 58 - len(term)), walls[:4], [-1, ROWS * COLS], term]).astype(np.int32)
    assert len(starts) == 64 and len(term) >= 1
    for max_len in (512, 8):
        paths, res = e.goal_field_paths(starts, max_len)
        kinds = set()
        for k, s in enumerate(starts):
            r = res[k]
            if s < 0 or s >= ROWS * COLS:
                assert r["status"] == 2
                continue
            if w.field[s] == UNREACHED:
                assert r["status"] == 1 and r["path_len"] == 0
                continue
            want = w.walk(s)
            assert r["cost"] == w.field[s] and r["path_len"] == len(want), k
            assert r["status"] == (3 if len(want) > max_len else 0), k
            kinds.add((int(r["status"]), len(want) == 1))
            assert list(paths[k][:min(len(want), max_len)]) == want[:max_len], k            # every step is next's
            if r["status"] == 0:
                assert paths[k][len(want) - 1] == goals[w.owner[s]], k
                if len(want) == 1:
                    assert r["cost"] == min(sd for g, sd in zip(goals, seed) if g == s)
        assert (0, True) in kinds and (0, False) in kinds and ((3, False) in kinds) == (max_len == 8)
        d_s, d_p, d_r = hip.upload(starts), hip.alloc(64 * max_len * 4, zero=True), hip.alloc(64 * 24)
        e.goal_field_paths_device(d_s, 64, d_p, max_len, d_r)
        e.synchronize_map()
        assert np.array_equal(hip.download(d_r, R.capi.ASTAR_RESULT_DTYPE, 64), res)
        assert np.array_equal(hip.download(d_p, np.int32, 64 * max_len).reshape(64, max_len), paths)
        for p in (d_s, d_p, d_r):
            hip.free(p)
    e.close()


# ---- 10. the device form ----
def test_device_form(R):
    hip = Hip()
    e = make_engine(R, ROWS, COLS, random_map(R, 0.2, 31))
    rng = np.random.default_rng(31)
    goals, seed = rng.choice(free_cells(e), 40), rng.integers(0, 9000, 40)
    check(e, goals, seed)
    host = downloads(e)
    check(e, goals, seed, device=hip)
    assert all(np.array_equal(a, b) for a, b in zip(host, downloads(e)))
    check(e, goals, None, device=hip)
    bad_goal, bad_seed = goals.copy(), seed.copy()
    bad_goal[13] = ROWS * COLS
    bad_seed[29] = LIMIT
    for g_, s_ in ((bad_goal, seed), (goals, bad_seed), (bad_goal, bad_seed)):
        d_g, d_s = hip.upload(g_.astype(np.int32)), hip.upload(s_.astype(np.int32))
        with pytest.raises(R.capi.RnaError, match="RNA_EINVAL"):
            e.goal_field_multi_device(d_g, d_s, 40, owners=True)
        assert e.goal_field_info()["goal"] == -1
        hip.free(d_g); hip.free(d_s)
        with pytest.raises(R.capi.RnaError, match="RNA_EINVAL"):
            e.goal_field_multi(g_, s_)
    check(e, goals, seed, device=hip)                                            # and the engine is as good as before
    e.close()


# ---- 11. without the flag ----
def test_without_the_flag(R):
    e = make_engine(R, ROWS, COLS, random_map(R, 0.1, 41))
    zero = {"sources": 0, "blocked_sources": 0, "terminals": 0, "owners": 0, "owner_rounds": 0}
    assert e.goal_field_sources_info() == zero and e.goal_field_owners_ptr() is None
    with pytest.raises(R.capi.RnaError, match="RNA_ESTATE"):
        e.goal_field_owners()
    free = free_cells(e)
    check(e, free[[5, 500, 900]], owners=False)
    assert e.goal_field_owners_ptr() is None
    for call in (e.goal_field_owners, lambda: e.goal_field_owners_at([3])):
        with pytest.raises(R.capi.RnaError, match="RNA_ESTATE"):
            call()
    check(e, free[[5, 500, 900]], owners=True)
    assert e.goal_field_owners_ptr() and e.goal_field_owners_at([-1, ROWS * COLS]).tolist() == [-1, -1]
    e.goal_field(int(free[5]))
    src = e.goal_field_sources_info()
    assert (src["sources"], src["owners"], src["owner_rounds"]) == (1, 0, 0) and e.goal_field_owners_ptr() is None
    with pytest.raises(R.capi.RnaError, match="RNA_ESTATE"):
        e.goal_field_owners()
    e.close()


# ---- 12. a snapshot ----
def test_snapshot_and_stale(R):
    master = door_map()
    e = make_engine(R, ROWS, COLS, master)
    e.upload(R.capi.LAYER_LASER, master)
    e.compose_master(1)
    goals, seed = [cell(20, 20), cell(100, 50), cell(70, 10)], [0, 700, 4000]
    check(e, goals, seed)
    old = downloads(e)
    rs = np.zeros(3, R.capi.RAY_DTYPE)                                           # close the door: a marking ray per door cell
    for k, j in enumerate((30, 31, 32)):
        rs["sx"][k], rs["sy"][k] = engine_centre(e, cell(70, j))
        rs["ex"][k], rs["ey"][k] = engine_centre(e, cell(66, j))
    e.update_map(rs, compose_mode=0)
    now = e.download(R.capi.LAYER_MASTER)
    assert (now[[cell(66, j) for j in (30, 31, 32)]] > 0).all()
    assert e.goal_field_info()["stale"] == 1
    assert all(np.array_equal(a, b) for a, b in zip(old, downloads(e)))
    w, _ = check(e, goals, seed)
    assert e.goal_field_info()["stale"] == 0 and not np.array_equal(w.owner, old[2])
    fresh = make_engine(R, ROWS, COLS, now)
    fresh.goal_field_multi(goals, seed, owners=True)
    assert all(np.array_equal(a, b) for a, b in zip(downloads(fresh), downloads(e)))
    fresh.close()
    e.close()


# ---- 13. / 14. the chains with the exploration frontiers ----
def explored_map(rows, cols, seed, rects=8, holes=12, specks=40):
    """unknown everywhere, known rectangles and two known bands across both tile borders at 64, obstacles, unknown holes"""
    rng = np.random.default_rng(seed)
    m = np.full((cols, rows), np.nan, np.float32)
    for _ in range(rects):
        w, h = rng.integers(20, 70, 2)
        i, j = rng.integers(0, rows - 20), rng.integers(0, cols - 20)
        m[j:j + h, i:i + w] = 0.0
    m[60:68, 5:rows - 5] = 0.0
    m[5:cols - 5, 60:68] = 0.0
    for _ in range(rects):
        w, h = rng.integers(1, 10, 2)
        i, j = rng.integers(0, rows - w), rng.integers(0, cols - h)
        m[j:j + h, i:i + w] = 180.0
    for _ in range(holes):
        w, h = rng.integers(1, 6, 2)
        i, j = rng.integers(0, rows - w), rng.integers(0, cols - h)
        m[j:j + h, i:i + w] = np.nan
    for _ in range(specks):
        m[rng.integers(0, cols), rng.integers(0, rows)] = 0.0
    return m


def known_free(e, R, k, seed):
    """k random cells that are known and free"""
    m = e.download(R.capi.LAYER_MASTER)
    ok = np.flatnonzero(~np.isnan(m) & (e.astar_blocked_mask() == 0))
    return np.random.default_rng(seed).choice(ok, k, replace=False)


def three_robots(e, R):
    """the known free cells nearest to the two ends of the known band along i and to one end of the band along j"""
    m = e.download(R.capi.LAYER_MASTER)
    ok = np.flatnonzero(~np.isnan(m) & (e.astar_blocked_mask() == 0))
    return np.array([ok[np.argmin((ok % ROWS - i) ** 2 + (ok // ROWS - j) ** 2)] for i, j in ((12, 64), (118, 64), (64, 8))])


def test_fleet_chain(R):
    e = make_engine(R, ROWS, COLS, explored_map(ROWS, COLS, 2).reshape(-1))
    robots = three_robots(e, R)
    w, _ = check(e, robots, [0, 2500, 800])
    recs, info = e.frontiers(rank=True)
    labels = e.frontier_labels()
    assert len(recs) >= 10
    owners_got = e.goal_field_owners_at(recs["nearest"])
    owning = set()
    for r, got in zip(recs, owners_got):
        cells = np.flatnonzero(labels == r["label"])
        cost = int(w.field[cells].min())
        nearest = int(cells[w.field[cells] == cost].min())
        assert (r["cost"], r["nearest"]) == (cost, nearest)
        assert got == w.owner[nearest]
        if cost < LIMIT:
            owning.add(int(w.owner[nearest]))
    assert len(owning) >= 2                                                      # at least two robots take frontiers
    e.close()


def test_nearest_frontier_chain(R):
    e = make_engine(R, ROWS, COLS, explored_map(ROWS, COLS, 3).reshape(-1))
    e.frontiers()
    labels = e.frontier_labels()
    ids, counts = np.unique(labels[labels >= 0], return_counts=True)
    want_cells = np.flatnonzero(np.isin(labels, ids[counts >= 3]))
    assert 0 < want_cells.size < (labels >= 0).sum()
    info, cells = e.goal_field_from_frontiers(min_size=3, owners=True)
    assert np.array_equal(cells, want_cells) and info["goal"] == want_cells[0]
    w = Want(e, want_cells)
    field, nx, own = downloads(e)
    assert np.array_equal(field, w.field) and np.array_equal(nx, w.next) and np.array_equal(own, w.owner)
    robots = known_free(e, R, 16, 6).astype(np.int32)
    paths, res = e.goal_field_paths(robots, 512)
    found = 0
    for k, s in enumerate(robots):
        assert res["cost"][k] == w.field[s]
        if w.field[s] < LIMIT:
            assert res["status"][k] == 0 and paths[k][res["path_len"][k] - 1] in want_cells
            assert paths[k][res["path_len"][k] - 1] == want_cells[w.owner[s]]
            found += 1
    assert found >= 8
    e.close()


# ---- 15. with a pipelined batch in flight ----
def test_coexists_with_a_pipelined_batch(R):
    hip = Hip()
    rows, cols = 192, 160
    master = R.synth.obstacles_rect(rows, cols, density=0.2, seed=2)
    e = make_engine(R, rows, cols, master)
    blocked, nbr = O.astar_masks(master, rows, cols)
    e.astar_pipeline_depth(2)
    e.astar_configure(max_queries=32)
    nq, max_len = 32, 2048
    q = R.synth.astar_queries(nq, master, rows, cols, seed=21)
    d_q, d_paths, d_res = hip.upload(q), hip.alloc(nq * max_len * 4), hip.alloc(nq * 24)
    e.astar_device(d_q, nq, d_paths, max_len, d_res)
    rng = np.random.default_rng(15)
    check(e, rng.choice(np.flatnonzero(blocked == 0), 12), rng.integers(0, 30000, 12))    # built while the batch is in flight
    e.synchronize()
    res = hip.download(d_res, R.capi.ASTAR_RESULT_DTYPE, nq)
    sp = hip.download(d_paths, np.int32, nq * max_len).reshape(nq, max_len)
    for k in range(nq):
        ores, opath, _ = O.astar_query(nbr, rows, cols, q["start"][k], q["goal"][k])
        assert (res["status"][k], res["path_len"][k], res["cost"][k]) == (ores.status, ores.path_len, ores.cost), k
        assert np.array_equal(sp[k][:ores.path_len], opath), k
    for p in (d_q, d_paths, d_res):
        hip.free(p)
    e.close()


# ---- 16. the C++ layer ----
def test_multi_goal_field_through_cpp(R, tmp_path):
    """tests/cpp/goal_field_multi_host_test.cpp builds the map of the case file, a GridGoalField from many goals with owners,
    and checks ownerOf, costToGoal, makePlan and assignFrontiers against the values written here (which check() has compared
    with the oracle)."""
    m = explored_map(ROWS, COLS, 2)
    e = make_engine(R, ROWS, COLS, m.reshape(-1))
    robots = three_robots(e, R)
    seed = [0, 2500, 800]
    w, _ = check(e, robots, seed)
    rng = np.random.default_rng(16)
    samples = np.concatenate([rng.integers(0, ROWS * COLS, 60), robots])
    paths, res = e.goal_field_paths(samples.astype(np.int32), 1024)
    recs, _ = e.frontiers(min_size=2, rank=True)
    order = np.lexsort((recs["label"], recs["cost"]))
    owners = e.goal_field_owners_at(recs["nearest"][order])
    assert len(set(owners.tolist()) - {-1}) >= 2
    lines = ["%d %d" % (ROWS, COLS), " ".join("nan" if np.isnan(v) else "%g" % v for v in m.reshape(-1)), "%d" % len(robots)]
    for c, s in zip(robots, seed):
        lines.append("%.17g %.17g %d" % (*engine_centre(e, int(c)), s))
    lines.append("%d" % len(samples))
    for k, c in enumerate(samples):
        ok = res["status"][k] == 0
        lines.append("%.17g %.17g %d %d %d" % (*engine_centre(e, int(c)), w.owner[c], res["cost"][k] if ok else -1, res["path_len"][k] if ok else 0))
    lines.append("%d" % len(owners))
    lines.append(" ".join(str(int(o)) for o in owners))
    case = tmp_path / "case.txt"
    case.write_text("\n".join(lines) + "\n")
    e.close()
    lib_dir = os.path.join(ROOT, "ros_navigation_amd")
    exe = str(tmp_path / "goal_field_multi_host_test")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "goal_field_multi_host_test.cpp"), "-o", exe,
                           "-I" + os.path.join(lib_dir, "host"), "-L" + lib_dir, "-lrna", "-Wl,-rpath," + lib_dir, "-lpthread"])
    run = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "goal field multi host OK" in run.stdout, run.stdout + run.stderr


# ---- 17. the fuzzer, a fixed seed and a short budget ----
def test_fuzz_goal_field_multi_fixed_seed():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fuzz_goal_field_multi.py"), "5", "305"], capture_output=True,
                         text=True, timeout=245, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-2000:])
    assert "fuzz ok" in out.stdout, out.stdout[-1000:]
    assert int(out.stdout.split("fuzz ok:")[1].split("fields")[0]) >= 3, out.stdout      # the budget went into builds, not start-up
