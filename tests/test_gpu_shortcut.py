"""GPU: line-of-sight shortcutting of cell paths (rna_shortcut_paths[_device], csrc/shortcut.hip), compared for equality --
way points, counts, blocked_steps, longest_span, statuses -- with the sequential rule of DESIGN.md section 4 written here in
plain Python:

    emit p[0]; a = 0
    while a < L-1:
        k = a + 1
        while k + 1 < L and (max_span == 0 or k + 1 - a <= max_span) and ok(a, k + 1): k += 1
        emit p[k]; a = k

line() comes from the oracle's og_line_cells_index (pinned to the reference's compiled LineIterator), the masks from
Engine.nbr_mask, clr from Engine.clearance_download, everything un-rotated to map space as tests/test_gpu_clearance.py does.
Maps are 130 x 70 cells: 3 x 2 ragged tiles, the smallest shape with tile borders and ragged edges in both directions."""
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
from _gpu import TABLE, Hip, R, make_engine, to_buffer, to_map  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.05
ROWS, COLS = 130, 70
ESTATE, EINVAL, ECAPACITY = -5, -1, -4
# neighbour number of the king move (di, dj) in the contract's order (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1)
MOVE = {(-1, -1): 0, (0, -1): 1, (1, -1): 2, (-1, 0): 3, (1, 0): 4, (-1, 1): 5, (0, 1): 6, (1, 1): 7}
MOVE_LUT = np.full((3, 3), 8, np.int64)          # [dj + 1, di + 1]
for (_di, _dj), _k in MOVE.items():
    MOVE_LUT[_dj + 1, _di + 1] = _k


def make(R, master=None, pos=(0.0, 0.0), rows=ROWS, cols=COLS):
    return make_engine(R, rows, cols, master, pos)


class Oracle:
    """the sequential definition over the engine's present masks (and clearance field), in map space"""

    def __init__(self, e, keep=False):
        g = e.geometry()
        self.rows, self.cols, self.s0, self.s1 = e.rows, e.cols, g.start_index[0], g.start_index[1]
        self.nbr = to_map(e.nbr_mask(), self.rows, self.cols, self.s0, self.s1).astype(np.int64)
        self.clr = to_map(e.clearance_download(), self.rows, self.cols, self.s0, self.s1).astype(np.int64) if keep else None
        self.memo = {}

    def cell(self, c):
        """buffer linear index -> map-space (i, j)"""
        return ((c % self.rows - self.s0) % self.rows, (c // self.rows - self.s1) % self.cols)

    def step_allowed(self, a, b):
        return bool((self.nbr[a[1], a[0]] >> MOVE[(b[0] - a[0], b[1] - a[1])]) & 1)

    def los(self, a, b):
        key = (a, b)
        if key not in self.memo:
            c = O.line_cells_index(a, b)
            ok = True
            if len(c) > 1:
                d = np.diff(c, axis=0)
                assert (np.abs(d).max(axis=1) == 1).all()
                k = MOVE_LUT[d[:, 1] + 1, d[:, 0] + 1]
                ok = bool((((self.nbr[c[:-1, 1], c[:-1, 0]] >> k) & 1) != 0).all())
            self.memo[key] = ok
        return self.memo[key]

    def line_clearance(self, a, b):
        c = O.line_cells_index(a, b)
        return int(self.clr[c[:, 1], c[:, 0]].min())

    def path_clearance(self, p, a, m):
        return min(int(self.clr[j, i]) for i, j in p[a:m + 1])

    def shortcut(self, row, in_status, path_len, max_len, max_span=0, keep=False):
        """-> (status, way points as buffer cells (all of them), blocked_steps, longest_span)"""
        if in_status != 0 or path_len < 1 or path_len > max_len:
            return 1, [], 0, 0
        cells = [int(c) for c in row[:path_len]]
        if any(c < 0 or c >= self.rows * self.cols for c in cells):
            return 2, [], 0, 0
        p = [self.cell(c) for c in cells]
        for a, b in zip(p[:-1], p[1:]):
            if (b[0] - a[0], b[1] - a[1]) not in MOVE:
                return 2, [], 0, 0
        blocked = sum(0 if self.step_allowed(a, b) else 1 for a, b in zip(p[:-1], p[1:]))

        def ok(a, m):
            if not self.los(p[a], p[m]):
                return False
            return not keep or self.line_clearance(p[a], p[m]) >= self.path_clearance(p, a, m)

        L = len(p)
        wp, longest, a = [cells[0]], 0, 0
        while a < L - 1:
            k = a + 1
            while k + 1 < L and (max_span == 0 or k + 1 - a <= max_span) and ok(a, k + 1):
                k += 1
            wp.append(cells[k])
            longest = max(longest, k - a)
            a = k
        return 0, wp, blocked, longest


def check(e, paths, results, max_span=0, keep=False, max_waypoints=None, oracle=None, got=None):
    """runs the shortcut (unless `got` = (waypoints, results) is given) and compares every row with the oracle; returns
    (waypoints, results, list of the oracle's way-point lists)"""
    ora = oracle or Oracle(e, keep)
    wp, out = got if got is not None else e.shortcut_paths(paths, results, max_span, keep, max_waypoints)
    n, max_len = paths.shape
    mw = wp.shape[1]
    wants = []
    for q in range(n):
        st, want, blocked, longest = ora.shortcut(paths[q], int(results["status"][q]), int(results["path_len"][q]), max_len, max_span, keep)
        r = out[q]
        wants.append(want)
        if st != 0:
            assert (r["status"], r["n_waypoints"], r["blocked_steps"], r["longest_span"]) == (st, 0, 0, 0), (q, r, st)
            assert (wp[q] == 0).all(), q
            continue
        assert r["status"] == (3 if len(want) > mw else 0), (q, r, len(want))
        assert (r["n_waypoints"], r["blocked_steps"], r["longest_span"]) == (len(want), blocked, longest), (q, r, len(want), blocked, longest)
        assert np.array_equal(wp[q][:min(mw, len(want))], want[:mw]), (q, wp[q][:len(want)].tolist(), want)
        assert (wp[q][len(want):] == 0).all(), q
        assert len(want) <= results["path_len"][q]
        if max_span:
            assert longest <= max_span
    return wp, out, wants


def legs_are_visible(ora, wants):
    """every leg of every answer passes the oracle's los (independent of how the oracle's loop found it), unless it is an
    original step of the path (always accepted)"""
    legs = 0
    for want in wants:
        for a, b in zip(want[:-1], want[1:]):
            ca, cb = ora.cell(a), ora.cell(b)
            if max(abs(cb[0] - ca[0]), abs(cb[1] - ca[1])) > 1:
                assert ora.los(ca, cb), (ca, cb)
                legs += 1
    return legs


def free_cells(e):
    return np.flatnonzero(e.astar_blocked_mask() == 0)


# ---- 1. empty map ----
def test_empty_map_gives_start_and_goal(R):
    e = make(R, np.zeros(ROWS * COLS, np.float32))
    q = np.zeros(3, R.capi.ASTAR_QUERY_DTYPE)
    q[0] = (0, ROWS * COLS - 1)                       # corner to corner
    q[1] = (777, 777)                                 # a one-cell path
    q[2] = (40 + 9 * ROWS, 41 + 10 * ROWS)            # a two-cell path
    res, paths = e.astar(q, 256)
    assert res["status"].tolist() == [0, 0, 0] and res["path_len"].tolist() == [130, 1, 2]
    wp, out, wants = check(e, paths, res)
    assert out["n_waypoints"].tolist() == [2, 1, 2] and out["longest_span"].tolist() == [129, 0, 1]
    assert wp[0][:2].tolist() == [0, ROWS * COLS - 1] and wp[1][0] == 777 and wp[2][:2].tolist() == [q[2]["start"], q[2]["goal"]]
    assert (out["blocked_steps"] == 0).all() and (out["status"] == 0).all()
    e.close()


# ---- 2. a wall with a door, random maps at two densities ----
def door_map():
    m = np.zeros((COLS, ROWS), np.float32)
    m[:, 64] = 180.0                                  # on the tile border
    m[30:32, 64] = 0.0
    return m


@pytest.mark.parametrize("kind", ["door", 0.1, 0.3])
def test_equal_to_the_oracle_on_64_queries(R, kind):
    if kind == "door":
        m = door_map()
    else:
        m = R.synth.obstacles_rect(ROWS, COLS, density=kind, seed=7, side=(2, 14)).reshape(COLS, ROWS).copy()
    m[50:58, 100:108] = 180.0                         # a closed pocket: no path out of it
    m[52:56, 102:106] = 0.0
    e = make(R, m.reshape(-1))
    free = np.flatnonzero(R.synth.free_component(m.reshape(-1), ROWS, COLS))
    q = np.zeros(64, R.capi.ASTAR_QUERY_DTYPE)
    q[:60] = R.synth.astar_queries(60, m.reshape(-1), ROWS, COLS, seed=3)
    q[60] = (-1, free[5])                             # invalid
    q[61] = (103 + 53 * ROWS, free[5])                # no path
    q[62] = (free[0], free[-1])
    q[63] = (free[9], free[9])
    max_len = int(np.sort(e.astar(q, 1024)[0]["path_len"])[-3])     # the two longest plans do not fit: too long
    res, paths = e.astar(q, max_len)
    assert {0, 1, 2, 3} <= set(res["status"].tolist()) and (res["status"] == 0).sum() >= 32
    ora = Oracle(e)
    for span in (0, 24):
        wp, out, wants = check(e, paths, res, max_span=span, oracle=ora)
        assert (out["status"][res["status"] != 0] == 1).all() and (out["status"][res["status"] == 0] == 0).all()
        assert legs_are_visible(ora, wants) >= 32
        assert (out["n_waypoints"] <= np.maximum(res["path_len"], 0))[res["status"] == 0].all()
        assert (out["blocked_steps"] == 0).all()
    assert out["n_waypoints"].max() >= 3              # plans that do have to turn
    e.close()


# ---- 3. the diagonal between two blocked cells that touch at a corner ----
def test_diagonal_between_two_touching_blocked_cells_is_not_taken(R):
    m = np.zeros((COLS, ROWS), np.float32)
    m[10, 10] = m[11, 11] = 180.0                     # m[j, i]
    e = make(R, m.reshape(-1))
    cells = [(9, 12), (9, 11), (9, 10), (9, 9), (10, 9), (11, 9), (12, 9)]      # round (10, 10) on its far side
    paths = np.zeros((1, 16), np.int32)
    paths[0, :len(cells)] = [i + j * ROWS for i, j in cells]
    res = np.zeros(1, R.capi.ASTAR_RESULT_DTYPE)
    res["path_len"] = len(cells)
    ora = Oracle(e)
    assert not ora.los((9, 12), (12, 9)) and not ora.los((10, 11), (11, 10))     # the pure diagonal squeezes between the two
    assert ora.nbr[11, 10] != 0 and ora.nbr[10, 11] != 0                          # ... although both of its inner cells are free
    wp, out, wants = check(e, paths, res, oracle=ora)
    assert out["n_waypoints"][0] > 2 and out["blocked_steps"][0] == 0
    assert legs_are_visible(ora, wants) >= 1
    e.close()


# ---- 4. the chunk edges of the speculative evaluation ----
@pytest.mark.parametrize("span", [0, 2, 3, 17, 63, 64, 65])
def test_max_span_at_the_chunk_edges(R, span):
    e = make(R, np.zeros(ROWS * COLS, np.float32))
    lens = (64, 65, 129, 130)
    q = np.zeros(len(lens), R.capi.ASTAR_QUERY_DTYPE)
    for k, n in enumerate(lens):
        q[k] = (0 + (20 + k) * ROWS, n - 1 + (20 + k) * ROWS)        # straight along i
    res, paths = e.astar(q, 130)
    assert res["path_len"].tolist() == list(lens) and (res["status"] == 0).all()
    wp, out, wants = check(e, paths, res, max_span=span)
    for k, n in enumerate(lens):
        legs = 1 if span == 0 else -(-(n - 1) // span)
        assert out["n_waypoints"][k] == legs + 1 and out["longest_span"][k] == (n - 1 if span == 0 else min(span, n - 1))
        if span:
            assert wp[k][:legs + 1].tolist() == [min(t * span, n - 1) + (20 + k) * ROWS for t in range(legs + 1)]
    e.close()


def test_a_staged_path_may_take_the_whole_lds(R):
    """max_path_len at RNA_SHORTCUT_MAX_PATH_LEN (160 KiB of LDS for the one workgroup) launches; one more is refused"""
    e = make(R, np.zeros(ROWS * COLS, np.float32))
    cap = R.capi.SHORTCUT_MAX_PATH_LEN
    paths = np.zeros((2, cap), np.int32)
    paths[0, :130] = np.arange(130) + 33 * ROWS
    j = np.arange(60)
    paths[1, :60] = 5 + j + (5 + j) * ROWS
    res = np.zeros(2, R.capi.ASTAR_RESULT_DTYPE)
    res["path_len"] = (130, 60)
    wp, out, wants = check(e, paths, res, max_waypoints=8)
    assert out["n_waypoints"].tolist() == [2, 2]
    big = np.zeros((1, cap + 1), np.int32)
    with pytest.raises(R.capi.RnaError, match="RNA_ECAPACITY"):
        e.shortcut_paths(big, res[:1], max_waypoints=8)
    e.close()


# ---- 5. max_waypoints too small ----
def test_max_waypoints_too_small(R):
    m = R.synth.obstacles_rect(ROWS, COLS, density=0.3, seed=7, side=(2, 14))
    e = make(R, m)
    q = R.synth.astar_queries(32, m, ROWS, COLS, seed=5)
    res, paths = e.astar(q, 256)
    ora = Oracle(e)
    full, out_full, wants = check(e, paths, res, oracle=ora)
    assert out_full["n_waypoints"].max() >= 5
    wp, out, _ = check(e, paths, res, max_waypoints=3, oracle=ora)
    over = out_full["n_waypoints"] > 3
    assert over.any() and (~over).any()
    assert (out["status"][over] == 3).all() and (out["status"][~over] == 0).all()
    assert np.array_equal(out["n_waypoints"], out_full["n_waypoints"]) and np.array_equal(wp, full[:, :3])
    e.close()


# ---- 6. robot radius ----
def test_robot_radius(R):
    m = R.synth.obstacles_rect(ROWS, COLS, density=0.1, seed=11, side=(2, 10))
    e = make(R, m)
    n_plain = int(e.astar_blocked_mask().sum())
    e.astar_robot_radius(0.15)
    assert int(e.astar_blocked_mask().sum()) > n_plain
    free = free_cells(e)
    rng = np.random.default_rng(4)
    q = np.zeros(48, R.capi.ASTAR_QUERY_DTYPE)
    q["start"], q["goal"] = rng.choice(free, 48), rng.choice(free, 48)
    res, paths = e.astar(q, 256)
    assert (res["status"] == 0).sum() >= 24
    ora = Oracle(e)
    wp, out, wants = check(e, paths, res, oracle=ora)
    assert legs_are_visible(ora, wants) >= 24 and out["n_waypoints"].max() >= 3
    e.close()


# ---- 7. a moved map: paths across the buffer seam; 9. hand-made rows ----
def moved_engine(R):
    e = make(R, np.zeros(ROWS * COLS, np.float32), pos=(1.25, -2.5))
    assert e.move(1.25 + 37 * RES, -2.5 - 22 * RES)
    g = e.geometry()
    s0, s1 = g.start_index[0], g.start_index[1]
    assert s0 % 64 != 0 and s1 % 64 != 0 and s0 != 0 and s1 != 0
    # map cell (i, j) sits at buffer ((i + s0) % rows, (j + s1) % cols): the seam lies between map rows - s0 - 1 | rows - s0
    si, sj = ROWS - s0, COLS - s1
    m = np.zeros((COLS, ROWS), np.float32)
    rng = np.random.default_rng(9)
    for _ in range(14):
        w, h = rng.integers(2, 12, 2)
        i, j = rng.integers(0, ROWS - w), rng.integers(0, COLS - h)
        m[j:j + h, i:i + w] = 180.0
    m[sj - 6:sj + 6, si - 1:si + 2] = 180.0              # a block across both seams
    e.upload(R.capi.LAYER_MASTER, to_buffer(m, ROWS, COLS, s0, s1))
    return e, m, s0, s1, si, sj


def test_moved_map_paths_across_the_seam(R):
    e, m, s0, s1, si, sj = moved_engine(R)
    buf = lambda i, j: (i + s0) % ROWS + ((j + s1) % COLS) * ROWS
    rng = np.random.default_rng(2)
    fj, fi = np.nonzero(m == 0)
    left = [k for k in range(len(fi)) if fi[k] < si - 20 and fj[k] < sj - 10]
    right = [k for k in range(len(fi)) if fi[k] > si + 20 and fj[k] > sj + 10]
    q = np.zeros(32, R.capi.ASTAR_QUERY_DTYPE)
    for k in range(32):
        a, b = rng.choice(left), rng.choice(right)
        q[k] = (buf(fi[a], fj[a]), buf(fi[b], fj[b])) if k % 2 else (buf(fi[b], fj[b]), buf(fi[a], fj[a]))
    res, paths = e.astar(q, 256)
    assert (res["status"] == 0).sum() >= 24
    p0 = paths[0][:res["path_len"][0]]
    assert np.abs(np.diff(p0 % ROWS)).max() > 1 and np.abs(np.diff(p0 // ROWS)).max() > 1      # the buffer seam is crossed both ways
    ora = Oracle(e)
    assert (ora.s0, ora.s1) == (s0, s1)
    for span in (0, 40):
        wp, out, wants = check(e, paths, res, max_span=span, oracle=ora)
    assert legs_are_visible(ora, wants) >= 24 and out["n_waypoints"].max() >= 3
    e.close()


def test_hand_made_rows_are_refused_without_harm(R):
    e, m, s0, s1, si, sj = moved_engine(R)
    buf = lambda i, j: (i + s0) % ROWS + ((j + s1) % COLS) * ROWS
    fj, fi = np.nonzero(m == 0)
    q = np.zeros(3, R.capi.ASTAR_QUERY_DTYPE)
    q[0] = (buf(fi[0], fj[0]), buf(fi[-1], fj[-1]))
    q[1] = (buf(fi[-1], fj[-1]), buf(fi[40], fj[40]))
    q[2] = (buf(fi[300], fj[300]), buf(fi[-300], fj[-300]))
    res3, paths3 = e.astar(q, 256)
    assert (res3["status"] == 0).all() and res3["path_len"].min() > 8
    paths = np.zeros((8, 256), np.int32)
    res = np.zeros(8, R.capi.ASTAR_RESULT_DTYPE)
    for k, src in ((0, 0), (2, 1), (7, 2)):               # good rows between the bad ones
        paths[k], res[k] = paths3[src], res3[src]
    for k in (1, 3, 4, 5, 6):
        paths[k], res[k] = paths3[0], res3[0]
    n0 = int(res3["path_len"][0])
    paths[1, n0 - 1] = ROWS * COLS                        # a cell >= n_cells (the last one of the path)
    paths[3, 0] = -7                                      # a negative cell
    c = paths3[0][4]
    ci, cj = (c % ROWS - s0) % ROWS, (c // ROWS - s1) % COLS
    paths[4, 5] = buf(ci + 2 if ci + 2 < ROWS else ci - 2, cj)        # a two-cell jump
    paths[5, :2] = (buf(ci, cj), buf(ci, cj))             # the same cell twice is no king move
    res[5]["path_len"] = 2
    paths[6, :2] = ((s0 - 1) + 20 * ROWS, s0 + 20 * ROWS)  # neighbours in the buffer, map i = rows - 1 and 0
    res[6]["path_len"] = 2
    ora = Oracle(e)
    assert ora.cell(int(paths[6, 0]))[0] == ROWS - 1 and ora.cell(int(paths[6, 1]))[0] == 0
    wp, out, wants = check(e, paths, res, oracle=ora)
    assert out["status"].tolist() == [0, 2, 0, 2, 2, 2, 2, 0]
    paths[6, :2] = (buf(si - 1, 3), buf(si, 3))           # ... while neighbours across the seam in map space are fine
    assert abs(int(paths[6, 0]) % ROWS - int(paths[6, 1]) % ROWS) == ROWS - 1
    wp, out, wants = check(e, paths, res, oracle=ora)
    assert out["status"].tolist() == [0, 2, 0, 2, 2, 2, 0, 0] and out["n_waypoints"][6] == 2
    e.close()


# ---- 8. an obstacle lands on a finished path ----
def test_blocked_steps_after_a_map_update(R):
    m = R.synth.obstacles_rect(ROWS, COLS, density=0.1, seed=7, side=(2, 14)).copy()
    e = make(R, m)
    q = R.synth.astar_queries(16, m, ROWS, COLS, seed=8)
    res, paths = e.astar(q, 256)
    assert (res["status"] == 0).all()
    wp0, out0, _ = check(e, paths, res)
    assert (out0["blocked_steps"] == 0).all()
    k = int(np.argmax(res["path_len"]))
    mid = paths[k][res["path_len"][k] // 2]
    m[mid] = 180.0                                        # buffer order == map order on an unmoved map
    m[paths[k][res["path_len"][k] // 2 + 7]] = 180.0
    e.upload(R.capi.LAYER_MASTER, m)
    wp, out, wants = check(e, paths, res)                 # the call refreshes the masks itself
    assert out["blocked_steps"][k] >= 2 and (out["status"] == 0).all()
    assert not np.array_equal(wp[k], wp0[k])
    e.close()


# ---- 10. keep_clearance ----
def test_keep_clearance(R):
    m = np.zeros((COLS, ROWS), np.float32)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 180.0
    m[35, 0:100] = 180.0                                  # a wall along j = 35 with its tip at i = 99: the way round is a U-turn
    m[12:20, 40:50] = 180.0                               # and something to steer round in each corridor
    m[48:60, 60:66] = 180.0
    e = make(R, m.reshape(-1))
    paths1 = np.zeros((1, 8), np.int32)
    paths1[0, :3] = (10 + 30 * ROWS, 11 + 30 * ROWS, 12 + 30 * ROWS)
    res1 = np.zeros(1, R.capi.ASTAR_RESULT_DTYPE)
    res1["path_len"] = 3
    wp1, out1 = np.zeros((1, 8), np.int32), np.zeros(1, R.capi.SHORTCUT_RESULT_DTYPE)
    args = (paths1.ctypes.data, res1.ctypes.data, 1, 8, 0, 1, wp1.ctypes.data, 8, out1.ctypes.data)
    assert e._L.rna_shortcut_paths(e.h, *args) == ESTATE              # no clearance field: nothing is built behind the caller's back
    assert e.clearance_info() == (0, False)
    e.goal_field_clearance_cost(TABLE)
    goal = 10 + 40 * ROWS
    e.goal_field(goal)
    assert e.clearance_info() == (7, False)
    rng = np.random.default_rng(6)
    free = free_cells(e)
    starts = np.concatenate([[10 + 30 * ROWS, 100 + 10 * ROWS, 30 + 5 * ROWS], rng.choice(free, 29)]).astype(np.int32)
    paths, res = e.goal_field_paths(starts, 512)
    assert (res["status"] == 0).all()
    ora = Oracle(e, keep=True)
    plain, out_plain, wants_plain = check(e, paths, res, oracle=ora)
    kept, out_kept, wants_kept = check(e, paths, res, keep=True, oracle=ora)
    check(e, paths, res, max_span=30, keep=True, oracle=ora)
    differ = [q for q in range(len(starts)) if wants_plain[q] != wants_kept[q]]
    assert differ                                         # the plain shortcut cuts back towards the walls somewhere
    for q, want in enumerate(wants_kept):                 # no leg comes closer to an obstacle than the piece it replaces
        cells = [int(c) for c in paths[q][:res["path_len"][q]]]
        p = [ora.cell(c) for c in cells]
        at = 0
        for a, b in zip(want[:-1], want[1:]):
            ia = cells.index(a, at)
            ib = cells.index(b, ia + 1)
            assert ora.line_clearance(p[ia], p[ib]) >= ora.path_clearance(p, ia, ib), (q, a, b)
            at = ib
    e.upload(R.capi.LAYER_MASTER, m.reshape(-1))          # a call that can change the masks: the field is stale
    assert e.clearance_info() == (7, True)
    assert e._L.rna_shortcut_paths(e.h, *args) == ESTATE
    assert e._L.rna_shortcut_paths(e.h, *(args[:5] + (0,) + args[6:])) == 0 and out1["n_waypoints"][0] == 2
    e.close()


# ---- 11. device pointers: chained behind the goal field's paths, and next to a pipelined batch ----
def test_device_form_chains_behind_the_goal_field_paths(R):
    hip = Hip()
    m = R.synth.obstacles_rect(ROWS, COLS, density=0.3, seed=7, side=(2, 14))
    e = make(R, m)
    free = np.flatnonzero(R.synth.free_component(m, ROWS, COLS))
    e.goal_field(int(free[len(free) // 2]))
    rng = np.random.default_rng(12)
    n, max_len, mw = 64, 256, 40
    starts = rng.choice(free, n).astype(np.int32)
    starts[5] = -3
    d_s, d_paths, d_res = hip.upload(starts), hip.alloc(n * max_len * 4, zero=True), hip.alloc(n * 24, zero=True)
    d_wp, d_out = hip.alloc(n * mw * 4, zero=True), hip.alloc(n * 16, zero=True)
    e.goal_field_paths_device(d_s, n, d_paths, max_len, d_res)
    e.shortcut_paths_device(d_paths, d_res, n, max_len, d_wp, mw, d_out, max_span=50)       # no synchronisation in between
    e.synchronize_map()
    paths, res = e.goal_field_paths(starts, max_len)
    assert (res["status"] == 0).sum() == n - 1 and res["status"][5] == 2
    wp, out, _ = check(e, paths, res, max_span=50, max_waypoints=mw)
    assert np.array_equal(hip.download(d_out, R.capi.SHORTCUT_RESULT_DTYPE, n), out)
    assert np.array_equal(hip.download(d_wp, np.int32, n * mw).reshape(n, mw), wp)
    for p in (d_s, d_paths, d_res, d_wp, d_out):
        hip.h.hipFree(p)
    e.close()


def test_a_call_while_a_pipelined_batch_is_in_flight(R):
    hip = Hip()
    rows = cols = 512
    m = R.synth.obstacles_rect(rows, cols, density=0.3, seed=2)
    e = make(R, m, rows=rows, cols=cols)
    e.astar_pipeline_depth(4)
    e.astar_configure(max_queries=64)
    nq, max_len = 64, 2048
    q0 = R.synth.astar_queries(8, m, rows, cols, seed=30)
    res0, paths0 = e.astar(q0, max_len)
    assert (res0["status"] == 0).all()
    issued = []
    # every buffer is allocated and zeroed before the first batch goes out: hipMemset runs on the null stream, which waits
    # for searches in flight -- issued between two batches it would land after the chained kernel's first answers
    bufs = []
    for b in range(2):
        q = R.synth.astar_queries(nq, m, rows, cols, seed=20 + b)
        bufs.append((q, hip.upload(q), hip.alloc(nq * max_len * 4, zero=True), hip.alloc(nq * 24, zero=True),
                     hip.alloc(nq * 64 * 4, zero=True), hip.alloc(nq * 16, zero=True)))
    assert hip.h.hipDeviceSynchronize() == 0
    for q, d_q, d_paths, d_res, d_wp1, d_out1 in bufs:
        e.astar_device(d_q, nq, d_paths, max_len, d_res)
        # chained behind the batch without the host seeing a path or waiting: the engine's stream waits for the search
        e.shortcut_paths_device(d_paths, d_res, nq, max_len, d_wp1, 64, d_out1, max_span=64)
        issued.append((q, d_q, d_paths, d_res, d_wp1, d_out1))
    wp, out = e.shortcut_paths(paths0, res0, max_span=64, max_waypoints=64)          # while the two batches are in flight
    e.synchronize()
    check(e, paths0, res0, max_span=64, max_waypoints=64, got=(wp, out))
    blocked, nbr = O.astar_masks(m, rows, cols)
    for q, d_q, d_paths, d_res, d_wp1, d_out1 in issued:  # the batches were not disturbed
        res = hip.download(d_res, R.capi.ASTAR_RESULT_DTYPE, nq)
        sp = hip.download(d_paths, np.int32, nq * max_len).reshape(nq, max_len)
        for k in range(0, nq, 8):
            ores, opath, _ = O.astar_query(nbr, rows, cols, q["start"][k], q["goal"][k])
            assert (res["status"][k], res["path_len"][k], res["cost"][k]) == (ores.status, ores.path_len, ores.cost), k
            assert np.array_equal(sp[k][:ores.path_len], opath), k
        # the same call once everything has settled gives what the chained one gave, and both are the oracle's
        d_wp, d_out = hip.alloc(nq * 64 * 4, zero=True), hip.alloc(nq * 16, zero=True)
        e.shortcut_paths_device(d_paths, d_res, nq, max_len, d_wp, 64, d_out, max_span=64)
        e.synchronize_map()
        got = (hip.download(d_wp, np.int32, nq * 64).reshape(nq, 64), hip.download(d_out, R.capi.SHORTCUT_RESULT_DTYPE, nq))
        chained = (hip.download(d_wp1, np.int32, nq * 64).reshape(nq, 64), hip.download(d_out1, R.capi.SHORTCUT_RESULT_DTYPE, nq))
        assert np.array_equal(chained[1], got[1]) and np.array_equal(chained[0], got[0])
        assert (got[1]["status"][res["status"] == 0] != 1).all()
        check(e, sp[:16], res[:16], max_span=64, got=(got[0][:16], got[1][:16]))
        for p in (d_q, d_paths, d_res, d_wp, d_out, d_wp1, d_out1):
            hip.h.hipFree(p)
    e.close()


# ---- 12. the C++ layer ----
def test_shortcut_plan_and_set_shortcut_through_cpp(R, tmp_path):
    """tests/cpp/shortcut_host_test.cpp plans on the door map through GridAStarPlanner / GridGoalField with and without
    setShortcut and through shortcutPlan, and prints the cells of what it got; the same plans through the Python engine and
    the oracle here."""
    lib_dir = os.path.join(ROOT, "ros_navigation_amd")             # (librna.so is there: the R fixture has loaded it)
    exe = str(tmp_path / "shortcut_host_test")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "shortcut_host_test.cpp"), "-o", exe,
                           "-I" + os.path.join(ROOT, "ros_navigation_amd", "host"), "-L" + lib_dir, "-lrna", "-Wl,-rpath," + lib_dir,
                           "-lpthread"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "shortcut host OK" in run.stdout, run.stdout + run.stderr
    got = {}
    for ln in run.stdout.splitlines():
        if ":" in ln:
            name, cells = ln.split(":")
            got[name] = [int(v) for v in cells.split()]
    m = door_map()
    m[10:40, 30:34] = 180.0
    m[35:69, 95:99] = 180.0
    e = make(R, m.reshape(-1))
    start, goal = 5 + 60 * ROWS, 120 + 8 * ROWS
    assert got["query"] == [start, goal]
    q = np.zeros(1, R.capi.ASTAR_QUERY_DTYPE)
    q[0] = (start, goal)
    res, paths = e.astar(q, 1024)
    ora = Oracle(e)
    full = paths[0][:res["path_len"][0]].tolist()
    assert got["plan"] == full
    for name, span in (("shortcut", 0), ("shortcut17", 17)):
        st, want, blocked, longest = ora.shortcut(paths[0], 0, len(full), 1024, span)
        assert st == 0 and got[name] == want and len(want) < len(full) // 4, name
    assert got["planner"] == got["shortcut"] and got["planner_off"] == full
    e.goal_field(goal)
    gp, gres = e.goal_field_paths(np.array([start], np.int32), 1024)
    st, want, blocked, longest = ora.shortcut(gp[0], 0, int(gres["path_len"][0]), 1024, 0)
    assert got["field"] == want and got["blocked"] == [0]
    e.clearance(7)
    ora = Oracle(e, keep=True)
    st, want, blocked, longest = ora.shortcut(paths[0], 0, len(full), 1024, 0, keep=True)
    assert got["keep"] == want
    e.close()
