"""Scan matching on the GPU (rna_scan_match, csrc/scanmatch.hip) against an oracle written here in plain numpy from the
definition of include/rna.h: un-rotate master to map space, dilate the occupied array (padded with False) to the bit_l, add them
to w, evaluate the point, rotation and cell formulas literally in 64-bit integers, sum w over the used points for every
(rotation, db, da), and pick the best by the stated order.  Integers only: every record and every volume is compared for
equality.

The maps are 96 x 80 cells (non-square, smaller than the largest window, so that R = 127 overhangs all four sides), plain and
moved by a non-multiple of 64 in both axes."""
import importlib.util
import os

import numpy as np
import pytest

from _gpu import Hip, R, engine_centre, make_engine, to_buffer, to_map  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu

RES = 0.05
RNA_ECAPACITY = -4
ROWS, COLS = 96, 80
CHUNK = 2048                       # points the kernel stages per turn (csrc/scanmatch.hip SM_CHUNK)
EXACT = ((16384, 0), (0, 16384), (-16384, 0), (0, -16384))
STEP = 0.06                        # rotation step of the planted-pose test (rad)


# ---- the oracle ----
class Want:
    """the definition's answer for a master layer in map order ([j, i]); Want.of(e, R) takes the engine's present one"""
    PAD = 4

    def __init__(self, m):
        m = np.asarray(m, np.float32)
        self.cols, self.rows = m.shape
        self.occupied = ~np.isnan(m) & (m > 0)
        self._w = {}

    @classmethod
    def of(cls, e, R):
        g = e.geometry()
        w = cls(to_map(e.download(R.capi.LAYER_MASTER), e.rows, e.cols, g.start_index[0], g.start_index[1]))
        w.s0, w.s1 = g.start_index[0], g.start_index[1]
        return w

    s0 = s1 = 0

    def buffer_cell(self, i, j):
        return ((j + self.s1) % self.cols) * self.rows + (i + self.s0) % self.rows

    def map_cell(self, c):
        return (c % self.rows - self.s0) % self.rows, (c // self.rows - self.s1) % self.cols

    def w(self, L):
        """w = sum of bit_0 .. bit_(L-1) over the map padded by PAD cells of False ([j + PAD, i + PAD]); zero beyond"""
        if L not in self._w:
            P = self.PAD
            bit = np.zeros((self.cols + 2 * P, self.rows + 2 * P), bool)
            bit[P:-P, P:-P] = self.occupied
            total = bit.astype(np.int64)
            for _ in range(1, L):
                grown = np.zeros_like(bit)
                for dj in (-1, 0, 1):
                    for di in (-1, 0, 1):
                        grown[max(dj, 0):bit.shape[0] + min(dj, 0), max(di, 0):bit.shape[1] + min(di, 0)] |= \
                            bit[max(-dj, 0):bit.shape[0] + min(-dj, 0), max(-di, 0):bit.shape[1] + min(-di, 0)]
                bit = grown
                total += bit
            self._w[L] = total
        return self._w[L]

    def w_at(self, L, a, b):
        wm, P = self.w(L), self.PAD
        inside = (a >= -P) & (a < self.rows + P) & (b >= -P) & (b < self.cols + P)
        return np.where(inside, wm[np.clip(b + P, 0, wm.shape[0] - 1), np.clip(a + P, 0, wm.shape[1] - 1)], 0)

    def match(self, query, points, rot, Rc, T, L):
        """(record tuple, volume [n_rot, 2T + 1, 2T + 1]) of one query; rot = its [n_rot, 2] pairs"""
        n_rot = len(rot)
        rc = n_rot // 2
        S = 2 * T + 1
        vol = np.zeros((n_rot, S, S), np.int64)
        cell = int(query["cell"])
        if cell < 0 or cell >= self.rows * self.cols:
            return (1, 0, rc, 0, 0, 0, 0, 0), vol
        off, n = int(query["points_offset"]), int(query["n_points"])
        p = np.asarray(points, np.int64).reshape(-1, 2)[off:off + n]
        px, py = p[:, 0], p[:, 1]
        used = (np.abs(px) <= 32767) & (np.abs(py) <= 32767) & (px * px + py * py <= (64 * Rc) ** 2)
        px, py = px[used], py[used]
        n_used = int(used.sum())
        if n_used == 0:
            return (2, 0, rc, 0, 0, 0, 0, 0), vol
        gi, gj = self.map_cell(cell)
        sub0, sub1 = int(query["sub"][0]), int(query["sub"][1])
        d = np.arange(-T, T + 1, dtype=np.int64)
        for r in range(n_rot):
            c, s = int(rot[r][0]), int(rot[r][1])
            qx = (c * px - s * py + 8192) >> 14
            qy = (s * px + c * py + 8192) >> 14
            oa, ob = (qx + sub0 + 32) >> 6, (qy + sub1 + 32) >> 6
            near = (np.abs(oa) <= Rc + 1) & (np.abs(ob) <= Rc + 1)      # (always, for a pair of magnitude 16384 and sub in range)
            a, b = gi + oa[near], gj + ob[near]
            vol[r] = self.w_at(L, a[:, None, None] + d[None, None, :], b[:, None, None] + d[None, :, None]).sum(axis=0)
        rr, db, da = np.meshgrid(np.arange(n_rot), d, d, indexing="ij")
        order = np.lexsort((da.ravel(), db.ravel(), rr.ravel(), np.abs(rr - rc).ravel(), (da * da + db * db).ravel(), -vol.ravel()))
        k = order[0]
        best = (0, int(vol.ravel()[k]), int(rr.ravel()[k]), int(da.ravel()[k]), int(db.ravel()[k]), n_used, int(vol[rc, T, T]), n_used * L)
        return best, vol


def as_tuples(recs):
    return [(int(r["status"]), int(r["score"]), int(r["rot"]), int(r["shift"][0]), int(r["shift"][1]), int(r["n_used"]),
             int(r["score_guess"]), int(r["score_max"])) for r in recs]


def check(e, R, queries, points, rot, Rc, T, L, want=None):
    """the host form with its volume, compared with the oracle; returns (oracle, record tuples, volume)"""
    w = want if want is not None else Want.of(e, R)
    queries = np.asarray(queries, R.capi.SCAN_MATCH_QUERY_DTYPE)
    rot = np.asarray(rot, np.int32).reshape(len(queries), -1, 2)
    recs, vol = e.scan_match(queries, points, rot, Rc, T, L, volume=True)
    plain = e.scan_match(queries, points, rot, Rc, T, L)
    assert plain.tobytes() == recs.tobytes()                       # the volume is optional, the records do not depend on it
    got = as_tuples(recs)
    for k in range(len(queries)):
        rec, v = w.match(queries[k], points, rot[k], Rc, T, L)
        assert np.array_equal(vol[k], v), (k, np.argwhere(vol[k] != v)[:5], vol[k][vol[k] != v][:5], v[vol[k] != v][:5])
        assert got[k] == rec, (k, got[k], rec)
    return w, got, vol


# ---- the maps ([j, i] arrays), the queries, the points, the rotations ----
def rooms_map(rows=ROWS, cols=COLS, seed=1, edges=True):
    """random rooms (rectangle outlines) with NaN patches and a sprinkle of single occupied cells; with `edges` occupied
    cells in rows 0 and rows - 1 and in columns 0 and cols - 1, corners included; one full line along each axis puts occupied
    bits on both sides of every 32-bit word boundary of whatever window is laid over the map"""
    rng = np.random.default_rng(seed)
    m = np.zeros((cols, rows), np.float32)
    for _ in range(7):
        i0, j0 = int(rng.integers(0, rows - 8)), int(rng.integers(0, cols - 8))
        i1, j1 = min(rows - 1, i0 + int(rng.integers(6, 40))), min(cols - 1, j0 + int(rng.integers(6, 40)))
        m[j0, i0:i1 + 1] = m[j1, i0:i1 + 1] = 180.0
        m[j0:j1 + 1, i0] = m[j0:j1 + 1, i1] = 180.0
    m[rng.random((cols, rows)) < 0.01] = 90.0
    for _ in range(4):
        i0, j0 = int(rng.integers(0, rows - 5)), int(rng.integers(0, cols - 5))
        m[j0:j0 + int(rng.integers(2, 9)), i0:i0 + int(rng.integers(2, 9))] = np.nan
    m[int(rng.integers(5, cols - 5)), :] = 180.0
    m[:, int(rng.integers(5, rows - 5))] = 180.0
    if edges:
        for i, j in ((0, 0), (rows - 1, 0), (0, cols - 1), (rows - 1, cols - 1), (0, 31), (0, 32), (rows - 1, 50), (31, 0), (32, 0), (63, cols - 1),
                     (64, cols - 1)):
            m[j, i] = 180.0
    return m


def engines(R, m):
    """the map on an unmoved engine, then on one moved by 37 and 22 cells (no multiples of 64): [(engine, oracle)]"""
    cols, rows = m.shape
    out = []
    e = make_engine(R, rows, cols, m.reshape(-1))
    out.append((e, Want.of(e, R)))
    e = make_engine(R, rows, cols, np.zeros(rows * cols, np.float32), pos=(1.25, -2.5))
    assert e.move(1.25 + 37 * RES, -2.5 - 22 * RES)
    g = e.geometry()
    s0, s1 = g.start_index[0], g.start_index[1]
    assert s0 % 64 != 0 and s1 % 64 != 0
    e.upload(R.capi.LAYER_MASTER, to_buffer(m, rows, cols, s0, s1))
    w = Want.of(e, R)
    assert np.array_equal(w.occupied, ~np.isnan(m) & (m > 0)) and w.buffer_cell(rows - s0, cols - s1) == 0
    out.append((e, w))
    return out


def random_points(rng, n, Rc):
    """n points: most inside the disc of 64 Rc units, negative and positive coordinates round zero (the floor of the
    arithmetic shifts), some beyond the disc and some beyond 32767 (both dropped)"""
    p = rng.integers(-64 * Rc, 64 * Rc + 1, (n, 2))
    small = rng.random(n) < 0.15
    p[small] = rng.integers(-70, 71, (int(small.sum()), 2))
    far = rng.random(n) < 0.05
    p[far] = rng.integers(-40000, 40001, (int(far.sum()), 2))
    huge = rng.random(n) < 0.02
    p[huge] = rng.choice([-(1 << 30), 32768, -32768, 1 << 30, 70000], (int(huge.sum()), 2))
    return p.astype(np.int32)


def rotations(rng, n, n_rot):
    """[n, n_rot, 2]: general angles a small step apart round a random yaw, with the four exact pairs mixed in"""
    rot = np.zeros((n, n_rot, 2), np.int32)
    for q in range(n):
        yaw, step = rng.uniform(-np.pi, np.pi), rng.uniform(0.002, 0.03)
        ang = yaw + (np.arange(n_rot) - n_rot // 2) * step
        rot[q, :, 0], rot[q, :, 1] = np.rint(16384 * np.cos(ang)), np.rint(16384 * np.sin(ang))
        for k in rng.integers(0, n_rot, min(4, n_rot)):
            rot[q, k] = EXACT[int(rng.integers(0, 4))]
    return rot


def batch(w, rng, counts, Rc, n_rot, at):
    """one query per entry of `counts` at the map cells `at` (cycled), sub cycling through (-32, -32), (31, 31) and random"""
    queries = np.zeros(len(counts), "i4, (2,)i4, i4, i4")
    pts, off = [], 0
    for k, n in enumerate(counts):
        i, j = at[k % len(at)]
        sub = ((-32, -32), (31, 31), tuple(int(v) for v in rng.integers(-32, 32, 2)))[k % 3]
        queries[k] = (w.buffer_cell(i, j), sub, off, n)
        pts.append(random_points(rng, n, Rc))
        off += n
    queries.dtype.names = ("cell", "sub", "points_offset", "n_points")
    return queries, np.concatenate(pts).reshape(-1, 2), rotations(rng, len(counts), n_rot)


# ---- 1. window reach x shifts x levels x rotation counts x point counts, on the plain and on the moved map ----
@pytest.mark.parametrize("Rc,T,L,n_rot", [(127, 16, 4, 1), (127, 1, 2, 2), (127, 0, 3, 41), (40, 16, 1, 2), (40, 1, 4, 41), (40, 0, 2, 1),
                                          (1, 16, 2, 1), (1, 1, 1, 41), (1, 0, 4, 2),
                                          # 2, 3 and 4 candidate slots per thread ((2T + 1)^2 = 289, 529, 841 over 256 threads)
                                          (40, 8, 3, 2), (40, 11, 3, 2), (40, 14, 3, 1)])
def test_windows_shifts_levels_and_rotations(R, Rc, T, L, n_rot):
    m = rooms_map(seed=3)
    corners_and_centre = [(0, 0), (ROWS - 1, 0), (0, COLS - 1), (ROWS - 1, COLS - 1), (ROWS // 2, COLS // 2), (33, 17)]
    counts = [0, 1, CHUNK, CHUNK + 1, 8192, 300] if n_rot <= 2 else [0, 1, CHUNK + 1, 300, 64, 65]
    for e, w in engines(R, m):
        rng = np.random.default_rng(100 * Rc + 10 * T + L)
        queries, points, rot = batch(w, rng, counts, Rc, n_rot, corners_and_centre)
        if Rc == 127:      # the window leaves the map on all four sides at once, from every guess cell
            H = Rc + 1 + T + (L - 1)
            assert all(i - H < 0 and j - H < 0 and i + H >= ROWS and j + H >= COLS for i, j in corners_and_centre)
        _, got, vol = check(e, R, queries, points, rot, Rc, T, L, w)
        assert got[0][0] == 2 and not vol[0].any()                                      # n_points == 0: no used point
        assert all(g[0] == 0 for g in got[2:]) and all(0 < g[5] < n for g, n in zip(got[2:], counts[2:]))      # some points were dropped
        assert all(g[1] >= g[6] and g[1] <= g[7] and g[7] == g[5] * L for g in got[2:])
        if Rc >= 40:
            assert any(g[1] > 0 for g in got[2:])
        e.close()


# ---- 2. a planted pose comes back exactly ----
@pytest.mark.parametrize("Rc,T,L,turn,plant", [(40, 16, 3, 1, (16, -16)), (127, 5, 4, 3, (-5, 2)), (20, 1, 1, 0, (1, 1)), (30, 8, 2, 2, (0, -7))])
def test_planted_pose(R, Rc, T, L, turn, plant):
    """points = the cell centres of the occupied cells within Rc of a true cell, turned back by one of the four exact
    rotations; the guess is off by `plant` cells and by two rotation slots: the match is that shift and that slot, with every
    point on an occupied cell"""
    m = rooms_map(seed=11, edges=False)
    ti, tj = 50, 37
    m[tj - 1:tj + 2, ti - 1:ti + 2] = 0.0
    for e, w in engines(R, m):
        assert np.array_equal(Want(m).occupied, w.occupied)
        jj, ii = np.nonzero(w.occupied)
        near = (ii - ti) ** 2 + (jj - tj) ** 2 <= Rc * Rc
        off = np.stack([ii[near] - ti, jj[near] - tj], axis=1) * 64                    # what the rotation has to produce
        c, s = EXACT[turn][0] // 16384, EXACT[turn][1] // 16384
        points = np.stack([c * off[:, 0] + s * off[:, 1], -s * off[:, 0] + c * off[:, 1]], axis=1).astype(np.int32)      # turned back
        n_rot, slot = 7, 5                                                             # r_c = 3: the true rotation sits two slots off
        base = np.arctan2(EXACT[turn][1], EXACT[turn][0])
        ang = base + (np.arange(n_rot) - slot) * STEP      # (a slot moves a point 20 cells out by more than a cell: no neighbour ties)
        rot = np.stack([np.rint(16384 * np.cos(ang)), np.rint(16384 * np.sin(ang))], axis=1).astype(np.int32)
        assert tuple(rot[slot]) == EXACT[turn]
        gi, gj = ti - plant[0], tj - plant[1]                                           # the guess cell: the shift leads back to the true one
        assert abs(plant[0]) <= T and abs(plant[1]) <= T
        q = np.zeros(1, R.capi.SCAN_MATCH_QUERY_DTYPE)
        q[0] = (w.buffer_cell(gi, gj), (0, 0), 0, len(points))
        _, got, _ = check(e, R, q, points, rot[None], Rc, T, L, w)
        status, score, r, da, db, n_used, _, score_max = got[0]
        assert (status, r, da, db) == (0, slot, plant[0], plant[1]) and n_used == len(points) > 20 and score == score_max == n_used * L
        g = e.geometry()
        x, y = engine_centre(e, int(q[0]["cell"]))
        fixed = R.capi.scan_match_pose(g, x, y, 0.5, STEP, n_rot, e.scan_match(q, points, rot[None], Rc, T, L)[0])
        tx, ty = engine_centre(e, w.buffer_cell(ti, tj))
        assert abs(fixed[0] - tx) < 1e-9 and abs(fixed[1] - ty) < 1e-9 and abs(fixed[2] - (0.5 + 2 * STEP)) < 1e-12
        e.close()


# ---- 3. ties ----
def test_ties(R):
    rows, cols = ROWS, COLS
    rng = np.random.default_rng(5)
    # an all-free map: every score is 0, the best is the guess itself
    e = make_engine(R, rows, cols, np.zeros(rows * cols, np.float32))
    w = Want.of(e, R)
    for n_rot in (1, 2, 41):
        queries, points, rot = batch(w, rng, [50, 700], 40, n_rot, [(10, 10), (80, 60)])
        _, got, vol = check(e, R, queries, points, rot, 40, 16, 4, w)
        assert not vol.any() and all(g[:5] == (0, 0, n_rot // 2, 0, 0) and g[5] > 0 and g[6] == 0 for g in got)
    # one long straight wall along j (every cell of map row i = 60): every shift along it ties
    m = np.zeros((cols, rows), np.float32)
    m[:, 60] = 180.0
    e.upload(R.capi.LAYER_MASTER, m.reshape(-1))
    w = Want.of(e, R)
    points = np.array([[64 * 3, 64 * k] for k in range(-6, 7)], np.int32)              # a piece of wall three cells ahead in i
    q = np.zeros(1, R.capi.SCAN_MATCH_QUERY_DTYPE)
    q[0] = (w.buffer_cell(55, 40), (0, 0), 0, len(points))                             # the wall is five cells ahead: da = +2
    rot = np.array([[EXACT[0]] * 3], np.int32)                                         # three identical rotation entries
    _, got, vol = check(e, R, q, points, rot, 40, 8, 2, w)
    assert got[0] == (0, 26, 1, 2, 0, 13, 0, 26)                                       # smallest da^2 + db^2, then r_c itself
    assert (vol[0, :, :, 8 + 2] == 26).all() and (vol[0, :, :, 8 + 1] == 13).all() and (vol[0, :, :, 8 + 3] == 13).all()
    # an even rotation count, both entries equal: r_c = 1 of 2 wins over r = 0
    _, got, _ = check(e, R, q, points, rot[:, :2], 40, 8, 2, w)
    assert got[0][2] == 1
    # two identical entries on either side of r_c, a worse one at r_c: the smaller r wins after |r - r_c|
    tilted = (int(np.rint(16384 * np.cos(0.3))), int(np.rint(16384 * np.sin(0.3))))
    rot3 = np.array([[EXACT[0], tilted, EXACT[0]]], np.int32)
    _, got, vol = check(e, R, q, points, rot3, 40, 8, 2, w)
    assert got[0][:5] == (0, 26, 0, 2, 0) and np.array_equal(vol[0, 0], vol[0, 2]) and vol[0, 1].max() < 26
    # two walls, seven cells either side of the guess, points three cells ahead and three behind: (da, db) = (-4, 0) and
    # (+4, 0) tie in score and in distance, and in r and db: the smaller da wins
    m[:, 46] = 180.0
    e.upload(R.capi.LAYER_MASTER, m.reshape(-1))
    w = Want.of(e, R)
    q[0] = (w.buffer_cell(53, 40), (0, 0), 0, len(points))
    both = np.concatenate([points, points * np.array([-1, 1], np.int32)])
    q[0]["n_points"] = len(both)
    _, got, vol = check(e, R, q, both, rot, 40, 8, 2, w)
    assert vol[0, 1, 8, 8 - 4] == vol[0, 1, 8, 8 + 4] == vol[0, 1].max() and got[0][:5] == (0, int(vol[0, 1].max()), 1, -4, 0)
    e.close()


# ---- 4. statuses mixed into a batch; pairs that are no rotation; the records' bounds ----
def test_statuses_in_a_batch(R):
    m = rooms_map(seed=21)
    for e, w in engines(R, m):
        rng = np.random.default_rng(9)
        queries, points, rot = batch(w, rng, [200, 200, 0, 200, 200, 30, 200], 40, 5, [(20, 20), (70, 50), (5, 75)])
        queries["cell"][1] = -1                                                        # status 1
        queries["cell"][4] = ROWS * COLS
        far = np.array([[64 * 40 + 1, 0], [0, -64 * 40 - 1], [32768, 0], [-1 << 30, 5], [2000, 2000]], np.int32)      # none within R = 40
        lo = int(queries["points_offset"][5])
        points[lo:lo + 30] = far[np.arange(30) % 5]                                    # status 2: points, none used
        rot[6, 1] = (16384, 16384)                                                     # no rotation: stretches points out of the window
        rot[6, 3] = (-16384, 16384)
        _, got, vol = check(e, R, queries, points, rot, 40, 3, 3, w)
        assert [g[0] for g in got] == [0, 1, 2, 0, 1, 2, 0]
        for k in (1, 2, 4, 5):
            assert got[k] == (got[k][0], 0, 2, 0, 0, 0, 0, 0) and not vol[k].any()
        assert got[0][5] > 0 and got[6][5] > 0
        # sub beyond its range is no contract, but it is not a fault either: such points fall out of the window
        queries["sub"][0] = (5000, -5000)
        check(e, R, queries, points, rot, 40, 3, 3, w)
        e.close()


# ---- 5. the two forms; the _device form behind a map update ----
def test_host_and_device_forms(R):
    hip = Hip()
    m = rooms_map(seed=31)
    m[30:50, 30:60] = 0.0
    e = make_engine(R, ROWS, COLS, m.reshape(-1))
    e.upload(R.capi.LAYER_LASER, m.reshape(-1))
    e.compose_master(1)
    w = Want.of(e, R)
    rng = np.random.default_rng(13)
    Rc, T, L, n_rot = 40, 4, 3, 5
    queries, points, rot = batch(w, rng, [300, 0, 2500, 77], Rc, n_rot, [(45, 40), (40, 35), (50, 45)])
    queries["cell"][3] = -7
    queries = np.ascontiguousarray(queries.astype(R.capi.SCAN_MATCH_QUERY_DTYPE))
    _, before, vol_before = check(e, R, queries, points, rot, Rc, T, L, w)
    S = 2 * T + 1
    d_q, d_p, d_r = hip.upload(queries), hip.upload(points), hip.upload(rot)
    d_out, d_vol = hip.alloc(32 * len(queries)), hip.alloc(4 * len(queries) * n_rot * S * S)
    for with_volume in (True, False):
        e.scan_match_device(d_q, len(queries), d_p, len(points), d_r, n_rot, Rc, T, L, d_out, d_vol if with_volume else None)
        e.synchronize()
        dev = hip.download(d_out, R.capi.SCAN_MATCH_DTYPE, len(queries))
        host, host_vol = e.scan_match(queries, points, rot, Rc, T, L, volume=True)
        assert dev.tobytes() == host.tobytes() and as_tuples(dev) == before
        assert hip.download(d_vol, np.int32, host_vol.size).tobytes() == host_vol.tobytes()
    # a query whose points leave the array: status 2 in the _device form (the host form refuses it)
    bad = queries.copy()
    bad["n_points"][0] = len(points) + 1
    bad["points_offset"][2] = -1
    with pytest.raises(R.capi.RnaError, match="RNA_EINVAL"):
        e.scan_match(bad, points, rot, Rc, T, L)
    d_bad = hip.upload(bad)
    e.scan_match_device(d_bad, len(bad), d_p, len(points), d_r, n_rot, Rc, T, L, d_out, d_vol)
    e.synchronize()
    dev = as_tuples(hip.download(d_out, R.capi.SCAN_MATCH_DTYPE, len(bad)))
    assert [g[0] for g in dev] == [2, 2, 2, 1] and all(g[1:] == (0, n_rot // 2, 0, 0, 0, 0, 0) for g in dev)
    assert not hip.download(d_vol, np.int32, len(bad) * n_rot * S * S).any()
    # ordered behind a map update enqueued before it, with no synchronisation in between: rays that end in the free room leave
    # occupied cells where the first query's points fall
    gi, gj = w.map_cell(int(queries["cell"][0]))
    rays = np.zeros(40, R.capi.RAY_DTYPE)
    for k in range(40):
        rays["sx"][k], rays["sy"][k] = engine_centre(e, w.buffer_cell(gi, gj))
        rays["ex"][k], rays["ey"][k] = engine_centre(e, w.buffer_cell(gi - 6 + k % 5, gj + 4 + k % 2))
    d_rays = hip.upload(rays)
    e.update_map_device(d_rays, len(rays), 0)
    e.scan_match_device(d_q, len(queries), d_p, len(points), d_r, n_rot, Rc, T, L, d_out, d_vol)
    e.synchronize()
    dev = hip.download(d_out, R.capi.SCAN_MATCH_DTYPE, len(queries))
    dev_vol = hip.download(d_vol, np.int32, vol_before.size).reshape(vol_before.shape)
    w2, after, vol_after = check(e, R, queries, points, rot, Rc, T, L)
    assert w2.occupied.sum() > w.occupied.sum()
    assert as_tuples(dev) == after and np.array_equal(dev_vol, vol_after) and not np.array_equal(vol_after, vol_before)
    for p in (d_q, d_p, d_r, d_out, d_vol, d_bad, d_rays):
        hip.free(p)
    e.close()


# ---- 6. the capacity rule, n == 0 ----
def test_capacity_and_empty_batches(R):
    e = make_engine(R, ROWS, COLS, np.zeros(ROWS * COLS, np.float32))
    q = np.zeros(1, R.capi.SCAN_MATCH_QUERY_DTYPE)
    q[0] = (5, (0, 0), 0, 1)
    points = np.array([[64, 64]], np.int32)
    out = np.zeros(1, R.capi.SCAN_MATCH_DTYPE)
    P = lambda a: a.ctypes.data      # noqa: E731
    for Rc, T, L, n_rot in ((128, 16, 4, 128), (127, 17, 4, 128), (127, 16, 5, 128), (127, 16, 4, 129)):
        rot = np.tile(np.array(EXACT[0], np.int32), (1, n_rot, 1))
        assert e._L.rna_scan_match(e.h, P(q), 1, P(points), 1, P(rot), n_rot, Rc, T, L, P(out), None) == RNA_ECAPACITY
        assert not out.view(np.uint8).any()
        with pytest.raises(R.capi.RnaError, match="RNA_ECAPACITY.*RNA_SCAN_MATCH_MAX"):
            e.scan_match(q, points, rot, Rc, T, L)
    rot = np.tile(np.array(EXACT[0], np.int32), (1, 128, 1))
    # one workgroup per (query, rotation) and one launch: 2^24 of them are refused before any buffer is read
    for fn in (e._L.rna_scan_match, e._L.rna_scan_match_device):
        assert fn(e.h, P(q), (1 << 24) // 128, P(points), 1, P(rot), 128, 10, 2, 2, P(out), None) == RNA_ECAPACITY
        assert b"2^24" in e._L.rna_last_error(e.h) and not out.view(np.uint8).any()
    recs = e.scan_match(q, points, rot, 127, 16, 4)                                    # the caps themselves are served
    assert as_tuples(recs) == [(0, 0, 64, 0, 0, 1, 0, 4)]
    assert len(e.scan_match(np.zeros(0, R.capi.SCAN_MATCH_QUERY_DTYPE), np.zeros((0, 2), np.int32), np.zeros((0, 3, 2), np.int32), 10, 2, 2)) == 0
    assert e._L.rna_scan_match(e.h, None, 0, None, 0, None, 3, 10, 2, 2, None, None) == 0
    assert e._L.rna_scan_match_device(e.h, None, 0, None, 0, None, 3, 10, 2, 2, None, None) == 0
    e.close()


# ---- 7. from laser scans to corrected poses ----
def test_scan_match_poses(R):
    """a square room, scans taken from a true pose, guesses off by a few cells and a few rotation steps: the corrected pose is
    back within a cell and a step of the true one, and the records are what scan_match gives for the prepared queries"""
    rows = cols = 120
    m = np.zeros((cols, rows), np.float32)
    m[20, 20:100] = m[99, 20:100] = 180.0
    m[20:100, 20] = m[20:100, 99] = 180.0
    m[60, 20:50] = 180.0                                                               # (breaks the square's symmetry)
    e = make_engine(R, rows, cols, m.reshape(-1))
    w = Want.of(e, R)
    truth = np.array([[0.3, -0.4, 0.2], [-0.6, 0.5, -1.1]])
    n_beams = 360
    scans = np.zeros(len(truth), R.capi.SCAN_DTYPE)
    ranges = np.zeros(len(truth) * n_beams, np.float32)
    jj, ii = np.nonzero(w.occupied)
    centres = np.array([engine_centre(e, w.buffer_cell(int(i), int(j))) for i, j in zip(ii, jj)])
    for k, (x, y, yaw) in enumerate(truth):
        inc = 2 * np.pi / n_beams
        scans[k] = (-np.pi, np.pi, inc, 0.1, 4.0, n_beams, k * n_beams, x, y, yaw, x, y, yaw)
        for b in range(n_beams):                                                       # the nearest wall cell centre within half a beam
            a = yaw - np.pi + b * np.float32(inc)
            d = centres - (x, y)
            along, across = d @ (np.cos(a), np.sin(a)), d @ (-np.sin(a), np.cos(a))
            hit = (along > 0) & (np.abs(across) < 0.5 * RES)
            ranges[k * n_beams + b] = along[hit].min() if hit.any() else np.inf
    yaw_step, n_rot, T, L = 0.01, 21, 8, 3
    guesses = truth + np.array([[3 * RES, -2 * RES, 4 * yaw_step], [-5 * RES, 1 * RES, -6 * yaw_step]])
    recs, fixed = e.scan_match_poses(scans, ranges, guesses, yaw_step, n_rot, T, L)
    assert all(r["status"] == 0 and r["n_used"] > 100 and r["score"] > r["score_guess"] for r in recs)
    assert np.abs(fixed[:, :2] - truth[:, :2]).max() <= RES + 1e-9 and np.abs(fixed[:, 2] - truth[:, 2]).max() <= yaw_step + 1e-9
    for k in range(len(truth)):
        assert tuple(fixed[k]) == R.capi.scan_match_pose(e.geometry(), *guesses[k], yaw_step, n_rot, recs[k])
    # the window's reach is floor(range_max / resolution) cells, refused outside 1..127 as move_control::matchScan refuses it
    for range_max, code in ((6.45, "RNA_ECAPACITY"), (0.04, "RNA_EINVAL")):
        wide = scans.copy()
        wide["range_max"][:] = range_max
        with pytest.raises(R.capi.RnaError, match=code):
            e.scan_match_poses(wide, ranges, guesses, yaw_step, n_rot, T, L)
    wide["range_max"][:] = 6.39                                                        # 127 cells: served
    assert all(r["status"] == 0 for r in e.scan_match_poses(wide, ranges, guesses, yaw_step, n_rot, T, L)[0])
    e.close()


# ---- 8. the fuzzer, briefly, in this process ----
def test_fuzzer_runs(R):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fuzz_scan_match", os.path.join(root, "scripts", "fuzz_scan_match.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    line = fuzz.run(5.0, 3)
    assert line.startswith("fuzz_scan_match ok") and "every record and volume equal" in line, line
