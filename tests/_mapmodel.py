"""A model of the engine's map state in plain Python over the oracles, the generator of random operation sequences and the
printer of the literal that replays one (test infrastructure; no GPU is needed to import or run any of it).

The model holds the oracle's geometry, the three layers as float32 arrays in buffer order and the robot radius, and its
operations are the documented semantics and nothing else: HIMM is og_himm_update, a compose is `master = laser` in either mode
(map_provider.cpp:221), an upload or a fill is an assignment, a move is og_move over the three layers at once, a clone is a
deep copy.  It mirrors none of the engine's flags.  expected_path() is the one exception and is used for accounting only: it
names the way through rna_compose_master that the documented rules select after a history, so that the tests can count
which ways the fixed seeds reach; no expected value is ever derived from it.

An operation is a tuple (who, kind, args, checked):
  who      which engine of the sequence it goes to: 0 is the first one, a "clone" appends the next
  kind     "himm" (layer, rays)   "compose" (mode,)   "update" (rays, mode)   "upload" (layer, seed, occupied)
           "fill" (layer, value or None for NaN)   "move" (cells in i, cells in j)   "radius" (metres,)   "clone" ()
           "search" ()  no change: a step that only looks     "features" (seed, table)  no change: build clearance, field, frontiers
  checked  True: masks, searches and stale flags are compared after it.  False: only geometry and layers are, which read no
           derived state, so that the masks stay pending across the next operation.
`rays` is (seed, n, box): n rays drawn from the seed, over the whole map (box None) or inside box = ((x0, x1), (y0, y1)),
metres from the map's centre at the time of the call.  Every argument is a number, so a sequence prints as a literal."""
import pprint

import numpy as np

import _oracle as O
import test_gpu_footprint as F      # sample_map, rays: the maps and whole-map ray batches of the robot radius' tests
import test_gpu_parity as P         # box_rays
from _gpu import blocked_of, to_buffer, to_map

MASTER, LASER, RANGE = 0, 1, 2
RES, POS, TILE = 0.05, (0.4, -0.3), 64
SHAPES = ((140, 96), (200, 150))                      # 3 x 2 tiles (last column 12 wide, second row 32 tall); 4 x 3 tiles, ragged
RADII = (0.0, 0.15, 0.25, 0.3, 0.125)
HIT = 0.15                                            # the marking share of the rays
N_OPS = 14
MOVE_KINDS = ("few", "tile", "far", "home")
PATHS = ("fused", "tiles", "footprint", "whole", "moved")     # the five ways through a compose, and "pending" (see expected_path)
# the fixed sequences of the suite: per shape, eight seeds (tests/test_map_model_host.py checks what they reach)
SEEDS = {(140, 96): (16, 50, 54, 62, 98, 99, 118, 130), (200, 150): (35, 37, 58, 97, 99, 100, 115, 162)}


def copy_geom(g):
    return type(g).from_buffer_copy(g)


def geom_tuple(g):
    return (tuple(g.pos), tuple(g.size), tuple(g.start))


def map_of(rows, cols, seed, occupied=0.002):
    return F.sample_map(rows, cols, seed, occupied=occupied, edge=False)


def rays_of(g, spec):
    seed, n, box = spec
    rng = np.random.default_rng(seed)
    cx, cy = g.pos[0], g.pos[1]
    if box is None:
        return F.rays(rng, n, 0.4 * max(g.len[0], g.len[1]), cx, cy, hit=HIT)
    (x0, x1), (y0, y1) = box
    return P.box_rays(rng, n, (cx + x0, cx + x1), (cy + y0, cy + y1), hit=HIT)


class MapModel:
    def __init__(self, rows, cols, seed):
        self.rows, self.cols = rows, cols
        self.g = O.make_geom(rows * RES, cols * RES, RES, *POS)
        assert (self.g.size[0], self.g.size[1]) == (rows, cols)
        m = map_of(rows, cols, seed)
        self.layers = [m.copy(), m.copy(), np.full(rows * cols, np.nan, np.float32)]
        self.r = 0.0

    def clone(self):
        c = MapModel.__new__(MapModel)
        c.rows, c.cols, c.g, c.r = self.rows, self.cols, copy_geom(self.g), self.r
        c.layers = [a.copy() for a in self.layers]
        return c

    @property
    def master(self):
        return self.layers[MASTER]

    def apply(self, kind, args):
        if kind == "himm":
            O.himm_update(self.g, self.layers[args[0]], rays_of(self.g, args[1]))
        elif kind == "compose":
            self.layers[MASTER] = self.layers[LASER].copy()
        elif kind == "update":
            O.himm_update(self.g, self.layers[LASER], rays_of(self.g, args[0]))
            self.layers[MASTER] = self.layers[LASER].copy()
        elif kind == "upload":
            self.layers[args[0]] = map_of(self.rows, self.cols, args[1], args[2])
        elif kind == "fill":
            self.layers[args[0]] = np.full(self.rows * self.cols, np.nan if args[1] is None else args[1], np.float32)
        elif kind == "move":
            O.move(self.g, self.layers, self.move_target(args))
        elif kind == "radius":
            self.r = float(args[0])
        else:
            assert kind in ("clone", "search", "features"), kind

    def move_target(self, cells):
        return (self.g.pos[0] + cells[0] * RES, self.g.pos[1] + cells[1] * RES)

    def moved(self):
        return (self.g.start[0], self.g.start[1]) != (0, 0)

    def point_blocked(self):
        return blocked_of(self.master)

    def stencil_blocked(self):
        """The blocked set of the radius by the fixed stencil di^2 + dj^2 <= (r / res)^2, in buffer order.  FOR COUNTING ONLY
        (how many queries have a path, whether an operation changed the set): the reference decides ties cell by cell
        (tests/test_gpu_footprint.py), and every expected value of the GPU tests comes from that predicate, never from here."""
        b = self.point_blocked()
        if self.r == 0.0:
            return b
        rows, cols, s0, s1 = self.rows, self.cols, self.g.start[0], self.g.start[1]
        m = to_map(b, rows, cols, s0, s1) != 0
        k = self.r / RES
        n = int(k)
        out = np.zeros_like(m)
        pad = np.zeros((cols + 2 * n, rows + 2 * n), bool)
        pad[n:n + cols, n:n + rows] = m
        for dj in range(-n, n + 1):
            for di in range(-n, n + 1):
                if di * di + dj * dj <= k * k + 1e-9:
                    out |= pad[n + dj:n + dj + cols, n + di:n + di + rows]
        return to_buffer(out.astype(np.uint8), rows, cols, s0, s1)

    def state_key(self, blocked):
        """what the stale flags answer for: the blocked set and the unknown set in map space, the geometry and the radius"""
        rows, cols, s0, s1 = self.rows, self.cols, self.g.start[0], self.g.start[1]
        return (to_map(blocked, rows, cols, s0, s1).tobytes(), to_map(np.isnan(self.master), rows, cols, s0, s1).tobytes(),
                geom_tuple(self.g), self.r)


# ---- accounting: which way through rna_compose_master the documented rules select ----
def lineage(ops, who):
    """the operations that made engine `who` what it is: its own, and before its "clone" those of the engine it was cloned from"""
    parents, n = {0: None}, 1
    for k, op in enumerate(ops):
        if op[1] == "clone":
            parents[n] = (op[0], k)
            n += 1
    out, upto = [], len(ops)
    while who is not None:
        out = [op for op in ops[:upto] if op[0] == who] + out
        if parents[who] is None:
            break
        who, upto = parents[who][0], parents[who][1]
        out = [(who, "cloned", (), False)] + out
    return out


def expected_path(history, shape):
    """history: the operations of one engine from its creation on (lineage()), the engine created as the tests create it (laser
    uploaded, compose mode 1: no layer replaced since, masks not built).  Returns one name per compose in it:
      "fused"      1. dirty tiles only, masks valid, point robot, buffer not moved: the one launch with the flag arrays swapped
      "tiles"      2. the copy, then the neighbour refresh of the dirty tiles plus ring (mode 1 while the masks are valid, r = 0)
      "footprint"  3. the copy, then footprint_refresh(e, 0) (masks valid, r > 0, either mode)
      "whole"      4. whole-layer copy because a layer was replaced (upload, fill, clone, HIMM on the master); masks rebuilt later
      "moved"      5. any of these on a moved buffer: only marks the masks
      "pending"    the copy alone: the masks were waiting for a rebuild already (after a radius, a move, a fresh engine)
    The rules (include/rna.h, csrc/engine.hpp): a mask consumer -- a checked step, a search, a feature build -- leaves the masks
    valid; a radius call, a move by at least a cell and a write to the master leave them waiting; a write to the laser or the
    master other than by HIMM on the laser makes the next compose a whole-layer copy."""
    valid, replaced, r, start = False, False, 0.0, [0, 0]
    out = []
    for who, kind, args, checked in history:
        if kind == "cloned":
            valid, replaced = False, True
            continue
        if kind in ("compose", "update"):
            mode = args[-1]
            moved = start != [0, 0]
            if moved:
                name, valid = "moved", False
            elif replaced:
                name, valid = "whole", False
            elif not valid:
                name = "pending"
            elif r > 0.0:
                name = "footprint"
            else:
                name = "tiles" if mode == 1 else "fused"
            replaced = False
            out.append(name)
        elif kind == "himm":
            if args[0] == MASTER:
                valid, replaced = False, True
        elif kind in ("upload", "fill"):
            if args[0] == MASTER:
                valid, replaced = False, True
            elif args[0] == LASER:
                replaced = True
        elif kind == "move":
            shift = [-int(round(args[0])), -int(round(args[1]))]
            if shift != [0, 0]:
                valid = False
                start = [(start[a] + shift[a]) % shape[a] for a in (0, 1)]
        elif kind == "radius":
            r, valid = float(args[0]), False
        if checked or kind in ("search", "features"):
            valid = True
    return out


def incremental(name):
    return name in ("fused", "tiles", "footprint")


# ---- the generator ----
def _box(rng, g, kind):
    """a box of the map, metres from its centre, a quarter of a cell inside the cells it names (map cell i has
    x = centre + length / 2 - (i + 1/2) res): one 64 x 64 tile, or one that reaches into the partial tile column or row"""
    rows, cols = g.size[0], g.size[1]
    ti, tj = (rows + TILE - 1) // TILE, (cols + TILE - 1) // TILE
    if kind == "tile":
        a, b = int(rng.integers(0, ti)), int(rng.integers(0, tj))
        i0, i1, j0, j1 = a * TILE, min(rows, (a + 1) * TILE), b * TILE, min(cols, (b + 1) * TILE)
    elif rng.random() < 0.5:          # into the partial column: the last 12 + 30 cells in i, any 50 in j
        j0 = int(rng.integers(0, cols - 50))
        i0, i1, j0, j1 = (ti - 1) * TILE - 30, rows, j0, j0 + 50
    else:
        i0 = int(rng.integers(0, rows - 50))
        i0, i1, j0, j1 = i0, i0 + 50, (tj - 1) * TILE - 30, cols
    q = 0.25 * RES
    return ((round(rows * RES / 2 - i1 * RES + q, 4), round(rows * RES / 2 - i0 * RES - q, 4)),
            (round(cols * RES / 2 - j1 * RES + q, 4), round(cols * RES / 2 - j0 * RES - q, 4)))


def _rays(rng, g):
    kind = ("whole", "tile", "partial")[int(rng.integers(0, 3))]
    return (int(rng.integers(0, 1 << 30)), int(rng.integers(200, 401)), None if kind == "whole" else _box(rng, g, kind))


def _move(rng, m, kind):
    rows, cols = m.rows, m.cols
    sign = lambda: 1 if rng.random() < 0.5 else -1   # noqa: E731
    if kind == "few":
        d = [sign() * int(rng.integers(0, 6)), sign() * int(rng.integers(0, 6))]
        if d == [0, 0]:
            d[0] = 3
    elif kind == "tile":              # more than a 64-cell tile and less than the map, along one axis (the other: a few cells)
        d = [sign() * int(rng.integers(65, min(100, rows - 1))), sign() * int(rng.integers(0, 4))]
        if rng.random() < 0.4:
            d = [d[1], sign() * int(rng.integers(65, min(100, cols - 1)))]
    elif kind == "far":               # more than the map: every cell becomes NaN
        d = [sign() * (rows + int(rng.integers(1, 40))), sign() * int(rng.integers(0, 4))]
    else:                             # home: the start index back to (0, 0), the short way round
        s = (m.g.start[0], m.g.start[1])
        d = [s[0] if s[0] <= rows // 2 else s[0] - rows, s[1] if s[1] <= cols // 2 else s[1] - cols]
    return (d[0], d[1])


NO_CHANGE = ("himm_range", "same_radius", "fill_range", "himm_laser", "zero_move")


def generate(shape, seed, n_ops=N_OPS):
    """n_ops operations and one "features" step for the map of `shape` with the initial map seed `seed`.  The draw depends on
    the models (the way home, the boxes of a moved map), so the generator runs them."""
    rows, cols = shape
    rng = np.random.default_rng([seed, rows, cols])
    models = [MapModel(rows, cols, seed)]
    ops = []
    features_at = int(rng.integers(1, 5))
    after_features = False
    last_incremental = False

    def emit(who, kind, args, checked=None):
        if checked is None:
            checked = bool(rng.random() < 0.8)
        ops.append((who, kind, tuple(args), checked))
        if kind == "clone":
            models.append(models[who].clone())
        else:
            models[who].apply(kind, args)

    def draw(who, what):
        m = models[who]
        if what == "update":
            emit(who, "update", (_rays(rng, m.g), 1 if rng.random() < 0.25 else 0))
        elif what == "himm_laser":
            emit(who, "himm", (LASER, _rays(rng, m.g)))
        elif what == "himm_range":
            emit(who, "himm", (RANGE, _rays(rng, m.g)))
        elif what == "himm_master":
            emit(who, "himm", (MASTER, _rays(rng, m.g)))
        elif what == "compose":
            emit(who, "compose", (1 if rng.random() < 0.3 else 0,))
        elif what == "upload":
            emit(who, "upload", (int(rng.integers(0, 3)), int(rng.integers(0, 1 << 30)), float(rng.choice([0.002, 0.004]))))
        elif what == "fill":
            layer = int(rng.integers(0, 3))
            emit(who, "fill", (layer, [0.0, None, 30.0][int(rng.integers(0, 3))] if layer == RANGE else [0.0, None][int(rng.integers(0, 2))]))
        elif what == "fill_range":
            emit(who, "fill", (RANGE, [0.0, None, 30.0][int(rng.integers(0, 3))]))
        elif what == "move":
            kinds = [k for k in MOVE_KINDS if k != "home" or m.moved()]
            p = np.array([{"few": 0.25, "tile": 0.25, "far": 0.1, "home": 0.9}[k] for k in kinds])
            emit(who, "move", _move(rng, m, kinds[int(rng.choice(len(kinds), p=p / p.sum()))]))
        elif what == "radius":
            emit(who, "radius", (float(rng.choice(RADII)),))
        elif what == "zero_move":                        # rna_move to the current position
            emit(who, "move", (0, 0))
        elif what == "same_radius":
            emit(who, "radius", (m.r,))
        elif what == "clone":
            emit(who, "clone", (), checked=True)

    kinds = ("update", "himm_laser", "himm_range", "himm_master", "compose", "upload", "fill", "move", "radius", "same_radius", "clone")
    weight = np.array((0.38, 0.05, 0.03, 0.04, 0.07, 0.06, 0.03, 0.11, 0.14, 0.03, 0.06))
    count = 0
    while count < n_ops:
        if count == features_at and not after_features:
            emit(0, "features", (int(rng.integers(0, 1 << 30)), bool(rng.random() < 0.5)), checked=True)
            after_features = True
            draw(0, NO_CHANGE[int(rng.integers(0, len(NO_CHANGE)))])     # an operation after which `stale` may stay 1: nothing changed
            ops[-1] = ops[-1][:3] + (True,)
            count += 1
            continue
        who = 0 if len(models) == 1 or rng.random() < 0.6 else int(rng.integers(1, len(models)))
        if last_incremental and rng.random() < 0.3:
            what = "radius"
        else:
            w = weight.copy()
            if len(models) >= 3:
                w[-1] = 0.0
            what = kinds[int(rng.choice(len(kinds), p=w / w.sum()))]
        draw(who, what)
        count += 1
        last = ops[-1]
        last_incremental = last[1] in ("update", "compose") and incremental(expected_path(lineage(ops, last[0]), shape)[-1])
    return ops


# ---- the three sequences written out (140 x 96; they stay when the generator changes) ----
_W = None                                           # rays over the whole map
_T = ((0.3125, 3.4875), (-0.7875, 2.3875))          # tile (0, 0) of the unmoved 140 x 96 map
_C = ((-3.4875, -1.2125), (-1.0, 1.4875))           # a box reaching into the partial tile column (i >= 94)
HAND_WRITTEN = {
    # (a) radius 0.3, two incremental refreshes, radius 0, a search so that the next update is the fused launch, radius 0.25
    "a": ((140, 96), 41, [
        (0, "radius", (0.3,), True),
        (0, "update", ((101, 300, _W), 0), True), (0, "update", ((102, 250, _T), 0), True),
        (0, "radius", (0.0,), False), (0, "search", (), True),
        (0, "update", ((103, 300, _C), 0), True), (0, "update", ((104, 200, _W), 0), True),
        (0, "radius", (0.25,), True), (0, "update", ((105, 300, _W), 0), True)]),
    # (b) move by 70 cells in i, an update on the moved buffer, back to start index (0, 0), a search, two fused updates
    "b": ((140, 96), 42, [
        (0, "update", ((111, 300, _W), 0), True),
        (0, "move", (70, 0), False), (0, "update", ((112, 300, _W), 0), False),
        (0, "move", (-70, 0), False), (0, "search", (), True),
        (0, "update", ((113, 250, _T), 0), True), (0, "update", ((114, 300, _C), 0), True)]),
    # (c) HIMM on the laser and no compose, junk into the master, compose 0, HIMM on RANGE, compose 0, HIMM on the master, update
    "c": ((140, 96), 43, [
        (0, "himm", (LASER, (121, 300, _W)), True), (0, "upload", (MASTER, 9001, 0.004), True), (0, "compose", (0,), True),
        (0, "himm", (RANGE, (122, 300, _W)), True), (0, "compose", (0,), True),
        (0, "himm", (MASTER, (123, 300, _T)), True), (0, "update", ((124, 300, _W), 0), True)]),
    # (e) the stale flags after each kind of change, each from flags that read 0: a move to the current position (no change: the
    # flags may read either way), a move, an upload / a fill / HIMM on the master, a compose, a radius, a fill of the laser
    # (no change), a compose that empties the master, the move back
    "e": ((140, 96), 44, [
        (0, "update", ((131, 300, _W), 0), True), (0, "features", (7, True), True), (0, "move", (0, 0), True),
        (0, "move", (3, -2), True), (0, "upload", (MASTER, 9002, 0.004), True), (0, "fill", (MASTER, 0.0), True),
        (0, "himm", (MASTER, (132, 300, _W)), True), (0, "compose", (0,), True), (0, "radius", (0.25,), True),
        (0, "fill", (LASER, None), True), (0, "compose", (1,), True), (0, "move", (-3, 2), True)]),
    # (d) found by scripts/fuzz_map_sequences.py 100 1 -- in the test, not in the engine: a clone on a buffer moved by (-2, -2) with
    # r = 2 1/2 cells blocks eleven cells of map row 93 (the disc's box ends on the far edge, row 95) that the same map blocks
    # on no unmoved buffer; the reference's predicate says so too, so a fresh engine must share the start index to compare
    "d": ((140, 96), 810854937, [
        (0, "radius", (0.125,), True), (0, "update", ((452296236, 291, None), 1), False),
        (0, "update", ((31263957, 359, ((0.3125, 3.4875), (-0.7875, 2.3875))), 0), True),
        (0, "radius", (0.125,), True), (0, "radius", (0.3,), True), (0, "update", ((368778590, 335, None), 1), True),
        (0, "move", (-2, -2), True), (0, "upload", (0, 834401560, 0.004), True),
        (0, "update", ((691519505, 248, ((0.3125, 3.4875), (-0.7875, 2.3875))), 0), False), (0, "fill", (2, None), True),
        (0, "clone", (), True), (1, "himm", (1, (914657510, 269, ((-2.8875, 0.2875), (-2.3875, -0.8125)))), True),
        (1, "radius", (0.125,), False), (0, "move", (160, 3), False)]),
}


def replay_literal(shape, seed, ops):
    """what a failing sequence prints: paste it into a test as `run_sequence(R, *REPLAY)`"""
    return "REPLAY = (%r, %r, %s)" % (tuple(shape), seed, pprint.pformat(list(ops), width=150))


# ---- what a sequence is worth, from the model alone (tests/test_map_model_host.py) ----
def queries_of(seed, step, who, blocked):
    """the sixteen queries of a step, drawn as queries() of tests/test_gpu_footprint.py draws them (no band); None when no
    cell is free"""
    if not (blocked == 0).any():
        return None
    return F.queries(np.random.default_rng([seed, step, who]), blocked, 17, np.zeros(0))[:16]


def survey(shape, seed, ops):
    """runs the model alone through a sequence and counts what the GPU test will meet.  Blocked sets of a radius come from
    stencil_blocked(): counts, not expected values."""
    rows, cols = shape
    models = [MapModel(rows, cols, seed)]
    s = dict(paths=dict.fromkeys(PATHS + ("pending",), 0), moves=dict.fromkeys(MOVE_KINDS, 0), radius_after_incremental=0, clones=0,
             composes=0, composes_changing=0, zero_moves=0, stale_quiet=0, queries=0, found=0, long=0, stale_changed=0, stale_unchanged=0)
    built, fresh = None, False
    for step, (who, kind, args, checked) in enumerate(ops):
        m = models[who]
        if kind == "clone":
            models.append(m.clone())
            s["clones"] += 1
        if kind in ("compose", "update"):
            before = m.master.copy()
            name = expected_path(lineage(ops[:step + 1], who), shape)[-1]
            s["paths"][name] += 1
        if kind == "move":
            start = (m.g.start[0], m.g.start[1])
            s["zero_moves"] += tuple(args) == (0, 0)
        if kind == "move" and tuple(args) != (0, 0):
            s["moves"]["far" if abs(args[0]) >= rows or abs(args[1]) >= cols else
                       "tile" if max(abs(args[0]), abs(args[1])) > TILE else "few"] += 1
        if kind == "radius" and step > 0 and ops[step - 1][0] == who and ops[step - 1][1] in ("compose", "update") and \
                incremental(expected_path(lineage(ops[:step], who), shape)[-1]):
            s["radius_after_incremental"] += 1
        m.apply(kind, args)
        if kind == "move" and not m.moved() and start != (0, 0):
            s["moves"]["home"] += 1                   # (counted as a few / a tile as well: it is both)
        if kind in ("compose", "update"):
            s["composes"] += 1
            a, b = before.view(np.uint32), m.master.view(np.uint32)
            s["composes_changing"] += bool(((a != b) & ~(np.isnan(before) & np.isnan(m.master))).any())
        if not checked:
            if who == 0 and built is not None:        # the flags are read, nothing is rebuilt: they are set when the next one runs
                fresh = False
                s["stale_quiet"] += 1
            continue
        blocked = m.stencil_blocked()
        q = queries_of(seed, step, who, blocked)
        if q is not None:
            stand_in = blocked.astype(np.float32)
            for k in range(len(q)):
                res, path = O.astar_query_on_map(m.g, stand_in, q["start"][k], q["goal"][k])
                s["queries"] += 1
                s["found"] += res.status == 0
                s["long"] += res.status == 0 and res.path_len > 30
        if who == 0:
            # the GPU test rebuilds the snapshots after every checked step of engine 0, so the flags read 0 before the next
            # operation: an operation counts as a trial of the flags only if it ITSELF changes the state while they read 0
            key = m.state_key(blocked)
            if kind != "features" and built is not None:
                s["stale_changed"] += fresh and key != built
                s["stale_unchanged"] += key == built
            if kind == "features" or built is not None:
                built, fresh = key, True
    return s
