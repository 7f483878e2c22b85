"""GPU: the engine's map state after a HISTORY against the model of tests/_mapmodel.py.  Every answer of the planners comes from
state the engine keeps lazily consistent with the master layer -- the neighbour masks, the footprint bits of a robot radius, the
dirty-tile flags and their double buffer, the epoch behind the stale flags -- and which refresh runs depends on what happened
before the call.  Here random sequences of every map operation (HIMM on each layer, compose in both modes, update, upload,
fill, four kinds of move, radius changes, clones that both go on) run on one engine, and after every operation the engine is
compared with the model: geometry, the three layers bit for bit, the blocked set and the neighbour masks, the dirty-tile report
of a compose, sixteen searches (every third step a pipelined batch that must answer for the map of its launch), and the stale
flags of clearance, goal field and frontiers.  The three are rebuilt after every such check, so that the flags read 0 before the
next operation and its own epoch bump is what the check sees; on the fifth of the steps that read no masks the flags are still
read, and a change the model alone can tell must have set them.  The sequence ends with a rebuild checked by their own modules.

With a radius the blocked set's oracle is ref_blocked of tests/test_gpu_footprint.py (the reference's predicate cell by cell) at
a few checkpoints, and at the other steps a FRESH engine given the model's geometry and map: its full build is pinned to the
predicate by that module, and what is new here is that history does not matter.

A failure prints the step and the sequence so far as a literal: `run_sequence(R, *REPLAY)` replays it."""
import ctypes as C
import collections

import numpy as np
import pytest

import _mapmodel as M
import _oracle as O  # noqa: F401  (the oracle library is built by the session fixture)
import test_gpu_clearance as TC
import test_gpu_footprint as F
import test_gpu_frontiers as TF
import test_gpu_goal_field as TG
from _gpu import TABLE, UNREACHED, Hip, R, blocked_of, map_nbr, same_f32, to_map  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu

NQ, MAX_LEN, DEPTH, CAP = 16, 4096, 4, 7
MASTER, LASER, RANGE = M.MASTER, M.LASER, M.RANGE
RES, TILE = M.RES, M.TILE


class Pair:
    """an engine and its model"""

    def __init__(self, e, m, replaced):
        self.e, self.m = e, m
        self.replaced = replaced      # a layer was replaced since the last compose: the next one is a whole-layer copy
        self.feat = None              # the snapshot of a feature build


def configure(e):
    e.astar_pipeline_depth(DEPTH)
    e.astar_configure(max_queries=NQ)
    return e


def new_engine(R, m):
    e = R.Engine(m.rows * RES, m.cols * RES, RES, *M.POS)
    assert (e.rows, e.cols) == (m.rows, m.cols)
    e.upload(LASER, m.layers[LASER])
    e.compose_master(1)                                   # master = laser, no layer replaced since
    return configure(e)


def clone_engine(R, e):
    """rna_clone, raw: the package has no wrapper for it"""
    h = C.c_void_p()
    assert e._L.rna_clone(e.h, C.byref(h)) == 0
    c = R.Engine.__new__(R.Engine)
    c._L, c.h, c.device = e._L, h, e.device
    c.rows, c.cols, c.ncell, c.resolution, c.hist_size = e.rows, e.cols, e.ncell, e.resolution, None
    return configure(c)


def apply_engine(R, e, m, kind, args):
    """the operation on the engine; m is the model BEFORE it (the rays and a move's target are drawn from its geometry)"""
    ray = lambda spec: M.rays_of(m.g, spec).view(R.capi.RAY_DTYPE)   # noqa: E731
    if kind == "himm":
        e.himm_update(args[0], ray(args[1]))
    elif kind == "compose":
        e.compose_master(args[0])
    elif kind == "update":
        e.update_map(ray(args[0]), compose_mode=args[1])
    elif kind == "upload":
        e.upload(args[0], M.map_of(m.rows, m.cols, args[1], args[2]))
    elif kind == "fill":
        e.fill(args[0], float("nan") if args[1] is None else args[1])
    elif kind == "move":
        e.move(*m.move_target(args))
    elif kind == "radius":
        assert e.astar_robot_radius(args[0]) == args[0]
    else:
        assert kind in ("search", "features"), kind


# ---- 1, 2: geometry and layers ----
def check_geometry_and_layers(p):
    ge, g = p.e.geometry(), p.m.g
    assert (tuple(ge.start_index), tuple(ge.position), tuple(ge.size), tuple(ge.length), ge.resolution) == \
        (tuple(g.start), tuple(g.pos), tuple(g.size), tuple(g.len), g.res), "geometry"
    for layer in (MASTER, LASER, RANGE):
        assert same_f32(p.e.download(layer), p.m.layers[layer]), "layer %d" % layer


# ---- 3: blocked set and neighbour masks ----
def fresh_engine(R, m):
    """A new engine with the model's geometry, START INDEX INCLUDED: created s cells away and moved once to the model's position,
    so that the same buffer order holds the same map.  (The start index is part of what the blocked set of a radius depends on:
    where a disc's box ends on the map's far edge the reference's iterator answers differently on a moved buffer, include/rna.h
    at rna_astar_set_robot_radius; a fresh engine at start index (0, 0) fed the map in map order is another map to it.)  None
    when the one move does not land on the model's position bit for bit."""
    s0, s1 = m.g.start[0], m.g.start[1]

    def origin(pos, s):
        """where to create the engine so that GridMap::move's own arithmetic (shift = -(int)(t +- 0.5), position += -shift * res)
        lands on `pos` with start index s: s cells away, or an ulp or two beside that"""
        first = pos + s * RES
        for c in (first, np.nextafter(first, np.inf), np.nextafter(first, -np.inf), first + 2 * np.spacing(first), first - 2 * np.spacing(first)):
            t = (pos - c) / RES
            shift = -int(t + (0.5 if t > 0 else -0.5))
            if shift == s and c + float(-shift) * RES == pos:
                return float(c)
        return float(first)

    e = R.Engine(m.rows * RES, m.cols * RES, RES, origin(m.g.pos[0], s0), origin(m.g.pos[1], s1))
    if (s0, s1) != (0, 0):
        e.move(m.g.pos[0], m.g.pos[1])
    g = e.geometry()
    if (tuple(g.position), tuple(g.start_index), tuple(g.size)) != (tuple(m.g.pos), (s0, s1), (m.rows, m.cols)):
        e.close()
        return None
    return e


def check_masks(R, p, use_ref, tally):
    """returns the engine's blocked set once it is tied to the model"""
    e, m = p.e, p.m
    got_b, got_n = e.astar_blocked_mask(), e.nbr_mask()
    if m.r == 0.0 or use_ref:
        want = blocked_of(m.master) if m.r == 0.0 else F.ref_blocked(m.g, m.master, m.r)
        bad = np.flatnonzero(got_b != want)
        assert bad.size == 0, ("blocked set, r=%g" % m.r, bad[:10], got_b[bad[:10]], want[bad[:10]])
        bad = np.flatnonzero(got_n != map_nbr(m.g, want))
        assert bad.size == 0, ("neighbour masks, r=%g" % m.r, bad[:10])
        tally["masks against the predicate" if m.r else "masks against blocked_of"] += 1
        return got_b
    fresh = fresh_engine(R, m)
    if fresh is None:                                     # (its position would not come out bit for bit: the predicate instead)
        tally["masks against the predicate because a fresh engine's position did not come out bit for bit (counted in the former)"] += 1
        return check_masks(R, p, True, tally)
    try:
        for layer in (LASER, MASTER):
            fresh.upload(layer, m.layers[layer])
        fresh.astar_robot_radius(m.r)
        fb, fn = fresh.astar_blocked_mask(), fresh.nbr_mask()
    finally:
        fresh.close()
    rows, cols, s0, s1 = m.rows, m.cols, m.g.start[0], m.g.start[1]
    bad = np.argwhere(to_map(got_b != fb, rows, cols, s0, s1))
    assert bad.size == 0, ("blocked set differs from a fresh engine's, r=%g, map cells [j, i]" % m.r, bad[:10])
    bad = np.argwhere(to_map(got_n != fn, rows, cols, s0, s1))
    assert bad.size == 0, ("neighbour masks differ from a fresh engine's, r=%g, map cells [j, i]" % m.r, bad[:10])
    tally["masks against a fresh engine"] += 1
    return got_b


# ---- 4: the dirty-tile report of a compose ----
def check_dirty(p, before, whole):
    e, m = p.e, p.m
    flags = e.last_dirty_tiles()
    after = m.master
    diff = before.view(np.uint32) != after.view(np.uint32)      # bitwise, NaN payloads included (both arrays are the model's)
    jj, ii = np.nonzero(diff.reshape(m.cols, m.rows))
    tiles = np.unique((jj // TILE) * e.tile_grid()[0] + ii // TILE)
    missing = tiles[flags[tiles] == 0]
    assert missing.size == 0, ("tiles whose master changed are not in last_dirty_tiles", missing, flags)
    if whole:
        assert flags.all(), ("a whole-layer copy reports every tile", flags)


# ---- 5: searches ----
class Batch:
    """a pipelined batch in flight and the model as it was at its launch"""

    def __init__(self, R, hip, p, blocked, q):
        self.dtype = R.capi.ASTAR_RESULT_DTYPE
        self.hip, self.e, self.g, self.blocked, self.q, self.moved = hip, p.e, M.copy_geom(p.m.g), blocked.copy(), q, p.m.moved()
        self.d_q, self.d_paths, self.d_res = hip.upload(q), hip.alloc(NQ * MAX_LEN * 4), hip.alloc(NQ * 24)
        p.e.astar_device(self.d_q, NQ, self.d_paths, MAX_LEN, self.d_res)

    def finish(self):
        self.e.synchronize()
        res = self.hip.download(self.d_res, self.dtype, NQ)
        paths = self.hip.download(self.d_paths, np.int32, NQ * MAX_LEN).reshape(NQ, MAX_LEN)
        self.free()
        return F.check_search(self.e, self.g, self.blocked, self.q, res, paths, None, self.moved)

    def free(self):
        for d in (self.d_q, self.d_paths, self.d_res):
            if d:
                self.hip.free(d)
        self.d_q = self.d_paths = self.d_res = None


def search(p, blocked, q):
    res, paths = p.e.astar(q, MAX_LEN)
    return F.check_search(p.e, p.m.g, blocked, q, res, paths, None, p.m.moved())


# ---- 6: the snapshots and their stale flags ----
def stale_flags(e):
    """(clearance, goal field, frontiers): getters that read no derived state"""
    return (int(e.clearance_info()[1]), e.goal_field_info()["stale"], e.frontiers_info()["stale"])


def build_features(R, p, blocked, args):
    """builds clearance, goal field and ranked frontiers and keeps what the snapshot must go on answering; all three flags
    read 0 afterwards, so the NEXT operation is the one its stale check is about"""
    e, m = p.e, p.m
    seed, table = args
    rng = np.random.default_rng(seed)
    free = np.flatnonzero(blocked == 0)
    if free.size == 0:
        p.feat = None
        return
    e.goal_field_clearance_cost(TABLE if table else [])
    e.clearance(CAP)
    goal = int(rng.choice(free))
    info = e.goal_field(goal)
    assert (info["goal"], info["status"], info["stale"]) == (goal, 0, 0)
    field, nx = e.goal_field_download(want_next=True)
    e.frontiers(rank=True)
    assert e.clearance_info() == (CAP, False) and stale_flags(e) == (0, 0, 0)
    reached = np.flatnonzero((field != UNREACHED) & (field != TG.FAR))
    starts = rng.choice(reached, 8).astype(np.int32)
    start_index = (m.g.start[0], m.g.start[1])
    want = [TG.walk_next(nx, m.rows, m.cols, int(s), start_index) for s in starts]
    paths, res = e.goal_field_paths(starts, MAX_LEN)
    p.feat = dict(args=(seed + 1, table), key=m.state_key(blocked), point=m.point_blocked(), starts=starts, want=want, cost=field[starts], paths=paths, res=res)
    check_snapshot_paths(p)


def check_snapshot_paths(p):
    f = p.feat
    paths, res = p.e.goal_field_paths(f["starts"], MAX_LEN)
    for k, w in enumerate(f["want"]):
        assert (res["status"][k], res["path_len"][k], res["cost"][k]) == (0, len(w), f["cost"][k]), ("a path of the snapshot", k)
        assert np.array_equal(paths[k][:len(w)], w), ("a path of the snapshot", k)


def must_refuse(R, what, call):
    try:
        call()
    except R.capi.RnaError:
        return
    raise AssertionError(what + " did not raise RnaError")


def check_stale(R, p, blocked, was, tally):
    """after an operation on an engine with snapshots.  `was`: the flags before the operation.  blocked: the engine's blocked
    set tied to the model (a checked step), or None (a step that reads no masks): then a change is known only from what the
    model alone says -- the unknown set, the geometry, the radius, and with r = 0 the blocked set."""
    e, f, m = p.e, p.feat, p.m
    if blocked is not None:
        changed = m.state_key(blocked) != f["key"]
    else:
        changed = m.state_key(f["point"])[1:] != f["key"][1:] or (m.r == 0.0 and not np.array_equal(m.point_blocked(), f["point"]))
    stale = stale_flags(e)
    if changed:
        assert stale == (1, 1, 1), ("stale flags (clearance, goal field, frontiers) after a change; before it they read", stale, was)
        tally["stale checks after a change, flags 0 0 0 before it" if was == (0, 0, 0) else "stale checks after a change, flags set before it"] += 1
    elif blocked is not None:
        tally["stale checks after no change (flags %d %d %d)" % stale] += 1
    if stale[0]:
        must_refuse(R, "shortcut_paths(keep_clearance=True) on a stale clearance field",
                    lambda: e.shortcut_paths(f["paths"], f["res"], keep_clearance=True))
    if stale[1]:
        must_refuse(R, "frontiers(rank=True) on a stale goal field", lambda: e.frontiers(rank=True))
        check_snapshot_paths(p)


# ---- 7: the rebuild at the end ----
def rebuild(R, p, blocked, table, tally):
    e = p.e
    e.goal_field_clearance_cost(table)
    TC.check_clearance(e, CAP)
    free = np.flatnonzero(blocked == 0)
    if free.size:
        want = TC.check_field(e, int(free[free.size // 2]), table)
        tally["cells the rebuilt fields reach"] += int((want[0] != UNREACHED).sum())
        w, _ = TF.check(e, R, rank=True)
        tally["frontier cells at the rebuild"] += w.cells
        assert e.goal_field_info()["stale"] == 0
    else:
        TF.check(e, R)
    assert e.clearance_info() == (CAP, False) and e.frontiers_info()["stale"] == 0


def run_sequence(R, shape, seed, ops, masks_only=False, tally=None):
    """runs `ops` (tests/_mapmodel.py) on a new engine of `shape` whose first map is map_of(seed) and checks every step"""
    rows, cols = shape
    tally = collections.Counter() if tally is None else tally
    hip = Hip()
    F._discs.clear()                                      # the disc lists of ref_blocked, per geometry: not kept across sequences
    m0 = M.MapModel(rows, cols, seed)
    pairs = [Pair(new_engine(R, m0), m0, False)]
    batch = None
    ref_left = 1                                          # ref_blocked checkpoints before the end (two more there at the most)
    due = 0                                               # pipelined batches owed: one every third step
    step = -1
    try:
        for step, (who, kind, args, checked) in enumerate(ops):
            p = pairs[who]
            looked = [p]
            before = p.m.master.copy()
            due += step % 3 == 2
            was = stale_flags(p.e) if p.feat is not None else None
            if kind == "clone":
                pairs.append(Pair(clone_engine(R, p.e), p.m.clone(), True))
                looked.append(pairs[-1])
            else:
                apply_engine(R, p.e, p.m, kind, args)
                p.m.apply(kind, args)
            tally["op " + kind] += 1
            if batch is not None:                         # launched before this operation: it answers for the map of its launch
                found = batch.finish()
                batch = None
                tally["pipelined batches"] += 1
                tally["searches with a path"] += found
            for t in looked:
                check_geometry_and_layers(t)
            if kind in ("compose", "update"):
                check_dirty(p, before, args[-1] == 1 or p.replaced)
                p.replaced = False
                tally["compose " + M.expected_path(M.lineage(ops[:step + 1], who), shape)[-1]] += 1
            elif (kind in ("upload", "fill") and args[0] in (MASTER, LASER)) or (kind == "himm" and args[0] == MASTER):
                p.replaced = True
            if not checked:
                if p.feat is not None and not masks_only:
                    check_stale(R, p, None, was, tally)   # (getters only: the masks stay as they are)
                continue
            for t in looked:
                use_ref = t.m.r > 0.0 and ref_left > 0
                ref_left -= use_ref
                blocked = check_masks(R, t, use_ref, tally)   # (of a clone step: the clone's, equal to the original's)
            if masks_only:
                continue
            if kind == "features":
                assert who == 0
                build_features(R, p, blocked, args)
            q = M.queries_of(seed, step, who, blocked)
            # a pipelined batch is launched as the LAST thing of its step, before an operation on the same engine
            pipelined = q is not None and due > 0 and step + 1 < len(ops) and ops[step + 1][0] == who
            if q is not None:
                tally["searches"] += NQ
                if not pipelined:
                    tally["searches with a path"] += search(p, blocked, q)
            if p.feat is not None and kind != "features":
                check_stale(R, p, blocked, was, tally)
                build_features(R, p, blocked, p.feat["args"])     # the flags read 0 again before the next operation
            if pipelined:
                batch = Batch(R, hip, p, blocked, q)
                due -= 1
        step = len(ops)
        last = pairs[ops[-1][0]] if ops else pairs[0]
        for who, p in enumerate(pairs):
            blocked = check_masks(R, p, p.m.r > 0.0 and (p is last or p is pairs[0]), tally)
            if not masks_only:
                rebuild(R, p, blocked, TABLE if who % 2 == 0 else [], tally)
        tally["sequences"] += 1
    except (AssertionError, R.capi.RnaError) as err:
        raise AssertionError("%s: %s\nat step %d (%s) of this sequence; `step` counts from 0 and the literal ends with it:\n%s"
                             % (type(err).__name__, err, step, "the end" if step >= len(ops) else ops[step][1],
                                M.replay_literal(shape, seed, ops[:step + 1]))) from err
    finally:
        for p in pairs:
            p.e.close()                                   # (waits for a batch in flight)
        if batch is not None:
            batch.free()
    return tally


CASES = [(shape, seed) for shape in M.SHAPES for seed in M.SEEDS[shape]]


@pytest.mark.parametrize("shape,seed", CASES, ids=["%dx%d-seed%d" % (s[0], s[1], k) for s, k in CASES])
def test_random_sequence_matches_the_model(R, shape, seed):
    tally = run_sequence(R, shape, seed, M.generate(shape, seed))
    print("\n%dx%d seed %d:" % (shape[0], shape[1], seed), dict(sorted(tally.items())))
    assert tally["sequences"] == 1 and tally["searches"] >= 8 * NQ


@pytest.mark.parametrize("name", sorted(M.HAND_WRITTEN))
def test_hand_written_sequence_matches_the_model(R, name):
    shape, seed, ops = M.HAND_WRITTEN[name]
    tally = run_sequence(R, shape, seed, ops)
    print("\n(%s):" % name, dict(sorted(tally.items())))
    want = {"a": {"compose footprint": 3, "compose fused": 2}, "b": {"compose moved": 1, "compose fused": 2},
            "c": {"compose whole": 2, "compose fused": 1}, "d": {"compose moved": 1, "op clone": 1},
            "e": {"stale checks after a change, flags 0 0 0 before it": 8}}[name]
    for k, n in want.items():          # (accounting: the sequence still walks the way it was written for)
        assert tally[k] >= n, (k, dict(tally))
    if name == "e":                    # the move to the current position and the fill of the laser: the flags may read either way
        assert sum(n for k, n in tally.items() if k.startswith("stale checks after no change")) == 2, dict(tally)
