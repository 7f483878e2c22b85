"""Pins the oracle's grid_map_core, HIMM and RRT restatements (oracle/gridmath.c, himm.c, rrt.c) and the product's host
walks (rna_line_cells / rna_circle_cells / rna_submap_cells) to the REFERENCE's own code: grid_map_core's GridMap,
GridMapMath and iterators, MapUpdater::lineOnMap and RrtPlanner::makePlan, compiled into oracle/_ref/libref_gridmap.so
(oracle/Makefile `ref`, oracle/ref_shim/).  Bit for bit on every output.

The inputs come from a fixed seed and are built to sit on edges: non-square maps, resolutions 0.025 / 0.05 / 0.1 / 0.2
and 0.03 (not exact in binary), off-origin positions, buffers moved by negative, fractional and larger-than-the-map
shifts; rays along axes and exact diagonals, ending on cell centres, cell edges and the border, of zero length, from
outside, crossing from outside to outside, across the buffer's wrap seam, and marking the same end cell repeatedly;
discs centred on cell edges and corners and clipped by every border; submap windows clipped at each border.

Where oracle/_ref is built the reference answers live; elsewhere against its recorded answers to exactly these inputs
(tests/golden/gridmap_ref_recorded.npz, written by tests/golden/gen_gridmap_ref_recorded.py).

Inputs on which the reference has no defined answer are generated too and then filtered out by name (EXCLUDED below);
each test asserts that the filter caught some and that the reference reported no out-of-range access on the rest.
"""
import collections
import ctypes as C
import functools
import hashlib
import math
import os

import numpy as np
import pytest

import _oracle as O

RECORDED = os.path.join(os.path.dirname(__file__), "golden", "gridmap_ref_recorded.npz")

# (length x, length y, resolution, position): non-square, off-origin; 0.03 is not exact in binary
BASES = [(1.0, 0.65, 0.025, (0.0, 0.0)),
         (2.3, 1.45, 0.05, (0.37, -1.21)),
         (3.1, 4.7, 0.1, (-2.35, 1.05)),
         (6.2, 3.8, 0.2, (5.1, -0.3)),
         (1.23, 0.87, 0.03, (0.41, 0.05))]
# GridMap::move shifts in cells, applied in turn: negative, fractional (rounds to 0 on one axis), larger than the map
MOVES = [(-3.4, 2.6), (0.37, -1.6), (1.3, -1.7)]   # the last one is in map lengths

# Inputs the reference leaves undefined, filtered out of every comparison with the reference.  Each is defined by the
# oracle and the kernels and covered elsewhere:
EXCLUDED = {
    # non-finite or longer than 2^20 cells: the clipping march (LineIterator.cpp:92-104) spins
    #   -> test_host_iterators.py::test_line_iterator_known_answers_of_the_reference, test_gpu_fuzz.py
    "malformed_ray",
    # zero length with its start outside the map: (end - start).normalized() is 0 / 0 and the march spins
    #   -> oracle/gridmath.c index_limited_to_map, test_host_iterators.py
    "zero_length_outside",
    # a position within rounding of the far edge: getIndexFromPosition gives index == size on an unmoved map and the
    #   reference indexes its matrix out of bounds
    #   -> test_oracle_gridmap.py::test_index_from_position_never_returns_an_index_past_the_map
    "far_edge",
    # a ray that misses the map: LineIterator's constructor initialises nothing and lineOnMap walks indeterminate
    #   counters (the cell lists below still compare it: the shim builds that iterator in zeroed storage, which is what
    #   LineIteratorTest.cpp:101-109 expects)  -> test_oracle_gridmap.py::test_line_iterator
    "ray_misses_map",
    # a disc whose corner lands on the far edge after limitPositionToRange: CircleIterator uses an uninitialised
    #   endIndex (see og_circle_cells)  -> test_host_iterators.py::test_index_math_and_walks_match_the_oracle
    "circle_corner_far_edge",
    # an RRT run that reaches the oracle's max_samples cap: extendTree's while(true) never ends
    #   -> test_oracle_misc.py::test_rrt_reaches_goal_and_is_collision_free
    "rrt_sample_cap",
}


def copy_geom(g):
    return O.raw_geom(tuple(g.len), tuple(g.pos), g.res, tuple(g.size), tuple(g.start))


def position(g, idx):
    p = O.d2(0.0, 0.0)
    assert O.lib().og_position_from_index(C.byref(g), O.i2(*idx), p)
    return (p[0], p[1])


def within(g, p):
    return bool(O.lib().og_position_within_map(O.d2(*p), g.len, g.pos))


def far_edge(g, p):
    """inside by checkIfPositionWithinMap's strict `<`, yet the index divides to the size (the oracle says outside)"""
    return within(g, p) and not O.lib().og_index_from_position(C.byref(g), O.d2(*p), O.i2(0, 0))


def limited(g, p):
    q = O.d2(*p)
    O.lib().og_limit_position_to_range(q, g.len, g.pos)
    return (q[0], q[1])


@functools.lru_cache(maxsize=None)
def geometries():
    """per base: the unmoved map, then the map after each of MOVES in turn (og_move; test_move pins it)"""
    out = []
    for lx, ly, res, pos in BASES:
        g = O.make_geom(lx, ly, res, *pos)
        out.append(copy_geom(g))
        layer = np.zeros(g.size[0] * g.size[1], np.float32)
        for k, (a, b) in enumerate(MOVES):
            d = (a * g.len[0], b * g.len[1]) if k == len(MOVES) - 1 else (a * res, b * res)
            O.move(g, [layer], (g.pos[0] + d[0], g.pos[1] + d[1]))
            out.append(copy_geom(g))
    return out


def special_point(g, rng):
    """a cell centre, a point on a cell edge or corner, a point on the map's border, or a point outside"""
    i, j = int(rng.integers(0, g.size[0])), int(rng.integers(0, g.size[1]))
    c = position(g, (i, j))
    h = 0.5 * g.res
    kind = int(rng.integers(0, 6))
    if kind == 0:
        return c
    if kind == 1:
        return (c[0] + h * rng.choice([-1, 1]), c[1])
    if kind == 2:
        return (c[0], c[1] + h * rng.choice([-1, 1]))
    if kind == 3:
        return (c[0] + h * rng.choice([-1, 1]), c[1] + h * rng.choice([-1, 1]))
    if kind == 4:   # on the border: the near edge (index 0) or the far one (index size, outside)
        a = int(rng.integers(0, 2))
        p = list(c)
        p[a] = g.pos[a] + 0.5 * g.len[a] * rng.choice([-1, 1])
        return tuple(p)
    return (g.pos[0] + g.len[0] * rng.uniform(-1.2, 1.2), g.pos[1] + g.len[1] * rng.uniform(-1.2, 1.2))


def rays_for(g, rng, n=90):
    """RAY_DTYPE array of adversarial rays on g (malformed and undefined ones included; see filter_rays)"""
    rays = []
    res = g.res

    def add(s, e, clear=None):
        rays.append((s[0], s[1], e[0], e[1], int(rng.random() < 0.3) if clear is None else clear, 0))

    for _ in range(n // 9):
        c = position(g, (int(rng.integers(0, g.size[0])), int(rng.integers(0, g.size[1]))))
        k = int(rng.integers(-12, 13)) * res
        add(c, (c[0] + k, c[1]))                                            # along an axis
        add(c, (c[0], c[1] + k))
        add(c, (c[0] + k, c[1] + k * rng.choice([-1, 1])))                  # exact diagonal
        add(special_point(g, rng), special_point(g, rng))                   # centres, edges, corners, border
        p = special_point(g, rng)
        add(p, p)                                                           # zero length
        a = int(rng.integers(0, 2))                                         # outside -> outside, across the map
        s, e = list(c), list(c)
        s[a] = g.pos[a] + g.len[a] * rng.uniform(0.55, 1.5)
        e[a] = g.pos[a] - g.len[a] * rng.uniform(0.55, 1.5)
        add(tuple(s), tuple(e))
        add((g.pos[0] + g.len[0] * rng.uniform(-1.5, 1.5), g.pos[1] + g.len[1] * 0.9), c)   # start outside
        # across the wrap seam: buffer rows / columns 0 and size - 1 are neighbours on a moved map
        j = int(rng.integers(0, g.size[1]))
        add(position(g, (0, j)), position(g, (g.size[0] - 1, int(rng.integers(0, g.size[1])))))
        i = int(rng.integers(0, g.size[0]))
        add(position(g, (i, g.size[1] - 1)), position(g, (int(rng.integers(0, g.size[0])), 0)))
    end = position(g, (int(rng.integers(0, g.size[0])), int(rng.integers(0, g.size[1]))))
    for _ in range(6):                                                      # the same end cell, marked again and again
        add(special_point(g, rng), end, clear=0)
    # ends within a few ulp of the far edge (index == size on an unmoved map)
    for a in range(2):
        e = list(position(g, (int(rng.integers(0, g.size[0])), int(rng.integers(0, g.size[1])))))
        e[a] = g.pos[a] - 0.5 * g.len[a]
        for _ in range(4):
            e[a] = float(np.nextafter(e[a], np.inf))
            add(g.pos, tuple(e), clear=0)
    # malformed rays (defined by the oracle, not by the reference)
    add((math.inf, 0.0), (0.0, 0.0))
    add((0.0, math.nan), (0.1, 0.1))
    add(g.pos, (g.pos[0] + 2.0 ** 21 * res, g.pos[1]))
    out = np.array(rays, O.RAY_DTYPE)
    rng.shuffle(out)
    return out


def ray_exclusion(g, r, for_himm):
    s, e = (float(r["sx"]), float(r["sy"])), (float(r["ex"]), float(r["ey"]))
    if not all(map(math.isfinite, s + e)) or math.hypot(e[0] - s[0], e[1] - s[1]) > 2.0 ** 20 * g.res:
        return "malformed_ray"
    if s == e and not within(g, s):
        return "zero_length_outside"
    if far_edge(g, s) or far_edge(g, e):
        return "far_edge"
    if for_himm and len(O.line_cells(g, s, e)) == 0:
        return "ray_misses_map"
    return None


def filter_rays(g, rays, for_himm, excluded):
    keep = []
    for k in range(len(rays)):
        why = ray_exclusion(g, rays[k], for_himm)
        if why is None:
            keep.append(k)
        else:
            excluded[why] += 1
    kept = rays[keep]
    assert all(ray_exclusion(g, r, for_himm) is None for r in kept)
    return kept


def seeded_layer(g, rng):
    """HIMM's thresholds and then some: NaN, negative, 0, 10, 150, 160, 170, 180, 1e3 and values between"""
    vals = np.array([np.nan, -3.0, 0.0, 10.0, 150.0, 160.0, 170.0, 180.0, 1e3, 5.0, 120.0, 149.99, 1e-30],
                    np.float32)
    return vals[rng.integers(0, len(vals), g.size[0] * g.size[1])]


# ---------------------------------------------------------------------------------------------
# the cases, one list per family (fixed seed)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20250611)
    ex = collections.Counter()
    line, himm, circle, window, subit = [], [], [], [], []
    for gi, g in enumerate(geometries()):
        rays = rays_for(g, rng)
        line.append((gi, filter_rays(g, rays, False, ex)))
        himm.append((gi, seeded_layer(g, rng), filter_rays(g, rays, True, ex)))
        discs = []
        for _ in range(40):
            c = special_point(g, rng)
            if rng.random() < 0.35:    # near a border (either side of it), so that the disc is clipped
                a = int(rng.integers(0, 2))
                c = list(c)
                c[a] = g.pos[a] + 0.5 * g.len[a] * rng.choice([-1, 1]) + g.res * rng.uniform(-3, 3)
                c = tuple(c)
            r = float(rng.choice([0.3, 0.3, 0.05, 0.12, 0.77, 2.0 * g.res, 0.5 * g.res]))
            corners = (limited(g, (c[0] + r, c[1] + r)), limited(g, (c[0] - r, c[1] - r)))
            if any(not O.lib().og_index_from_position(C.byref(g), O.d2(*q), O.i2(0, 0)) for q in corners):
                ex["circle_corner_far_edge"] += 1
                continue
            discs.append((c, r))
        circle.append((gi, discs))
        wins = []
        for _ in range(16):
            c = special_point(g, rng)
            if rng.random() < 0.5:     # at a border or corner
                for a in range(2):
                    if rng.random() < 0.7:
                        c = list(c)
                        c[a] = g.pos[a] + (0.5 * g.len[a] - g.res * rng.uniform(0, 4)) * rng.choice([-1, 1])
                        c = tuple(c)
            ln = [(1.5, 1.5), (0.3, 0.7), (2.2 * g.len[0], 0.5 * g.len[1]), (0.0, 0.0)][int(rng.integers(0, 4))]
            corners = (limited(g, (c[0] + 0.5 * ln[0], c[1] + 0.5 * ln[1])),
                       limited(g, (c[0] - 0.5 * ln[0], c[1] - 0.5 * ln[1])))
            if far_edge(g, c) or any(far_edge(g, q) for q in corners):
                ex["far_edge"] += 1
                continue
            wins.append((c, ln))
        window.append((gi, seeded_layer(g, rng), wins))
        tls = []
        for _ in range(12):
            tl = (int(rng.integers(0, g.size[0])), int(rng.integers(0, g.size[1])))
            sz = (int(rng.integers(1, g.size[0] + 1)), int(rng.integers(1, g.size[1] + 1)))
            tls.append((tl, sz))
        subit.append((gi, tls))
    move = [(bi, seeded_layer(O.make_geom(lx, ly, res, *pos), rng)) for bi, (lx, ly, res, pos) in enumerate(BASES)]
    return dict(line=line, himm=himm, circle=circle, window=window, subit=subit, move=move, rrt=rrt_cases(ex),
                excluded=ex)


def rrt_map(n_rows, n_cols, seed):
    rng = np.random.default_rng(seed)
    m = np.full((n_cols, n_rows), np.nan, np.float32)       # m[j, i]: column-major layer
    m[rng.random(m.shape) < 0.5] = 0.0
    for _ in range(6):
        i0, j0 = int(rng.integers(0, n_rows - 6)), int(rng.integers(0, n_cols - 6))
        m[j0:j0 + int(rng.integers(2, 12)), i0:i0 + int(rng.integers(2, 12))] = 100.0
    return m.reshape(-1)


def rrt_cases(ex):
    out = []
    for k, (rows, cols, res, pos) in enumerate([(40, 40, 0.05, (0.0, 0.0)), (64, 48, 0.05, (1.3, -0.4)),
                                               (100, 90, 0.05, (-2.0, 3.0)), (37, 53, 0.1, (0.0, 0.0)),
                                               # cells closer than the stride: samples land on cell centres, the same
                                               # centre twice gives two nodes at one position and exact nearest-node ties
                                               (30, 26, 0.2, (0.3, -0.2)), (24, 24, 0.25, (0.0, 0.0))]):
        g = O.make_geom(rows * res, cols * res, res, *pos)
        master = rrt_map(rows, cols, 100 + k)
        free = [(i, j) for i in range(2, rows - 2) for j in range(2, cols - 2)
                if not O.lib().og_if_blocked(C.byref(g), O.fptr(master), O.d2(*position(g, (i, j))))]
        rng = np.random.default_rng(200 + k)
        for q in range(5):
            s = position(g, free[int(rng.integers(0, len(free)))])
            if q < 3:    # the farthest of a few free cells
                cand = [position(g, free[int(rng.integers(0, len(free)))]) for _ in range(12)]
                t = max(cand, key=lambda p: math.hypot(p[0] - s[0], p[1] - s[1]))
            else:                # outside the map: plan to the border
                t = (g.pos[0] + g.len[0] * rng.choice([-0.8, 0.8]), g.pos[1] + g.len[1] * rng.uniform(-1, 1))
            for seed in (1, 2, 7):
                res_, _ = O.rrt_plan(g, master, s, t, seed=seed, max_samples=20000)
                if res_.status == -1:
                    ex["rrt_sample_cap"] += 1
                    continue
                out.append((k, g, master, s, t, seed))
    g = O.make_geom(1.0, 1.0, 0.05)   # no free cell at all: every extension is blocked
    res_, _ = O.rrt_plan(g, np.full(400, 100.0, np.float32), (0.0, 0.0), (0.3, 0.3), seed=1, max_samples=20000)
    if res_.status == -1:
        ex["rrt_sample_cap"] += 1
    return out


def inputs_digest():
    """sha256 of every input in cases(): the recorded answers belong to exactly these inputs"""
    h = hashlib.sha256()
    cs = cases()
    for g in geometries():
        h.update(bytes(g))
    for gi, rays in cs["line"]:
        h.update(rays.tobytes())
    for gi, layer, rays in cs["himm"]:
        h.update(layer.tobytes() + rays.tobytes())
    for gi, discs in cs["circle"]:
        h.update(repr(discs).encode())
    for gi, layer, wins in cs["window"]:
        h.update(layer.tobytes() + repr(wins).encode())
    for gi, tls in cs["subit"]:
        h.update(repr(tls).encode())
    for bi, layer in cs["move"]:
        h.update(layer.tobytes())
    for k, g, master, s, t, seed in cs["rrt"]:
        h.update(bytes(g) + master.tobytes() + repr((s, t, seed)).encode())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------
# answers: the same arrays from the oracle and from the reference
# ---------------------------------------------------------------------------------------------
def _ragged(lists, dtype, width):
    n = np.array([len(a) for a in lists], np.int32)
    flat = np.concatenate([np.asarray(a, dtype).reshape(-1, width) for a in lists]) if lists else np.zeros((0, width))
    return n, flat.astype(dtype)


def answers(family, reference):
    cs, geoms = cases(), geometries()
    if family == "line":
        out = [O.line_cells(geoms[gi], (r["sx"], r["sy"]), (r["ex"], r["ey"]), reference)
               for gi, rays in cs["line"] for r in rays]
        n, flat = _ragged(out, np.int16, 2)
        return {"line_n": n, "line_cells": flat}
    if family == "circle":
        out = [O.circle_cells(geoms[gi], c, r, reference) for gi, discs in cs["circle"] for c, r in discs]
        n, flat = _ragged(out, np.int16, 2)
        return {"circle_n": n, "circle_cells": flat}
    if family == "subit":
        out = [O.submap_cells(geoms[gi], tl, sz, reference) for gi, tls in cs["subit"] for tl, sz in tls]
        n, flat = _ragged(out, np.int16, 4)
        return {"subit_n": n, "subit_cells": flat}
    if family == "himm":
        layers = []
        for gi, layer, rays in cs["himm"]:
            a = layer.copy()
            (O.ref_himm_update if reference else O.himm_update)(geoms[gi], a, rays)
            layers.append(a)
        return {"himm_layers": np.concatenate(layers)}
    if family == "window":
        ok, geo, data, info = [], [], [], []
        for gi, layer, wins in cs["window"]:
            g = geoms[gi]
            for c, ln in wins:
                s, sub, d = O.get_submap(g, layer, c, ln, reference)
                ok.append(s)
                geo.append(list(sub.len) + list(sub.pos) + [sub.res] + list(sub.size) + list(sub.start) if s else [0.0] * 9)
                data.append(d)
                o = O.SubmapInfo()
                fn = O.ref_gridmap().refgm_submap_information if reference else O.lib().og_submap_information
                r = fn(C.byref(g), O.d2(*c), O.d2(*ln), C.byref(o))
                info.append([r] + list(o.top_left) + list(o.size) + list(o.pos) + list(o.len) + list(o.requested_index)
                            if r else [0] * 11)
        n, flat = _ragged(data, np.float32, 1)
        return {"window_ok": np.array(ok, np.int8), "window_geom": np.array(geo, np.float64), "window_n": n,
                "window_data": flat.reshape(-1), "window_info": np.array(info, np.float64)}
    if family == "move":
        regs, moved, geo, layers = [], [], [], []
        for bi, layer in cs["move"]:
            lx, ly, res, pos = BASES[bi]
            g = O.make_geom(lx, ly, res, *pos)
            a, b = layer.copy(), layer[::-1].copy()
            for k, (sx, sy) in enumerate(MOVES):
                d = (sx * g.len[0], sy * g.len[1]) if k == len(MOVES) - 1 else (sx * res, sy * res)
                rg, mv = O.move(g, [a, b], (g.pos[0] + d[0], g.pos[1] + d[1]), reference)
                regs.append(sum(([*i, *s, q] for i, s, q in rg), []) + [-1] * 5 * (4 - len(rg)))
                moved.append(mv)
                geo.append(list(g.len) + list(g.pos) + [g.res] + list(g.size) + list(g.start))
                layers += [a.copy(), b.copy()]
        return {"move_regions": np.array(regs, np.int32), "move_moved": np.array(moved, np.int8),
                "move_geom": np.array(geo, np.float64), "move_layers": np.concatenate(layers)}
    if family == "rrt":
        st, paths = [], []
        for k, g, master, s, t, seed in cs["rrt"]:
            if reference:
                res, path = O.ref_rrt_plan(g, master, s, t, seed=seed)
            else:
                res, path = O.rrt_plan(g, master, s, t, seed=seed, max_samples=20000, steer=0)
            st.append([res.status, res.tree_size, res.path_len])
            paths.append(path)
        n, flat = _ragged(paths, np.float64, 2)
        return {"rrt_status": np.array(st, np.int32), "rrt_n": n, "rrt_path": flat}
    raise KeyError(family)


FAMILIES = ["line", "circle", "subit", "himm", "window", "move", "rrt"]

# The window this pin found: centred on the far edge of the map (outside it by the strict `<`), whose requested position
# then lies within rounding of the SUBMAP's far edge.  getSubmapInformation succeeds there (the index it reports equals
# the submap's size, and nothing reads it); the oracle used to reject it, so og_get_submap failed where getSubmap does
# not.  tests/golden/submap_far_edge_case.npz holds the reference's answer.
SUBMAP_FAR_EDGE_CASE = {"geometry": (2.3, 1.45, 0.05, 0.37, -1.21), "center": (1.195, -1.935),
                        "length": (5.060000000000001, 0.7250000000000001)}
REGRESSION = os.path.join(os.path.dirname(__file__), "golden", "submap_far_edge_case.npz")


def reference_answers(family):
    """live from oracle/_ref when it is built, else the recorded answers to these very inputs"""
    if O.ref_gridmap() is not None:
        return answers(family, True)
    z = np.load(RECORDED)
    assert str(z["inputs_sha256"]) == inputs_digest(), "recorded answers belong to other inputs: regenerate them"
    return {k: z[k] for k in z.files if k.startswith(family + "_")}


def assert_same(got, want, what):
    assert set(got) == set(want)
    for k in got:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a != b) & ~(np.isnan(a.astype(float)) & np.isnan(b.astype(float))) if a.dtype.kind == "f"
                                 else (a != b).reshape(-1))
            pytest.fail("%s: %s differs from the reference at %d of %d entries, first at %s"
                        % (what, k, len(bad), a.size, bad[:5].tolist() if len(bad) else "(NaN payload / sign)"))


def case_index(family, flat_k):
    """the (geometry, input) of the k-th entry of a ragged family, for failure messages"""
    cs = cases()
    items = [(gi, x) for gi, xs in cs[family] for x in (xs if family != "himm" else [])]
    return items[flat_k] if flat_k < len(items) else None


# ---------------------------------------------------------------------------------------------
# 2. the Eigen stand-in checked first: the gtest answers against the reference build itself
# ---------------------------------------------------------------------------------------------
needs_ref = pytest.mark.skipif(O.ref_gridmap() is None and not os.path.exists(RECORDED),
                               reason="neither oracle/_ref/libref_gridmap.so nor its recording is present")


def _live():
    if O.ref_gridmap() is None:
        pytest.skip("oracle/_ref/libref_gridmap.so is not built here (the reference sources are absent)")
    return O.ref_gridmap()


def test_stand_in_reproduces_the_gtest_answers_of_grid_map_math():
    """GridMapMathTest.cpp:26-156, 404-597 (the answers of tests/test_oracle_gridmap.py) through the reference's own
    GridMapMath compiled against the Eigen stand-in"""
    R = _live()
    EPS = np.finfo(float).eps

    def pos(g, i, j):
        p = O.d2(0, 0)
        return bool(R.refgm_position_from_index(C.byref(g), O.i2(i, j), p)), (p[0], p[1])

    def idx(g, x, y):
        i = O.i2(0, 0)
        return bool(R.refgm_index_from_position(C.byref(g), O.d2(x, y), i)), (i[0], i[1])

    def deq(a, b):
        return abs(a - b) <= 4 * EPS * max(abs(a), abs(b), 1e-300) or a == b

    g = O.raw_geom((3.0, 2.0), (-1.0, 2.0), 1.0, (3, 2))
    for ij, e in (((0, 0), (1.0, 0.5)), ((1, 0), (0.0, 0.5)), ((1, 1), (0.0, -0.5)), ((2, 1), (-1.0, -0.5))):
        ok, p = pos(g, *ij)
        assert ok and deq(p[0], e[0] - 1.0) and deq(p[1], e[1] + 2.0)
    assert not pos(g, 3, 1)[0]
    g = O.raw_geom((0.5, 0.4), (-0.1, 13.4), 0.1, (5, 4), (3, 1))
    for ij, e in (((3, 1), (0.2, 0.15)), ((4, 2), (0.1, 0.05)), ((2, 0), (-0.2, -0.15)), ((0, 0), (0.0, -0.15)),
                  ((4, 3), (0.1, -0.05))):
        ok, p = pos(g, *ij)
        assert ok and deq(p[0], e[0] - 0.1) and deq(p[1], e[1] + 13.4)
    mp = (-12.4, -7.1)
    g = O.raw_geom((3.0, 2.0), mp, 1.0, (3, 2))
    for p, e in (((1.0, 0.5), (0, 0)), ((-1.0, -0.5), (2, 1)), ((0.6, 0.1), (0, 0)), ((0.4, -0.1), (1, 1)),
                 ((0.4, 0.1), (1, 0))):
        assert idx(g, p[0] + mp[0], p[1] + mp[1]) == (True, e)
    assert not idx(g, 4.0 + mp[0], 0.5 + mp[1])[0]
    g = O.raw_geom((3.0, 2.0), (0.0, 0.0), 1.0, (3, 2))
    assert idx(g, 0.0, EPS) == (True, (1, 0)) and idx(g, 0.5 - EPS, -EPS) == (True, (1, 1))
    assert idx(g, -0.5 - EPS, -EPS) == (True, (2, 1)) and not idx(g, -1.5, 1.0)[0]
    mp = (0.4, -0.9)
    g = O.raw_geom((0.5, 0.4), mp, 0.1, (5, 4), (3, 1))
    assert idx(g, 0.2 + mp[0], 0.15 + mp[1]) == (True, (3, 1)) and idx(g, 0.03 + mp[0], -0.17 + mp[1]) == (True, (0, 0))

    def info(g, rp, rl):
        o = O.SubmapInfo()
        return bool(R.refgm_submap_information(C.byref(g), O.d2(*rp), O.d2(*rl), C.byref(o))), o

    g = O.raw_geom((5.0, 4.0), (0.0, 0.0), 1.0, (5, 4))
    ok, o = info(g, (0.0, 0.5), (0.9, 2.9))
    assert ok and tuple(o.top_left) == (2, 0) and tuple(o.size) == (1, 3) and tuple(o.requested_index) == (0, 1)
    assert deq(o.pos[0], 0.0) and deq(o.pos[1], 0.5) and deq(o.len[0], 1.0) and deq(o.len[1], 3.0)
    ok, o = info(g, (2.0, 1.5), (2.9, 2.9))
    assert ok and tuple(o.top_left) == (0, 0) and tuple(o.size) == (2, 2) and deq(o.pos[0], 1.5) and deq(o.len[1], 2.0)
    g = O.raw_geom((5.0, 4.0), (0.0, 0.0), 1.0, (5, 4), (2, 1))
    ok, o = info(g, (0.0, 0.5), (0.9, 2.9))
    assert ok and tuple(o.top_left) == (4, 1) and tuple(o.size) == (1, 3) and tuple(o.requested_index) == (0, 1)
    g = O.raw_geom((4.98, 4.98), (-4.98, -5.76), 0.06, (83, 83), (0, 13))
    ok, o = info(g, (-7.44, -3.42), (0.12, 0.12))
    assert ok and tuple(o.size) == (2, 3) and deq(o.len[0], 0.12) and deq(o.len[1], 0.18)


def test_stand_in_reproduces_the_gtest_answers_of_the_iterators_and_move():
    """LineIteratorTest.cpp:45-109, SubmapIteratorTest.cpp:28-167, GridMapTest.cpp:57-85 through the reference build"""
    _live()
    g = O.make_geom(8.0, 5.0, 1.0)
    assert O.line_cells(g, (0.0, 0.0), (9.0, 6.0), True).tolist() == [[4, 2], [3, 1], [2, 1], [1, 0], [0, 0]]
    c = O.line_cells(g, (-7.0, -9.0), (8.0, 8.0), True).tolist()
    assert c[:3] == [[5, 4], [4, 3], [3, 2]] and 3 <= len(c) <= 6
    assert len(O.line_cells(g, (-8.0, 8.0), (8.0, 8.0), True)) == 0
    g = O.make_geom(8.1, 5.1, 1.0)
    assert O.submap_cells(g, (3, 1), (3, 2), True).tolist() == [[3, 1, 0, 0], [3, 2, 0, 1], [4, 1, 1, 0], [4, 2, 1, 1],
                                                                [5, 1, 2, 0], [5, 2, 2, 1]]
    layer = np.zeros(40, np.float32)
    regs, moved = O.move(g, [layer], (-3.0, -2.0), True)
    assert tuple(g.start) == (3, 2) and moved == 1
    assert [(i, s) for i, s, q in regs] == [((0, 0), (3, 5)), ((0, 0), (8, 2))]
    m = layer.reshape(5, 8).T
    for i in range(8):
        for j in range(5):
            assert math.isnan(m[i, j]) == (i < 3 or j < 2)
    assert O.submap_cells(g, (6, 3), (2, 4), True).tolist() == [[6, 3, 0, 0], [6, 4, 0, 1], [6, 0, 0, 2], [6, 1, 0, 3],
                                                                [7, 3, 1, 0], [7, 4, 1, 1], [7, 0, 1, 2], [7, 1, 1, 3]]


# ---------------------------------------------------------------------------------------------
# 3. the pins
# ---------------------------------------------------------------------------------------------
def test_the_generators_hit_every_undefined_case_and_filter_it():
    ex = cases()["excluded"]
    assert set(ex) == EXCLUDED, set(ex) ^ EXCLUDED
    assert sum(len(r) for _, r in cases()["line"]) > 1000 and len(cases()["rrt"]) >= 40


@needs_ref
def test_line_iterator_matches_the_reference():
    want = reference_answers("line")
    got = answers("line", False)
    assert_same(got, want, "og_line_cells")
    assert want["line_n"].sum() > 5000


@needs_ref
def test_circle_iterator_matches_the_reference():
    want = reference_answers("circle")
    assert_same(answers("circle", False), want, "og_circle_cells")
    assert (want["circle_n"] > 0).sum() > len(want["circle_n"]) // 2 and want["circle_n"].max() > 500


@needs_ref
def test_submap_iterator_matches_the_reference():
    assert_same(answers("subit", False), reference_answers("subit"), "og_submap_cells")


@needs_ref
def test_get_submap_matches_the_reference():
    want = reference_answers("window")
    assert_same(answers("window", False), want, "og_get_submap / og_submap_information")
    assert 0.6 < want["window_ok"].mean() < 1.0


@needs_ref
def test_move_matches_the_reference_whole_layers():
    """every cell of two layers after each move, the NaN it resets included, plus regions, start index and position"""
    want = reference_answers("move")
    assert_same(answers("move", False), want, "og_move")
    assert want["move_moved"].all() or want["move_moved"].any()


@needs_ref
def test_himm_update_matches_line_on_map():
    """og_himm_update against the reference's MapUpdater::lineOnMap, ray by ray in order, bit for bit on the layer"""
    want = reference_answers("himm")
    assert_same(answers("himm", False), want, "og_himm_update")
    # the thresholds were exercised: marked cells at each step of markCell's ladder survive in the answer
    v = want["himm_layers"]
    assert all((v == x).any() for x in (30.0, 180.0, 140.0, 0.0))


@needs_ref
def test_rrt_steer0_matches_make_plan():
    """og_rrt_plan_steer(steer=0) against srand(seed); RrtPlanner::makePlan: status, node count and every waypoint,
    bit for bit (both on this machine's glibc rand / atan2 / cos / sin)"""
    want = reference_answers("rrt")
    assert_same(answers("rrt", False), want, "og_rrt_plan_steer(steer=0)")
    st = want["rrt_status"]
    assert (st[:, 0] == 1).sum() > len(st) // 2 and st[:, 1].max() > 40


# ---------------------------------------------------------------------------------------------
# the product's host twins against the same reference answers
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "ros_navigation_amd", "csrc"), "-j4", "-s"])
    from ros_navigation_amd import capi
    return capi


def host_geom(capi, g):
    return capi.make_geometry(g.len[0], g.len[1], g.res, (g.pos[0], g.pos[1]), (g.start[0], g.start[1]))


@needs_ref
def test_host_walks_match_the_reference(capi):
    geoms, cs = geometries(), cases()
    hg = [host_geom(capi, g) for g in geoms]
    for h, g in zip(hg, geoms):
        assert (h.size[0], h.size[1], h.length[0], h.length[1]) == (g.size[0], g.size[1], g.len[0], g.len[1])
    got = [capi.line_cells(hg[gi], r["sx"], r["sy"], r["ex"], r["ey"]) for gi, rays in cs["line"] for r in rays]
    n, flat = _ragged(got, np.int16, 2)
    assert_same({"line_n": n, "line_cells": flat}, reference_answers("line"), "rna_line_cells")
    got = [capi.circle_cells(hg[gi], c[0], c[1], r) for gi, discs in cs["circle"] for c, r in discs]
    n, flat = _ragged(got, np.int16, 2)
    assert_same({"circle_n": n, "circle_cells": flat}, reference_answers("circle"), "rna_circle_cells")
    want = reference_answers("subit")
    got = [capi.submap_cells(hg[gi], tl, sz) for gi, tls in cs["subit"] for tl, sz in tls]   # buffer indices only
    n, flat = _ragged(got, np.int16, 2)
    assert np.array_equal(n, want["subit_n"]) and np.array_equal(flat, want["subit_cells"][:, :2]), "rna_submap_cells"


def test_submap_far_edge_regression_case():
    """og_get_submap on the window centred on the map's far edge: the reference's own answer (recorded)"""
    z = np.load(REGRESSION)
    g = O.make_geom(*z["geometry"], *z["position"])
    ok, sub, data = O.get_submap(g, z["layer"].copy(), tuple(z["center"]), tuple(z["length"]))
    assert ok
    assert np.array(list(sub.len) + list(sub.pos) + [sub.res] + list(sub.size), np.float64).tobytes() == z["ref_geom"].tobytes()
    assert data.tobytes() == z["ref_data"].tobytes()
