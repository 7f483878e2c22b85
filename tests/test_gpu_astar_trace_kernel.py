"""GPU parity tests of the grid-A* trace kernel.  A pipelined batch of more than 32 queries is searched by the eight-wavefront
kernel, which leaves "found, path pending" (status 0, path_len 0) in the result record of a search that found its goal, and
tsa_trace_kernel behind it walks the paths: one wavefront per path, eight per workgroup, wavefront w of workgroup g serving position
8 g + w of the batch's launch order (astar_tile.hip).  Every batch here runs at pipeline depth 2 with 33 to 47 queries, so that this
is the way taken, and is compared with the CPU oracle: status, cost, length and every cell of every path.

Maps: 192 x 96 cells = 3 x 6 search tiles of 64 x 16, all free but for one closed room, where the shortest paths are known well enough
to say on the CPU which tile edge or corner they cross; and 200 x 150 with random rectangles and partial tiles on both far edges."""
import ctypes as C
import functools

import numpy as np
import pytest

from ros_navigation_amd import synth

import _oracle as O
from _gpu import R, make_engine_and_geom, to_buffer, to_map  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu

TI, TJ = 64, 16
ROWS, COLS = 192, 96
ROOM = (170, 80)          # a free 3 x 3 room behind a closed wall: its cells have free neighbours and cannot be reached


def cell(i, j, rows=ROWS):
    return j * rows + i


@functools.lru_cache(maxsize=None)
def open_map():
    m = np.zeros((COLS, ROWS), np.float32)   # m[j, i]
    i, j = ROOM
    m[j - 2:j + 3, i - 2:i + 3] = 180.0
    m[j - 1:j + 2, i - 1:i + 2] = 0.0
    m = m.reshape(-1)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def rect_map():
    rows, cols = 200, 150
    m = synth.obstacles_rect(rows, cols, density=0.2, seed=32, side=(3, 20))
    m.setflags(write=False)
    return rows, cols, m, np.flatnonzero(synth.free_component(m, rows, cols))


# from the middle tile (i 64..127, j 32..47) across each of its edges and, on a pure diagonal, through each of its corners; the walk
# goes from the goal back to the start, so each pair is there in both directions
CROSSINGS = [((96, 40), (96, 20)), ((96, 40), (96, 60)), ((96, 40), (40, 40)), ((96, 40), (150, 40)),
             ((72, 40), (56, 24)), ((120, 39), (136, 23)), ((72, 39), (56, 55)), ((120, 40), (136, 56))]
INSIDE = ((70, 20), (100, 28))     # both in tile (1, 1), and so is every shortest path between them


def directed_queries():
    pairs = [INSIDE] + CROSSINGS + [(b, a) for a, b in CROSSINGS]
    q = np.zeros(len(pairs), synth.ASTAR_QUERY_DTYPE)
    q["start"] = [cell(*a) for a, _ in pairs]
    q["goal"] = [cell(*b) for _, b in pairs]
    return q


def filled(q, n, free, seed):
    """q and random queries over `free` behind it, n in all"""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, synth.ASTAR_QUERY_DTYPE)
    out[:len(q)] = q
    out["start"][len(q):], out["goal"][len(q):] = rng.choice(free, n - len(q)), rng.choice(free, n - len(q))
    return out


_oracle_cache = {}


def oracle(g, ref, q):
    """[(result, path)] of the oracle in map space, computed once per (geometry, map, batch)"""
    key = (tuple(g.start), ref.tobytes(), q.tobytes())
    if key not in _oracle_cache:
        _oracle_cache[key] = [O.astar_query_on_map(g, ref, q["start"][k], q["goal"][k]) for k in range(len(q))]
    return _oracle_cache[key]


def check(e, g, ref, q, max_len=None):
    """the batch against the oracle; with a max_len shorter than a path that query must come back with status 3, the cost and
    the length of the whole path"""
    res, paths = e.astar(q, max_len or e.ncell)
    for k, (ores, opath) in enumerate(oracle(g, ref, q)):
        if ores.status == 0 and max_len and ores.path_len > max_len:
            assert (res["status"][k], res["cost"][k], res["path_len"][k]) == (3, ores.cost, ores.path_len), (k, q[k], res[k])
            continue
        assert res["status"][k] == ores.status, (k, q[k], res[k])
        if ores.status == 0:
            assert res["cost"][k] == ores.cost and res["path_len"][k] == ores.path_len, (k, q[k], res[k])
            assert np.array_equal(paths[k, :ores.path_len], opath), (k, q[k])
        else:
            assert res["path_len"][k] == 0, (k, q[k], res[k])
    return res, paths


def engine(R, rows, cols, master, depth, n):
    e, g = make_engine_and_geom(R, rows, cols, master.copy())
    e.astar_pipeline_depth(depth)
    e.astar_configure(max_queries=n)
    return e, g


def tile_steps(path, rows):
    """the set of (tile offset along i, along j) between consecutive cells of a path"""
    i, j = path % rows, path // rows
    di, dj = np.diff(i // TI), np.diff(j // TJ)
    return set(zip(di.tolist(), dj.tolist())) - {(0, 0)}


def test_paths_inside_a_tile_and_across_every_edge_and_corner(R):
    m = open_map()
    free = np.flatnonzero(synth.free_component(m, ROWS, COLS))
    q = filled(directed_queries(), 40, free, 5)
    e, g = engine(R, ROWS, COLS, m, 2, 40)
    ref = oracle(g, m, q)
    # the premise, on the CPU: one path never leaves its tile, and the others cross a tile border in each of the eight directions
    assert ref[0][0].status == 0 and tile_steps(ref[0][1], ROWS) == set()
    seen = set().union(*(tile_steps(p, ROWS) for _, p in ref[1:17]))
    assert seen == {(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)} - {(0, 0)}, seen
    check(e, g, m, q)
    e.close()


@pytest.mark.parametrize("n", [33, 40, 47])
def test_found_unreachable_and_one_cell_paths_share_a_trace_workgroup(R, n):
    """Every third query is answered without a path -- a goal in the closed room (the search floods the component: status 1), a
    start walled in the same way, an invalid index (status 2) -- and every ninth has start == goal, a path of one cell that must
    not be taken for the pending mark; the rest are found.  The launch order sorts by distance, so the kinds mix in the trace
    workgroups, and with 33, 40 and 47 queries the last workgroup has 1, 8 and 7 of its eight ranks inside the batch."""
    rows, cols, m0, _ = rect_map()
    m = m0.copy().reshape(cols, rows)
    ri, rj = 100, 75
    m[rj - 2:rj + 3, ri - 2:ri + 3] = 180.0
    m[rj - 1:rj + 2, ri - 1:ri + 2] = 0.0
    m = m.reshape(-1)
    free = np.flatnonzero(synth.free_component(m, rows, cols))
    q = filled(np.zeros(0, synth.ASTAR_QUERY_DTYPE), n, free, 9)
    k = np.arange(n)
    room = cell(ri, rj, rows)
    q["goal"][k % 9 == 0] = room
    q["start"][k % 9 == 3] = room + 1
    q["goal"][k % 9 == 6] = rows * cols
    q["goal"][k % 9 == 7] = q["start"][k % 9 == 7]
    e, g = engine(R, rows, cols, m, 2, n)
    ref = oracle(g, m, q)
    status = np.array([r.status for r, _ in ref])
    assert (status == 1).sum() >= n // 6 and (status == 2).sum() >= n // 10 and (status == 0).sum() >= n // 2, status
    assert sum(r.status == 0 and r.path_len == 1 for r, _ in ref) >= n // 12
    for _ in range(2):      # once on each stage
        res, _ = check(e, g, m, q)
    assert np.all(res["path_len"][status == 0] >= 1)
    e.close()


def test_a_path_longer_than_the_caller_asked_for(R):
    rows, cols, m, free = rect_map()
    q = filled(np.zeros(0, synth.ASTAR_QUERY_DTYPE), 40, free, 13)
    e, g = engine(R, rows, cols, m, 2, 40)
    lens = np.array([r.path_len for r, _ in oracle(g, m, q) if r.status == 0])
    max_len = int(np.median(lens))
    assert (lens > max_len).sum() >= 10 and (lens <= max_len).sum() >= 10, lens
    check(e, g, m, q, max_len=max_len)
    e.close()


def test_a_moved_map(R):
    """after GridMap::move the buffer's start index is not zero: the walk runs in map space and writes buffer indices"""
    rows, cols, m, _ = rect_map()
    e, g = engine(R, rows, cols, m, 2, 40)
    ref = m.copy()
    for layer in range(3):
        e.upload(layer, ref)
    ptrs = (C.POINTER(C.c_float) * 1)(O.fptr(ref))
    regs, mv = (O.Region * 4)(), C.c_int(0)
    target = (0.31 * rows * 0.05, -0.27 * cols * 0.05)
    O.lib().og_move(C.byref(g), ptrs, 1, O.d2(*target), regs, C.byref(mv))
    assert e.move(*target) and tuple(e.geometry().start_index) == tuple(g.start) and 0 not in tuple(g.start)
    s0, s1 = g.start[0], g.start[1]
    in_map = to_map(ref, rows, cols, s0, s1).reshape(-1)
    free = np.flatnonzero(synth.free_component(in_map, rows, cols))     # map-space indices
    rng = np.random.default_rng(17)
    a, b = rng.choice(free, 40), rng.choice(free, 40)
    q = np.zeros(40, synth.ASTAR_QUERY_DTYPE)
    for name, lin in (("start", a), ("goal", b)):
        q[name] = (lin % rows + s0) % rows + ((lin // rows + s1) % cols) * rows
    assert sum(r.status == 0 and r.path_len > 20 for r, _ in oracle(g, ref, q)) >= 20
    check(e, g, ref, q)
    e.close()


def test_the_walk_inside_the_search_kernel_gives_the_same_answers(R):
    """the same batch at depth 1, where the sixteen-wavefront kernel walks its path itself"""
    m = open_map()
    free = np.flatnonzero(synth.free_component(m, ROWS, COLS))
    q = filled(directed_queries(), 40, free, 5)
    q["goal"][20] = cell(*ROOM)
    out = []
    for depth in (2, 1):
        e, g = engine(R, ROWS, COLS, m, depth, 40)
        out.append(check(e, g, m, q))
        assert e.astar_effective_config()[0] == depth
        e.close()
    (res2, paths2), (res1, paths1) = out
    for name in ("status", "path_len", "cost"):
        assert np.array_equal(res2[name], res1[name]), name
    assert np.array_equal(paths2, paths1)
