"""GPU parity tests of the grid-A* path walk over a per-tile parent map (tsa_backtrace_wave, astar_tile.hip): per tile the walking
wavefront works out every cell's parent at once, a step reads that code, and the cells leave 64 at a time.  Every batch runs at
pipeline depth 2 and is compared with the CPU oracle: status, cost, length and every cell of every path.  With 33 to 47 queries a
batch is walked by tsa_trace_kernel; the same cases once more with at most 32 queries, where the sixteen-wavefront search kernel
walks inside, and once with three pages per query, where the long searches are searched and walked again by the retry
instantiation.

  ties           an all-free 192 x 96 map: most cells have several parents that tie, the lowest linear index wins
  lengths        paths of 1 (start == goal), 2, 63, 64, 65, 128 and 129 cells on straight lines of that map: round the 64 cells a store
  crossings      pure diagonals that clip the four corner cells of tile (1, 2) and the cells next to them: they come in through each
                 edge and each corner and are out again after one or two cells
  partial tiles  200 x 150 with random rectangles, starts and goals in the strips of the partial tiles on both far edges
  moved map      the same with non-zero buffer start indices
  narrow         192 x 96 crossed by diagonal walls one cell thin with one-cell gaps: the move bits forbid to cut between two wall
                 cells, so the geometrically nearest parent is often not allowed
  status 3       max_path smaller than the path: status 3, the cost and the whole length all the same"""
import ctypes as C
import functools

import numpy as np
import pytest

from ros_navigation_amd import synth

import _oracle as O
from _gpu import R, make_engine_and_geom, to_map  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu

TI, TJ = 64, 16
ROWS, COLS = 192, 96
LENGTHS = (1, 2, 63, 64, 65, 128, 129)


def cell(i, j, rows=ROWS):
    return j * rows + i


def queries(pairs):
    q = np.zeros(len(pairs), synth.ASTAR_QUERY_DTYPE)
    q["start"] = [a for a, _ in pairs]
    q["goal"] = [b for _, b in pairs]
    return q


def filled(q, n, free, seed):
    """q and random queries over `free` behind it, n in all"""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, synth.ASTAR_QUERY_DTYPE)
    out[:len(q)] = q
    out["start"][len(q):], out["goal"][len(q):] = rng.choice(free, n - len(q)), rng.choice(free, n - len(q))
    return out


def frozen(m):
    m = np.ascontiguousarray(m, np.float32).reshape(-1)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def free_map():
    return frozen(np.zeros((COLS, ROWS), np.float32))


@functools.lru_cache(maxsize=None)
def rect_map():
    rows, cols = 200, 150
    m = frozen(synth.obstacles_rect(rows, cols, density=0.2, seed=32, side=(3, 20)))
    return rows, cols, m, np.flatnonzero(synth.free_component(m, rows, cols))


@functools.lru_cache(maxsize=None)
def narrow_map():
    """walls along i + j = 0 (mod 10) and i - j = 0 (mod 14), one cell thin, a cell left out here and there"""
    j, i = np.mgrid[0:COLS, 0:ROWS]
    wall = (((i + j) % 10 == 0) & (i % 7 != 3)) | (((i - j) % 14 == 0) & (i % 5 != 1))
    m = frozen(np.where(wall, 180.0, 0.0))
    return m, np.flatnonzero(synth.free_component(m, ROWS, COLS))


def length_queries():
    """straight lines of every length of LENGTHS along i (both ways), and the shorter ones along j"""
    pairs = []
    for n in LENGTHS:
        pairs.append((cell(20, 40), cell(20 + n - 1, 40)))
        pairs.append((cell(150, 50), cell(150 - (n - 1), 50)))
        if n <= COLS - 10:
            pairs.append((cell(30, 5), cell(30, 5 + n - 1)))
    return queries(pairs), [n for n in LENGTHS for _ in range(3 if n <= COLS - 10 else 2)]


def crossing_queries():
    """diagonals of 25 cells through the corner cells of tile (1, 2) -- i 64..127, j 32..47 -- and through their neighbours along the
    tile's top and bottom rows, in both diagonal directions and walked both ways"""
    pairs = []
    for pi in (64, 65, 126, 127):
        for pj in (32, 47):
            for dj in (1, -1):
                a, b = cell(pi - 12, pj - 12 * dj), cell(pi + 12, pj + 12 * dj)
                pairs += [(a, b), (b, a)]
    return queries(pairs)


def stays(path, rows):
    """lengths of the runs of consecutive cells of a path within one tile, and the tile offsets between the runs"""
    t = (path // rows // TJ) * 1000 + (path % rows) // TI
    cut = np.flatnonzero(np.diff(t)) + 1
    runs = np.diff(np.concatenate(([0], cut, [len(path)])))
    ti, tj = (path % rows) // TI, path // rows // TJ
    steps = set(zip(np.diff(ti)[cut - 1].tolist(), np.diff(tj)[cut - 1].tolist()))
    return runs, steps


_oracle_cache = {}


def oracle(g, ref, q):
    """[(result, path)] of the oracle, computed once per (geometry, map, query)"""
    out = []
    for k in range(len(q)):
        key = (tuple(g.start), tuple(g.size), ref.ctypes.data if not ref.flags.writeable else ref.tobytes(), int(q["start"][k]), int(q["goal"][k]))
        if key not in _oracle_cache:
            _oracle_cache[key] = O.astar_query_on_map(g, ref, q["start"][k], q["goal"][k])
        out.append(_oracle_cache[key])
    return out


def check(e, g, ref, q, max_len=None):
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


def engine(R, rows, cols, master, n=40):
    """an engine of the test's own at pipeline depth 2, closed by the test: one at a time, as in the other A* test files, so that
    the test process never holds more streams than one engine's (tests/test_gpu_bench_contract.py starts the full-size bench from
    this process, and the queues the process has made count against it)"""
    e, g = make_engine_and_geom(R, rows, cols, np.array(master))
    e.astar_pipeline_depth(2)
    e.astar_configure(max_queries=n)
    return e, g


# ---- the cases: name -> (rows, cols, map, 40 queries), with their premises checked on the CPU ----
@functools.lru_cache(maxsize=None)
def case(name):
    if name == "ties":
        m = free_map()
        return ROWS, COLS, m, filled(queries([]), 40, np.arange(ROWS * COLS), 3)
    if name == "lengths":
        q, _ = length_queries()
        return ROWS, COLS, free_map(), filled(q, 40, np.arange(ROWS * COLS), 4)
    if name == "crossings":
        return ROWS, COLS, free_map(), filled(crossing_queries(), 40, np.arange(ROWS * COLS), 5)
    if name == "partial tiles":
        rows, cols, m, free = rect_map()
        far_i, far_j = free[free % rows >= 3 * TI], free[free // rows >= 9 * TJ]
        assert len(far_i) > 50 and len(far_j) > 50
        rng = np.random.default_rng(6)
        q = np.zeros(40, synth.ASTAR_QUERY_DTYPE)
        q["start"] = np.concatenate((rng.choice(far_i, 10), rng.choice(far_j, 10), rng.choice(free, 10), rng.choice(far_i, 10)))
        q["goal"] = np.concatenate((rng.choice(free, 10), rng.choice(free, 10), rng.choice(far_j, 10), rng.choice(far_j, 10)))
        return rows, cols, m, q
    if name == "narrow":
        m, free = narrow_map()
        return ROWS, COLS, m, filled(queries([]), 40, free, 7)
    raise KeyError(name)


CASES = ("ties", "lengths", "crossings", "partial tiles", "narrow")


def premise(name, g, m, q):
    ref = oracle(g, m, q)
    rows = g.size[0]
    if name == "ties":
        assert sum(r.status == 0 and r.path_len > 20 for r, _ in ref) >= 30
    if name == "lengths":
        _, want = length_queries()
        assert [r.path_len for r, _ in ref[:len(want)]] == want and all(r.status == 0 for r, _ in ref[:len(want)])
    if name == "crossings":
        runs, steps = zip(*(stays(p, rows) for _, p in ref[:32]))
        assert all(r.status == 0 and r.path_len == 25 for r, _ in ref[:32])
        assert sum(1 in r[1:-1].tolist() for r in runs) >= 8 and sum(2 in r[1:-1].tolist() for r in runs) >= 8, runs    # stays of one and of two cells
        assert set().union(*steps) == {(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)} - {(0, 0)}, steps
    if name == "partial tiles":
        assert sum(r.status == 0 and r.path_len > 20 for r, _ in ref) >= 30
    if name == "narrow":
        assert sum(r.status == 0 and r.path_len > 40 for r, _ in ref) >= 30
        # cells whose diagonal neighbour is free and the move to it forbidden all the same: it would cut between two wall cells
        blocked, nbr = O.astar_masks(np.array(m), ROWS, COLS)
        b, n = blocked.reshape(COLS, ROWS), nbr.reshape(COLS, ROWS)
        cut = (b[1:, 1:] == 0) & (b[:-1, :-1] == 0) & ((n[1:, 1:] & 1) == 0)      # move 0 of (i, j): to (i - 1, j - 1)
        assert cut.sum() > 500, cut.sum()
    return ref


@pytest.mark.parametrize("name", CASES)
def test_the_trace_kernel_walks_the_parent_map(R, name):
    rows, cols, m, q = case(name)
    e, g = engine(R, rows, cols, m)
    premise(name, g, m, q)
    for _ in range(2):      # once on each stage
        check(e, g, m, q)
    e.close()


@pytest.mark.parametrize("name", CASES)
def test_the_sixteen_wavefront_kernel_walks_the_same_way(R, name):
    """at most 32 queries: the latency instantiation of the search kernel, which walks its path itself"""
    rows, cols, m, q = case(name)
    e, g = engine(R, rows, cols, m, 32)
    check(e, g, m, q[:32])
    e.close()


def test_a_path_longer_than_the_caller_asked_for(R):
    rows, cols, m, q = case("partial tiles")
    e, g = engine(R, rows, cols, m)
    lens = np.array([r.path_len for r, _ in oracle(g, m, q) if r.status == 0])
    # below, at and above a multiple of the 64 cells of a store
    for max_len in (63, 64, int(np.median(lens))):
        assert (lens > max_len).sum() >= 10 and (lens <= max_len).sum() >= 3, (max_len, lens)
        check(e, g, m, q, max_len=max_len)
    e.close()


def test_a_moved_map(R):
    """after GridMap::move the buffer's start index is not zero: the walk runs in map space and writes buffer indices"""
    rows, cols, m, _ = rect_map()
    e, g = engine(R, rows, cols, m)
    ref = np.array(m)
    for layer in range(3):
        e.upload(layer, ref)
    ptrs = (C.POINTER(C.c_float) * 1)(O.fptr(ref))
    regs, mv = (O.Region * 4)(), C.c_int(0)
    target = (-0.23 * rows * 0.05, 0.36 * cols * 0.05)
    O.lib().og_move(C.byref(g), ptrs, 1, O.d2(*target), regs, C.byref(mv))
    assert e.move(*target) and tuple(e.geometry().start_index) == tuple(g.start) and 0 not in tuple(g.start)
    s0, s1 = g.start[0], g.start[1]
    in_map = to_map(ref, rows, cols, s0, s1).reshape(-1)
    free = np.flatnonzero(synth.free_component(in_map, rows, cols))     # map-space indices
    rng = np.random.default_rng(19)
    a, b = rng.choice(free, 40), rng.choice(free, 40)
    q = np.zeros(40, synth.ASTAR_QUERY_DTYPE)
    for name, lin in (("start", a), ("goal", b)):
        q[name] = (lin % rows + s0) % rows + ((lin // rows + s1) % cols) * rows
    assert sum(r.status == 0 and r.path_len > 20 for r, _ in oracle(g, ref, q)) >= 20
    check(e, g, ref, q)
    e.close()


def test_the_retry_instantiation_walks_the_same_way(R):
    """three pages per query (rna_astar_set_page_cap): a search that settles more than three tiles' worth of cells ends its first pass
    with status 5, is searched again in a retry slot after the trace kernel has gone by, and walks its path there"""
    rows, cols, m, q = case("partial tiles")
    e, g = engine(R, rows, cols, m)
    assert sum(r.settled > 3 * TI * TJ for r, _ in oracle(g, m, q)) >= 4      # (more cells than three pages hold)
    e.astar_page_cap(3)
    for _ in range(2):
        check(e, g, m, q)
        assert e.astar_effective_config()[1] == 3
    e.close()
