"""GPU: the paths through a tile job that the large square maps of the other A* tests reach seldom, at shapes where each of them
occurs in every batch -- first jobs of a bucket (a bucket of 8 000 is eight straight cells: searches run on into further ones), tiles
beyond the bucket's bound (far tiles), the first page of a tile, the start and the goal tile (also one and the same tile), column
candidates into rows 0 and 15 (maps two to seventeen tiles high, tiles of 64 x 16 cells), sticky turns.  Two maps whose sizes are
no multiples of the tile (192 x 80 has a whole number of tiles along i only, 130 x 260 along neither), 30 % and 45 % rectangles,
each also after GridMap::move (the search runs in map space, the tiles are cut there), at pipeline depth 1 (sixteen wavefronts per
query) and depth 4 (eight: the pipelined kernel).  Status, length, cost, every path cell and the settled count are the oracle's.

The inputs are a function of the case alone (inputs()), so that the premises -- the oracle finds a path for at least 48 of the 64
queries, at least one query has start and goal in one tile -- are checked on the CPU in test_premises_hold_without_a_gpu."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
from _gpu import R, to_buffer  # noqa: F401

RES = 0.05
NQ = 64
BUCKET = 8000
TI, TJ = 64, 16
CASES = [(192, 80, 0.30, False), (192, 80, 0.45, False), (130, 260, 0.30, False), (130, 260, 0.45, False),
         (192, 80, 0.30, True), (192, 80, 0.45, True), (130, 260, 0.30, True), (130, 260, 0.45, True)]
MOVE = (1.37, -0.82)      # 27 cells along one axis, 16 along the other: the seam runs through tiles
_cache = {}


def obstacles(rows, cols, density, seed):
    """rectangles of 2..9 cells a side up to `density`, a border; map order (linear = i + j * rows)"""
    rng = np.random.default_rng(seed)
    m = np.zeros((cols, rows), np.float32)
    while np.count_nonzero(m) < density * rows * cols:
        w, h = rng.integers(2, 10, 2)
        i0, j0 = rng.integers(0, rows), rng.integers(0, cols)
        m[j0:j0 + h, i0:i0 + w] = 180.0
    m[0, :] = m[-1, :] = 180.0
    m[:, 0] = m[:, -1] = 180.0
    return m.reshape(-1)


def geometry(rows, cols, moved):
    g = O.make_geom(rows * RES, cols * RES, RES)
    if moved:
        dummy = np.zeros(rows * cols, np.float32)
        ptrs = (C.POINTER(C.c_float) * 1)(O.fptr(dummy))
        regs, mv = (O.Region * 4)(), C.c_int(0)
        O.lib().og_move(C.byref(g), ptrs, 1, O.d2(*MOVE), regs, C.byref(mv))
        assert mv.value and tuple(g.start) != (0, 0)
    return g


def tile_of(g, lin):
    rows, cols = g.size[0], g.size[1]
    i, j = (lin % rows - g.start[0]) % rows, (lin // rows - g.start[1]) % cols      # map space
    return (i // TI) + (j // TJ) * ((rows + TI - 1) // TI)


def inputs(case):
    """master layer (buffer order), geometry, queries and the oracle's answers of a case, computed once"""
    if case not in _cache:
        rows, cols, density, moved = case
        seed = 11 + CASES.index(case)
        g = geometry(rows, cols, moved)
        master = to_buffer(obstacles(rows, cols, density, seed), rows, cols, g.start[0], g.start[1])   # laid out in map space
        rng = np.random.default_rng(1000 + seed)
        free = np.flatnonzero(master == 0)
        tiles = np.array([tile_of(g, int(c)) for c in free])
        q = np.zeros(NQ, np.dtype([("start", "<i4"), ("goal", "<i4")]))
        q["start"] = rng.choice(free, NQ)
        q["goal"] = rng.choice(free, NQ)
        for k in range(8):       # start and goal in one tile
            q["goal"][k] = rng.choice(free[tiles == tile_of(g, int(q["start"][k]))])
        q["goal"][8] = q["start"][8]
        q["goal"][9] = int(np.flatnonzero(master != 0)[5 * rows + 7])   # a blocked goal
        ref = [O.astar_query_on_map(g, master, q["start"][k], q["goal"][k]) for k in range(NQ)]
        _cache[case] = (master, g, q, ref)
    return _cache[case]


@pytest.mark.parametrize("case", CASES)
def test_premises_hold_without_a_gpu(case):
    master, g, q, ref = inputs(case)
    assert sum(r.status == 0 for r, _ in ref) >= 48
    same_tile = [k for k in range(NQ) if tile_of(g, int(q["start"][k])) == tile_of(g, int(q["goal"][k])) and q["start"][k] != q["goal"][k]]
    assert any(ref[k][0].status == 0 for k in same_tile)
    # several buckets per search, several tiles per path, both columns and rows of tiles crossed
    assert np.median([r.cost for r, _ in ref if r.status == 0]) > 4 * BUCKET
    assert ref[9][0].status != 0 and ref[8][0].status == 0 and ref[8][0].path_len == 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_tile_job_paths_match_the_oracle(R, case):
    rows, cols, density, moved = case
    master, g, q, ref = inputs(case)
    e = R.Engine(rows * RES, cols * RES, RES)
    assert (e.rows, e.cols) == (rows, cols)
    if moved:
        assert e.move(*MOVE)
    assert tuple(e.geometry().start_index) == tuple(g.start)
    e.upload(R.capi.LAYER_MASTER, master)
    queries = np.zeros(NQ, R.capi.ASTAR_QUERY_DTYPE)
    queries["start"], queries["goal"] = q["start"], q["goal"]
    for depth in (1, 4):
        e.astar_pipeline_depth(depth)
        e.astar_configure(max_queries=NQ, bucket_width=BUCKET)
        res, paths = e.astar(queries, rows * cols)
        settled = e.astar_settled(NQ)
        for k in range(NQ):
            ores, opath = ref[k]
            assert res["status"][k] == (0 if ores.status == 0 else 1), (depth, k, res[k])
            if ores.status == 0:
                assert res["path_len"][k] == ores.path_len and res["cost"][k] == ores.cost, (depth, k, res[k])
                assert np.array_equal(paths[k][:ores.path_len], opath), (depth, k)
                assert settled[k] == ores.settled, (depth, k, settled[k], ores.settled)
        c = e.astar_job_counters()      # (of this engine's batches so far)
        # the paths of a job this file is about did occur: searches that went on into a further bucket (first jobs, far tiles:
        # a search starts in the bucket of h(start) and runs as many more as its detours cost), sticky turns, turns that found nothing
        assert c["buckets"] > c["searches"] and c["sticky_turns"] > 0 and c["jobs_noop"] > 0, (depth, c)
    e.close()
