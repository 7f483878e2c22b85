"""Exploration frontiers on the GPU (rna_frontiers_build, csrc/frontier.hip) against an oracle written here in plain numpy /
Python from the definitions of include/rna.h: un-rotate to map space, free = known and not in the engine's own blocked set,
frontier = free with an unknown edge neighbour inside the map, flood-fill the 8-connected components, label = smallest buffer
index, records from the cells.  Integers only: every value is compared for equality.

The maps are small (130 x 70, 200 x 136, 192 x 160: two to twelve 64 x 64 tiles) and built so that clusters cross the tile
borders, the tile corner and -- on a moved map -- both buffer seams; the tests assert those properties on the ORACLE's answer,
so a map that stops exercising the seams fails loudly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
from _gpu import TABLE, UNREACHED, Hip, R, engine_centre, make_engine, to_buffer, to_map  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu

RES = 0.05
RNA_ECAPACITY, RNA_ESTATE = -4, -5
NAN = np.float32(np.nan)


# ---- the map generators ([j, i] arrays) ----
def explored_map(rows, cols, seed, rects=8, holes=12, specks=40):
    rng = np.random.default_rng(seed); m = np.full((cols, rows), np.nan, np.float32)
    for _ in range(rects):
        w, h = rng.integers(20, 70, 2); i, j = rng.integers(0, rows - 20), rng.integers(0, cols - 20); m[j:j + h, i:i + w] = 0.0
    m[60:68, 5:rows - 5] = 0.0; m[5:cols - 5, 60:68] = 0.0            # known bands across both tile borders at 64
    for _ in range(rects):
        w, h = rng.integers(1, 10, 2); i, j = rng.integers(0, rows - w), rng.integers(0, cols - h); m[j:j + h, i:i + w] = 180.0
    for _ in range(holes):
        w, h = rng.integers(1, 6, 2); i, j = rng.integers(0, rows - w), rng.integers(0, cols - h); m[j:j + h, i:i + w] = np.nan
    for _ in range(specks): m[rng.integers(0, cols), rng.integers(0, rows)] = 0.0
    return m
def serpentine(rows, cols, pitch=3):                                   # one-cell corridors in the unknown, joined at alternating ends
    m = np.full((cols, rows), np.nan, np.float32); js = list(range(1, cols - 1, pitch))
    for k, j in enumerate(js):
        m[j, 1:rows - 1] = 0.0
        if k + 1 < len(js): m[j:js[k + 1] + 1, rows - 2 if k % 2 == 0 else 1] = 0.0
    return m


# ---- the oracle ----
class Want:
    """the definitions' answer for the engine's present master layer and blocked set"""

    def __init__(self, e, R, field=None):
        rows, cols = e.rows, e.cols
        g = e.geometry()
        s0, s1 = g.start_index[0], g.start_index[1]
        self.rows, self.cols, self.s0, self.s1 = rows, cols, s0, s1
        m = to_map(e.download(R.capi.LAYER_MASTER), rows, cols, s0, s1)
        blocked = to_map(e.astar_blocked_mask(), rows, cols, s0, s1)
        unknown = np.isnan(m)
        free = ~unknown & (blocked == 0)
        nb = np.zeros_like(unknown)
        nb[1:, :] |= unknown[:-1, :]; nb[:-1, :] |= unknown[1:, :]; nb[:, 1:] |= unknown[:, :-1]; nb[:, :-1] |= unknown[:, 1:]
        fr = free & nb
        self.frontier = fr
        jj, ii = np.mgrid[0:cols, 0:rows]
        buf = ((jj + s1) % cols) * rows + (ii + s0) % rows                   # buffer linear index of map cell [j, i]
        self.buf = buf
        comp = np.full((cols, rows), -1, np.int64)
        self.clusters = []                                                   # lists of (i, j)
        for j0, i0 in zip(*np.nonzero(fr)):
            if comp[j0, i0] >= 0:
                continue
            k = len(self.clusters)
            comp[j0, i0] = k
            stack, cells = [(int(i0), int(j0))], []
            while stack:
                i, j = stack.pop()
                cells.append((i, j))
                for dj in (-1, 0, 1):
                    for di in (-1, 0, 1):
                        a, b = i + di, j + dj
                        if 0 <= a < rows and 0 <= b < cols and fr[b, a] and comp[b, a] < 0:
                            comp[b, a] = k
                            stack.append((a, b))
            self.clusters.append(cells)
        self.comp = comp
        labels = np.full(rows * cols, -1, np.int32)
        recs = []
        for cells in self.clusters:
            ci = np.array([c[0] for c in cells]); cj = np.array([c[1] for c in cells])
            b = buf[cj, ci]
            label = int(b.min())
            labels[b] = label
            cost, nearest = UNREACHED, label
            if field is not None:
                f = field[b].astype(np.int64)
                cost = int(f.min())
                nearest = int(b[f == cost].min())
            recs.append((label, len(cells), int(ci.min()), int(ci.max()), int(cj.min()), int(cj.max()), nearest, cost,
                         int(ci.sum()), int(cj.sum())))
        recs.sort()
        self.labels = labels
        self.records = recs
        self.cells = int(fr.sum())

    def kept(self, min_size):
        return [r for r in self.records if r[1] >= min_size]

    def tiles_of(self, cells):
        return {(i >> 6, j >> 6) for i, j in cells}

    def label_at(self, i, j):
        return int(self.labels[self.buf[j, i]])


def as_tuples(recs):
    return [tuple(int(v) for v in r) for r in recs]


def check(e, R, min_size=1, rank=False, want=None):
    """one build compared with the oracle: labels for every cell, records, order and info"""
    field = e.goal_field_download() if rank else None
    w = want if want is not None else Want(e, R, field)
    recs, info = e.frontiers(min_size=min_size, rank=rank)
    assert np.array_equal(e.frontier_labels(), w.labels)
    keep = w.kept(min_size)
    assert as_tuples(recs) == keep
    assert [r[0] for r in keep] == sorted(r[0] for r in keep)
    assert info == {"cells": w.cells, "clusters_all": len(w.records), "clusters": len(keep),
                    "largest": max([r[1] for r in w.records], default=0), "min_size": min_size, "ranked": int(rank), "stale": 0,
                    "reserved": 0}
    assert e.frontiers_info() == info
    assert e.frontier_labels_ptr()
    return w, recs


# ---- 1. explored maps: labels, records, info, order; the size filter; the capacity rules ----
@pytest.fixture(scope="module")
def scipy_count():
    from scipy import ndimage

    def count(fr):
        return ndimage.label(fr, structure=np.ones((3, 3), int))[1]
    return count


@pytest.mark.parametrize("seed", range(6))
def test_explored_map(R, seed, scipy_count):
    rows, cols = 130, 70
    e = make_engine(R, rows, cols)
    L, h = e._L, e.h
    # before any build
    lab = np.zeros(rows * cols, np.int32)
    assert L.rna_frontiers_download(h, lab.ctypes.data, lab.size) == RNA_ESTATE
    assert e.frontier_labels_ptr() is None
    assert e.frontiers_info() == dict.fromkeys(R.capi.FRONTIER_INFO_DTYPE.names, 0)
    e.upload(R.capi.LAYER_MASTER, explored_map(rows, cols, seed).reshape(-1))
    w, recs = check(e, R)
    if seed == 0:
        assert scipy_count(w.frontier) == len(w.clusters)
    # the map does what it is here for (asserted on the oracle's answer)
    sizes = [len(c) for c in w.clusters]
    largest = w.clusters[int(np.argmax(sizes))]
    assert len(w.clusters) >= 15 and len(w.tiles_of(largest)) >= 2 and sizes.count(1) >= 5
    assert 0 < len(w.kept(5)) < len(w.records)
    # min_size = 5: labels unchanged, records a subset
    _, recs5 = check(e, R, min_size=5, want=w)
    assert set(as_tuples(recs5)) < set(as_tuples(recs))
    # cap = the exact count
    n = len(w.records)
    exact, info = e.frontiers(cap=n)
    assert as_tuples(exact) == w.records and info["clusters"] == n
    # cap = count - 1: RNA_ECAPACITY, the true counts in info, out untouched, labels valid
    out = np.zeros(n - 1, R.capi.FRONTIER_DTYPE)
    out.view(np.uint8)[:] = 0xA5
    before = out.tobytes()
    info = np.zeros(1, R.capi.FRONTIER_INFO_DTYPE)
    assert L.rna_frontiers_build(h, 1, 0, out.ctypes.data, n - 1, info.ctypes.data) == RNA_ECAPACITY
    assert out.tobytes() == before
    assert (int(info["cells"][0]), int(info["clusters_all"][0]), int(info["clusters"][0])) == (w.cells, n, n)
    assert np.array_equal(e.frontier_labels(), w.labels)
    with pytest.raises(R.capi.RnaError, match="RNA_ECAPACITY.*%d clusters" % n):
        e.frontiers(cap=n - 1)
    # cap = 0 / NULL: count only
    info = np.zeros(1, R.capi.FRONTIER_INFO_DTYPE)
    assert L.rna_frontiers_build(h, 5, 0, None, 0, info.ctypes.data) == 0
    assert int(info["clusters"][0]) == len(w.kept(5)) and int(info["clusters_all"][0]) == n
    assert L.rna_frontiers_build(h, 1, 0, None, 0, None) == 0
    assert e.frontiers(cap=0)[1]["clusters"] == n
    e.close()


# ---- 2. one long component through every tile ----
def test_serpentine(R):
    rows, cols = 200, 136
    e = make_engine(R, rows, cols, serpentine(rows, cols).reshape(-1))
    w, recs = check(e, R)
    assert len(w.clusters) == 1 and len(w.tiles_of(w.clusters[0])) == 12
    r = recs[0]
    assert r["size"] == 8998 == w.cells and r["label"] == w.records[0][0]
    assert (r["min_i"], r["max_i"], r["min_j"], r["max_j"]) == (1, rows - 2, 1, 133)
    assert r["sum_i"] == w.records[0][8] and r["sum_j"] == w.records[0][9]
    assert r["sum_i"] > (1 << 16) and r["sum_j"] > (1 << 16)                 # sums of coordinates outgrow the coordinates' own width
    e.close()


# ---- 3. degenerate maps ----
def test_degenerate_maps(R):
    rows, cols = 130, 70
    e = make_engine(R, rows, cols)

    def run(m):
        e.upload(R.capi.LAYER_MASTER, m.reshape(-1))
        return check(e, R)

    for fill in (np.nan, 0.0, 180.0):                                        # all unknown, all free (the map edge is no frontier), all blocked
        w, recs = run(np.full((cols, rows), fill, np.float32))
        assert w.cells == 0 and len(recs) == 0 and (e.frontier_labels() == -1).all()
    m = np.zeros((cols, rows), np.float32)
    m[30, 40] = np.nan                                                       # the four edge neighbours touch by their diagonals
    w, recs = run(m)
    assert len(recs) == 1 and recs[0]["size"] == 4 and recs[0]["label"] == 40 + 29 * rows
    m = np.zeros((cols, rows), np.float32)
    m[0, 1] = np.nan                                                         # the free cell in the map's corner is a frontier cell
    w, recs = run(m)
    assert w.label_at(0, 0) >= 0 and len(recs) == 1 and recs[0]["size"] == 3 and recs[0]["label"] == 0
    m[cols - 1, rows - 2] = np.nan
    w, recs = run(m)
    assert w.label_at(rows - 1, cols - 1) >= 0 and len(recs) == 2
    # two frontier cells that touch only by the diagonal across the tile corner (63, 63) - (64, 64)
    m = np.full((cols, rows), np.nan, np.float32)
    m[63, 63] = m[64, 64] = 0.0
    w, recs = run(m)
    assert len(recs) == 1 and recs[0]["size"] == 2 and recs[0]["label"] == 63 + 63 * rows
    # ... and the other diagonal (64, 63) - (63, 64)
    m = np.full((cols, rows), np.nan, np.float32)
    m[63, 64] = m[64, 63] = 0.0
    w, recs = run(m)
    assert len(recs) == 1 and recs[0]["size"] == 2
    # two cells two apart: two clusters
    m = np.full((cols, rows), np.nan, np.float32)
    m[63, 63] = m[63, 65] = 0.0
    w, recs = run(m)
    assert len(recs) == 2 and [r["size"] for r in recs] == [1, 1]
    e.close()


# ---- 4. robot radius: frontier cells inside the inflated set disappear ----
def test_robot_radius(R):
    rows, cols = 130, 70
    e = make_engine(R, rows, cols, explored_map(rows, cols, 3).reshape(-1))
    w0, _ = check(e, R)
    e.astar_robot_radius(0.15)
    assert e.frontiers_info()["stale"] == 1
    assert np.array_equal(e.frontier_labels(), w0.labels)                     # a snapshot until it is rebuilt
    w1, _ = check(e, R)                                                      # (the oracle reads the engine's inflated blocked mask)
    assert not (w1.frontier & ~w0.frontier).any() and (w0.frontier & ~w1.frontier).any()
    assert not np.array_equal(w0.labels, w1.labels)
    check(e, R, min_size=5, want=w1)
    e.close()


# ---- 5. a moved map: clusters across both buffer seams, buffer neighbours that are no map neighbours ----
def test_moved_map(R):
    rows, cols = 130, 70
    e = make_engine(R, rows, cols, np.zeros(rows * cols, np.float32), pos=(1.25, -2.5))
    assert e.move(1.25 + 37 * RES, -2.5 - 22 * RES)
    g = e.geometry()
    s0, s1 = g.start_index[0], g.start_index[1]
    assert s0 % 64 != 0 and s1 % 64 != 0 and s0 != 0 and s1 != 0
    si, sj = rows - s0, cols - s1                                            # the seams lie before map column si and map row sj
    m = np.zeros((cols, rows), np.float32)
    m[sj - 2:sj + 2, si - 2:si + 2] = np.nan                                 # its ring of frontier cells lies across both seams
    m[20, 1] = m[20, rows - 2] = np.nan                                      # frontier cells (0, 20) and (rows - 1, 20): buffer neighbours
    m[1, 100] = m[cols - 2, 100] = np.nan                                    # ... (100, 0) and (100, cols - 1)
    m[40:44, 5:9] = 180.0
    e.upload(R.capi.LAYER_MASTER, to_buffer(m, rows, cols, s0, s1))
    w, recs = check(e, R)
    assert abs(int(w.buf[20, 0]) - int(w.buf[20, rows - 1])) == 1
    assert w.label_at(0, 20) >= 0 and w.label_at(rows - 1, 20) >= 0 and w.label_at(0, 20) != w.label_at(rows - 1, 20)
    assert abs(int(w.buf[0, 100]) - int(w.buf[cols - 1, 100])) == rows
    assert w.label_at(100, 0) >= 0 and w.label_at(100, cols - 1) >= 0 and w.label_at(100, 0) != w.label_at(100, cols - 1)
    seam = w.clusters[int(w.comp[sj - 3, si - 2])]
    assert len(seam) == 16
    assert {i >= si for i, _ in seam} == {False, True} and {j >= sj for _, j in seam} == {False, True}
    label = w.label_at(si - 2, sj - 3)
    j_min, i_min = min((j, i) for i, j in seam)                               # its smallest MAP index is not its label
    assert label != int(w.buf[j_min, i_min]) and label == int(w.buf[sj, si + 2])
    assert len(recs) == 5
    # the same with an explored map behind the moved origin: every seam case at once
    e.upload(R.capi.LAYER_MASTER, to_buffer(explored_map(rows, cols, 1), rows, cols, s0, s1))
    w, _ = check(e, R)
    assert len(w.clusters) >= 15
    check(e, R, min_size=5, want=w)
    e.close()


# ---- 6. ranking by the goal field ----
def room_map(rows, cols):
    m = np.full((cols, rows), np.nan, np.float32)
    m[9:61, 9:121] = 180.0
    m[10:60, 10:120] = 0.0                                                   # a walled room ...
    m[9, 20:23] = 0.0                                                        # ... with a gap near the robot
    m[40:43, 120] = 0.0                                                      # ... and one far from it: the unknown lies beyond both
    m[62:69, 28:42] = 180.0
    m[63:68, 29:41] = 0.0                                                    # a sealed room (the search crosses unknown cells, not walls)
    m[65, 33:37] = np.nan                                                    # ... with unknown cells inside: frontiers nobody can reach
    return m


@pytest.mark.parametrize("table", [None, TABLE])
def test_ranking(R, table):
    rows, cols = 130, 70
    e = make_engine(R, rows, cols, room_map(rows, cols).reshape(-1))
    if table is not None:
        e.goal_field_clearance_cost(table)
    with pytest.raises(R.capi.RnaError, match="RNA_ESTATE"):
        e.frontiers(rank=True)                                               # no field yet
    robot = 21 + 30 * rows
    assert e.goal_field(robot)["status"] == 0
    w, recs = check(e, R, rank=True)
    assert len(recs) == 3
    near, far, island = (recs[recs["label"] == w.label_at(i, j)][0] for i, j in ((21, 9), (120, 41), (33, 64)))
    assert 0 < near["cost"] < far["cost"] < 0x7ffffffe and island["cost"] == UNREACHED and island["nearest"] == island["label"]
    if table is None:
        assert near["cost"] == 1000 * 21 and near["nearest"] == 21 + 9 * rows and far["cost"] >= 1000 * 99
    for r in (near, far):
        paths, res = e.goal_field_paths([r["nearest"]], 512)
        assert res["status"][0] == 0 and res["cost"][0] == r["cost"] and paths[0, res["path_len"][0] - 1] == robot
    check(e, R, rank=False, want=Want(e, R))                                 # unranked again: cost / nearest are the defaults
    # an explored map, field rooted at a free cell
    mm = explored_map(rows, cols, 2)
    e.upload(R.capi.LAYER_MASTER, mm.reshape(-1))
    with pytest.raises(R.capi.RnaError, match="RNA_ESTATE"):
        e.frontiers(rank=True)                                               # the field is stale after the upload
    assert e.frontiers_info()["stale"] == 1
    assert mm[64, 30] == 0.0                                                 # (in the known band)
    assert e.goal_field(30 + 64 * rows)["status"] == 0
    w, recs = check(e, R, rank=True)
    costs = recs["cost"]
    assert (costs < 0x7ffffffe).sum() >= 3 and len(set(costs.tolist())) >= 4
    check(e, R, min_size=5, rank=True, want=w)
    e.close()


# ---- 7. a snapshot: stale after a HIMM batch, the rebuild equals a fresh engine's ----
def test_snapshot_and_stale(R):
    rows, cols = 130, 70
    m = np.full((cols, rows), np.nan, np.float32)
    m[20:50, 20:70] = 0.0
    m[30:33, 40:44] = 180.0
    master = m.reshape(-1)
    e = make_engine(R, rows, cols, master)
    e.upload(R.capi.LAYER_LASER, master)
    e.compose_master(1)
    old, _ = check(e, R)
    rs = np.zeros(1, R.capi.RAY_DTYPE)
    rs["sx"][0], rs["sy"][0] = engine_centre(e, 60 + 35 * rows)                     # from the known space out into the unknown
    rs["ex"][0], rs["ey"][0] = engine_centre(e, 90 + 35 * rows)
    e.update_map(rs, compose_mode=0)
    assert e.frontiers_info()["stale"] == 1
    assert np.array_equal(e.frontier_labels(), old.labels)                    # unchanged until a rebuild
    now = e.download(R.capi.LAYER_MASTER)
    assert np.isnan(now).sum() < np.isnan(master).sum()                      # the ray made unknown cells known
    new, _ = check(e, R)
    assert e.frontiers_info()["stale"] == 0 and not np.array_equal(new.labels, old.labels)
    fresh = make_engine(R, rows, cols, now)
    frecs, finfo = fresh.frontiers()
    recs, info = e.frontiers()
    assert np.array_equal(fresh.frontier_labels(), e.frontier_labels()) and frecs.tobytes() == recs.tobytes() and finfo == info
    fresh.close()
    e.close()


# ---- 8. with one pipelined batch in flight ----
def test_coexists_with_a_pipelined_batch(R):
    hip = Hip()
    rows, cols = 192, 160
    m = R.synth.obstacles_rect(rows, cols, density=0.2, seed=2).reshape(cols, rows).copy()
    m[:, 150:] = np.nan
    m[130:, :] = np.nan
    m[60:70, 60:70] = np.nan
    master = np.ascontiguousarray(m.reshape(-1))
    e = make_engine(R, rows, cols, master)
    blocked, nbr = O.astar_masks(master, rows, cols)
    e.astar_pipeline_depth(4)
    e.astar_configure(max_queries=32)
    nq, max_len = 32, 2048
    q = R.synth.astar_queries(nq, master, rows, cols, seed=21)
    d_q, d_paths, d_res = hip.upload(q), hip.alloc(nq * max_len * 4), hip.alloc(nq * 24)
    e.astar_device(d_q, nq, d_paths, max_len, d_res)
    w, recs = check(e, R)                                                    # built while the batch is in flight
    assert len(recs) >= 2 and max(len(w.tiles_of(c)) for c in w.clusters) >= 4
    e.synchronize()
    res = hip.download(d_res, R.capi.ASTAR_RESULT_DTYPE, nq)
    sp = hip.download(d_paths, np.int32, nq * max_len).reshape(nq, max_len)
    for k in range(nq):
        ores, opath, _ = O.astar_query(nbr, rows, cols, q["start"][k], q["goal"][k])
        assert (res["status"][k], res["path_len"][k], res["cost"][k]) == (ores.status, ores.path_len, ores.cost), k
        assert np.array_equal(sp[k][:ores.path_len], opath), k
    for p in (d_q, d_paths, d_res):
        hip.h.hipFree(p)
    e.close()


# ---- clones and submaps copy nothing of it ----
def test_clone_and_submap_copy_nothing(R):
    rows, cols = 130, 70
    e = make_engine(R, rows, cols, explored_map(rows, cols, 4).reshape(-1))
    e.frontiers()
    zero = dict.fromkeys(R.capi.FRONTIER_INFO_DTYPE.names, 0)
    h = C.c_void_p()
    assert e._L.rna_clone(e.h, C.byref(h)) == 0
    c = R.Engine.__new__(R.Engine)
    c._L, c.h, c.device, c.rows, c.cols, c.ncell, c.resolution, c.hist_size = e._L, h, e.device, rows, cols, rows * cols, e.resolution, None
    sub = e.submap_engine(0.0, 0.0, 2.0, 2.0)
    assert sub is not None
    for x in (c, sub):
        assert x.frontiers_info() == zero and x.frontier_labels_ptr() is None
        x.close()
    e.close()


# ---- the C++ layer ----
def test_find_frontiers_through_cpp(R, tmp_path):
    """tests/cpp/frontier_host_test.cpp runs findFrontiers and GridGoalField::frontiers on a moved map and checks every
    Frontier (size, centroid, bounding box, order, cost) against the labels the engine returns and against getPosition /
    costToGoal; a second map has more clusters than the first record buffer holds."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.join(root, "ros_navigation_amd")             # (librna.so is there: the R fixture has loaded it)
    exe = str(tmp_path / "frontier_host_test")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", os.path.join(root, "tests", "cpp", "frontier_host_test.cpp"), "-o", exe,
                           "-I" + os.path.join(root, "ros_navigation_amd", "host"), "-L" + lib_dir, "-lrna", "-Wl,-rpath," + lib_dir,
                           "-lpthread"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "frontier host OK" in run.stdout, run.stdout + run.stderr
