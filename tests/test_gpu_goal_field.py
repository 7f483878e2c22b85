"""GPU: the goal distance field (rna_goal_field_*, csrc/goal_field.hip) against the CPU oracle, everything bit-exact.

The oracle is oracle/astar.c as it stands: og_astar_query(start = goal, goal = a blocked cell) floods the goal's
component, answers status 1 and leaves the complete exact distance field of the goal in its work array (the heuristic is
consistent, so every cell is closed once at its true distance; the adjacency is symmetric, so cost-to-goal = cost-from-
goal); og_astar_query(start = goal, goal = s) reversed is the field's path from s (the canonical backtrace is the rule the
field's `next` bytes store)."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
from _gpu import (NB_DI, NB_DJ, UNREACHED, Hip, R, blocked_of, centre, make_engine_and_geom, map_nbr,  # noqa: F401  (R: the fixture)
                  to_buffer, to_map)

pytestmark = pytest.mark.gpu

FAR = 0x7ffffffe
RES = 0.05


def add_pocket(master, rows, cols, i0, j0):
    """a closed 8 x 8 ring of obstacle with a free 4 x 4 interior; returns a cell of the interior"""
    m = master.reshape(cols, rows)
    m[j0:j0 + 8, i0:i0 + 8] = 180.0
    m[j0 + 2:j0 + 6, i0 + 2:i0 + 6] = 0.0
    return (i0 + 3) + (j0 + 3) * rows


def ref_field(nbr, rows, cols, goal, blocked):
    """(field, oracle result) of `goal` on an unmoved map: the oracle's flood towards a blocked cell"""
    b = int(np.flatnonzero(blocked)[-1])
    res, _, field = O.astar_query(nbr, rows, cols, goal, b)
    assert res.status == 1
    return field.copy(), res


def ref_path(nbr, rows, cols, goal, s):
    res, path, _ = O.astar_query(nbr, rows, cols, goal, s)
    return res, path[::-1].copy()


def check_field(e, info, field_ref, res):
    field = e.goal_field_download()
    bad = np.flatnonzero(field != field_ref)
    assert bad.size == 0, (bad[:10], field[bad[:10]], field_ref[bad[:10]])
    reached = field_ref != UNREACHED
    assert info["status"] == 0 and info["stale"] == 0
    assert info["reached"] == res.settled == int(reached.sum())
    assert info["max_cost"] == int(field_ref[reached].max())
    assert info["tile_jobs"] >= info["tiles_reached"] >= 1 and info["rounds"] >= 1
    return field


def check_paths(paths, results, starts, ref, max_len):
    """ref(s) -> (oracle result, reversed oracle path); returns the number of starts that answered status 0"""
    found = 0
    for k, s in enumerate(starts):
        ores, opath = ref(int(s))
        r = results[k]
        assert (r["expanded"], r["rounds"], r["buckets"]) == (0, 0, 0)
        if ores.status == 0 and ores.path_len > max_len:
            assert (r["status"], r["path_len"], r["cost"]) == (3, ores.path_len, ores.cost), k
            continue
        assert r["status"] == ores.status, (k, s, r, ores.status)
        if ores.status == 0:
            assert (r["path_len"], r["cost"]) == (ores.path_len, ores.cost), k
            assert np.array_equal(paths[k][:ores.path_len], opath), k
            assert paths[k][0] == s
            found += 1
    return found


def walk_next(nx, rows, cols, s, start_index=(0, 0)):
    """the path the `next` bytes spell from buffer cell s (host side, map-space steps)"""
    s0, s1 = start_index
    i, j = (s % rows - s0) % rows, (s // rows - s1) % cols
    out = []
    while True:
        b = (i + s0) % rows + ((j + s1) % cols) * rows
        out.append(b)
        k = int(nx[b])
        if k == 8:
            return np.array(out, np.int32)
        assert k < 8, (b, k)
        i, j = i + NB_DI[k], j + NB_DJ[k]


def maps_for(R, rows, cols, kind):
    if kind == "sparse":
        return R.synth.occupancy_sparse(rows, cols, seed=rows + 1)
    return R.synth.obstacles_rect(rows, cols, density=kind, seed=cols + 3)


@pytest.mark.parametrize("kind", [0.1, 0.3, "sparse"])
@pytest.mark.parametrize("rows,cols", [(96, 80), (192, 160), (200, 333), (1024, 1024)])
def test_field_parity(R, rows, cols, kind):
    master = maps_for(R, rows, cols, kind).copy()
    pocket = add_pocket(master, rows, cols, rows // 3, cols // 2)
    e, g = make_engine_and_geom(R, rows, cols, master)
    blocked, nbr = O.astar_masks(master, rows, cols)
    assert np.array_equal(e.nbr_mask(), nbr)
    comp = np.flatnonzero(R.synth.free_component(master, rows, cols))
    rng = np.random.default_rng(rows * 7 + cols)
    n_free = int((blocked == 0).sum())
    for goal in list(rng.choice(comp, 2)) + [pocket]:
        info = e.goal_field(int(goal))
        assert info["goal"] == goal and e.goal_field_info() == info
        field_ref, res = ref_field(nbr, rows, cols, int(goal), blocked)
        check_field(e, info, field_ref, res)
        if goal == pocket:
            assert info["reached"] == 16
        else:
            assert 2 * info["reached"] >= n_free, (info, n_free)
    e.close()


def test_empty_map_is_octile_distance(R):
    rows, cols = 200, 333
    e, g = make_engine_and_geom(R, rows, cols, np.full(rows * cols, np.nan, np.float32))
    goal = 77 + 150 * rows
    info = e.goal_field(goal)
    i, j = np.meshgrid(np.arange(rows), np.arange(cols))          # [j, i]
    dx, dy = np.abs(i - 77), np.abs(j - 150)
    want = (1000 * np.maximum(dx, dy) + 414 * np.minimum(dx, dy)).astype(np.int32).reshape(-1)
    assert np.array_equal(e.goal_field_download(), want)
    assert info["reached"] == rows * cols and info["max_cost"] == int(want.max()) and info["status"] == 0
    e.close()


def paths_case(R, rows=192, cols=160, density=0.3, seed=5):
    master = R.synth.obstacles_rect(rows, cols, density=density, seed=seed).copy()
    pocket = add_pocket(master, rows, cols, 120, 30)
    blocked, nbr = O.astar_masks(master, rows, cols)
    comp = np.flatnonzero(R.synth.free_component(master, rows, cols))
    rng = np.random.default_rng(seed)
    goal = int(rng.choice(comp))
    starts = np.concatenate([rng.choice(comp, 256), [goal, np.flatnonzero(blocked)[7], pocket, -1, rows * cols]]).astype(np.int32)
    return master, blocked, nbr, goal, starts


def test_paths_match_reversed_oracle_paths(R):
    rows, cols = 192, 160
    master, blocked, nbr, goal, starts = paths_case(R)
    e, g = make_engine_and_geom(R, rows, cols, master)
    info = e.goal_field(goal)
    assert 2 * info["reached"] >= int((blocked == 0).sum())
    ref = lambda s: ref_path(nbr, rows, cols, goal, s)   # noqa: E731
    paths, results = e.goal_field_paths(starts, 4096)
    found = check_paths(paths, results, starts, ref, 4096)
    assert found >= 0.9 * 256
    assert list(results["status"][-5:]) == [0, 1, 1, 2, 2]
    assert (results["path_len"][256], results["cost"][256], paths[256][0]) == (1, 0, goal)
    # a bound shorter than some paths: status 3 with the true length for exactly those
    lens = results["path_len"][:256]
    cut = int(np.median(lens[results["status"][:256] == 0]))
    paths2, results2 = e.goal_field_paths(starts, cut)
    check_paths(paths2, results2, starts, ref, cut)
    longer = (results["status"] == 0) & (results["path_len"] > cut)
    assert longer.any() and np.array_equal(results2["status"] == 3, longer)
    assert np.array_equal(results2["path_len"][longer], results["path_len"][longer])
    # the next bytes spell the same paths on the host
    field, nx = e.goal_field_download(want_next=True)
    assert nx[goal] == 8 and (nx[field == UNREACHED] == 255).all() and (nx[field != UNREACHED] <= 8).all()
    for k in np.flatnonzero(results["status"] == 0)[:64]:
        assert np.array_equal(walk_next(nx, rows, cols, int(starts[k])), paths[k][:results["path_len"][k]])
    e.close()


def test_agrees_with_the_batch_search(R):
    rows, cols = 192, 160
    master, blocked, nbr, goal, starts = paths_case(R, seed=8)
    starts = starts[:257]
    e, g = make_engine_and_geom(R, rows, cols, master)
    e.goal_field(goal)
    paths, results = e.goal_field_paths(starts, 4096)
    q = np.zeros(len(starts), R.capi.ASTAR_QUERY_DTYPE)
    q["start"], q["goal"] = goal, starts
    sres, spaths = e.astar(q, 4096)
    assert np.array_equal(sres["status"], results["status"]) and (results["status"] == 0).sum() >= 0.9 * 256
    for k in np.flatnonzero(results["status"] == 0):
        n = results["path_len"][k]
        assert sres["path_len"][k] == n and sres["cost"][k] == results["cost"][k]
        assert np.array_equal(spaths[k][:n][::-1], paths[k][:n])
    e.close()


def test_robot_radius(R):
    rows = cols = 256
    master = R.synth.obstacles_rect(rows, cols, density=0.1, seed=4)
    e, g = make_engine_and_geom(R, rows, cols, master)
    e.astar_robot_radius(0.3)
    nbr, blocked = e.nbr_mask(), e.astar_blocked_mask()
    assert blocked.sum() > blocked_of(master).sum()
    comp = np.flatnonzero(R.synth.free_component(blocked.astype(np.float32), rows, cols))
    rng = np.random.default_rng(12)
    goal = int(rng.choice(comp))
    info = e.goal_field(goal)
    field_ref, res = ref_field(nbr, rows, cols, goal, blocked)
    check_field(e, info, field_ref, res)
    assert 2 * info["reached"] >= int((blocked == 0).sum())
    band = np.flatnonzero((blocked == 1) & (blocked_of(master) == 0))
    starts = np.concatenate([rng.choice(comp, 62), band[:2]]).astype(np.int32)
    paths, results = e.goal_field_paths(starts, 4096)
    found = check_paths(paths, results, starts, lambda s: ref_path(nbr, rows, cols, goal, s), 4096)
    assert found >= 0.9 * 62 and list(results["status"][-2:]) == [1, 1]   # inside the inflated band: as a blocked start
    e.close()


def test_moved_map(R):
    rows, cols = 200, 170
    master = R.synth.obstacles_rect(rows, cols, density=0.2, seed=6).copy()
    m = master.reshape(cols, rows)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 0.0     # no border wall: it would lie along the buffer seam after the move
    e, g = make_engine_and_geom(R, rows, cols, master, pos=(1.25, -2.5))
    ref = master.copy()
    ptrs = (C.POINTER(C.c_float) * 1)(O.fptr(ref))
    regs = (O.Region * 4)()
    mv = C.c_int(0)
    target = (1.25 + 67 * RES, -2.5 - 22 * RES)   # 67 and 22 cells: no multiple of the 64-cell tile
    O.lib().og_move(C.byref(g), ptrs, 1, O.d2(*target), regs, C.byref(mv))
    assert e.move(*target) and tuple(e.geometry().start_index) == tuple(g.start)
    s0, s1 = g.start[0], g.start[1]
    assert s0 % 64 != 0 and s1 % 64 != 0
    blocked = blocked_of(ref)
    nbr = map_nbr(g, blocked)
    assert np.array_equal(e.nbr_mask(), nbr)

    def flat_map(a):     # buffer order -> map order, flat
        return np.ascontiguousarray(to_map(a, rows, cols, s0, s1).reshape(-1))

    def lin_to_map(c):
        return (c % rows - s0) % rows + ((c // rows - s1) % cols) * rows

    comp = np.flatnonzero(R.synth.free_component(flat_map(ref), rows, cols))       # map-space cells
    comp = (comp % rows + s0) % rows + ((comp // rows + s1) % cols) * rows        # -> buffer cells
    rng = np.random.default_rng(3)
    goal = int(rng.choice(comp))
    info = e.goal_field(goal)
    field_map, res = ref_field(flat_map(nbr), rows, cols, lin_to_map(goal), flat_map(blocked))
    field_ref = to_buffer(field_map, rows, cols, s0, s1)
    check_field(e, info, field_ref, res)
    assert 2 * info["reached"] >= int((blocked == 0).sum())
    starts = rng.choice(comp, 64).astype(np.int32)
    paths, results = e.goal_field_paths(starts, 4096)

    def ref_on_map(s):
        ores, p = O.astar_query_on_map(g, ref, goal, s)
        return ores, p[::-1].copy()

    found = check_paths(paths, results, starts, ref_on_map, 4096)
    assert found >= 0.9 * 64
    seam = 0
    for k in np.flatnonzero(results["status"] == 0):
        p = paths[k][:results["path_len"][k]]
        seam += int((np.abs(np.diff(p % rows)) > 1).any() or (np.abs(np.diff(p // rows)) > 1).any())
    assert seam >= 1
    field, nx = e.goal_field_download(want_next=True)
    k = int(np.flatnonzero(results["status"] == 0)[0])
    assert np.array_equal(walk_next(nx, rows, cols, int(starts[k]), (s0, s1)), paths[k][:results["path_len"][k]])
    e.close()


def test_snapshot_and_stale(R):
    """two rooms, a wall along j = 64 with two doors; a HIMM batch closes the door the paths use"""
    rows = cols = 128
    m = np.zeros((cols, rows), np.float32)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 180.0
    m[64, :] = 180.0
    m[64, 20:23] = 0.0
    m[64, 100:103] = 0.0
    master = m.reshape(-1)
    e, g = make_engine_and_geom(R, rows, cols, master)
    e.upload(R.capi.LAYER_LASER, master)
    e.compose_master(1)
    goal = 21 + 20 * rows
    rng = np.random.default_rng(1)
    starts = (rng.integers(5, 45, 32) + rng.integers(70, 120, 32) * rows).astype(np.int32)
    blocked, nbr = O.astar_masks(master, rows, cols)
    old_field, old_res = ref_field(nbr, rows, cols, goal, blocked)
    old = lambda s: ref_path(nbr, rows, cols, goal, s)   # noqa: E731
    info = e.goal_field(goal)
    check_field(e, info, old_field, old_res)
    paths, results = e.goal_field_paths(starts, 2048)
    assert check_paths(paths, results, starts, old, 2048) == 32
    door = [i + 64 * rows for i in (20, 21, 22)]
    assert all(np.isin(door, paths[k][:results["path_len"][k]]).any() for k in range(32))
    assert e.goal_field_info()["stale"] == 0
    # close the door: one marking ray per door cell, from inside the far room
    rs = np.zeros(3, O.RAY_DTYPE)
    for k, d in enumerate(door):
        rs["sx"][k], rs["sy"][k] = centre(g, d + 4 * rows)
        rs["ex"][k], rs["ey"][k] = centre(g, d)
    ref = master.copy()
    O.himm_update(g, ref, rs)
    assert (ref[door] > 0).all()
    e.update_map(rs.view(R.capi.RAY_DTYPE), compose_mode=0)
    assert np.array_equal(e.download(R.capi.LAYER_MASTER), ref, equal_nan=True)
    assert e.goal_field_info()["stale"] == 1
    # the snapshot still answers as before
    assert np.array_equal(e.goal_field_download(), old_field)
    paths_b, results_b = e.goal_field_paths(starts, 2048)
    assert np.array_equal(paths_b, paths) and np.array_equal(results_b, results)
    # rebuild: the new map's answers
    blocked2, nbr2 = O.astar_masks(ref, rows, cols)
    assert np.array_equal(e.nbr_mask(), nbr2)
    info = e.goal_field(goal)
    new_field, new_res = ref_field(nbr2, rows, cols, goal, blocked2)
    check_field(e, info, new_field, new_res)
    assert e.goal_field_info()["stale"] == 0 and not np.array_equal(new_field, old_field)
    paths_c, results_c = e.goal_field_paths(starts, 2048)
    assert check_paths(paths_c, results_c, starts, lambda s: ref_path(nbr2, rows, cols, goal, s), 2048) == 32
    assert (results_c["cost"] > results["cost"]).all()
    e.close()


def test_coexists_with_pipelined_batches(R):
    hip = Hip()
    rows = cols = 512
    master = R.synth.obstacles_rect(rows, cols, density=0.3, seed=2)
    e, g = make_engine_and_geom(R, rows, cols, master)
    blocked, nbr = O.astar_masks(master, rows, cols)
    e.astar_pipeline_depth(4)
    e.astar_configure(max_queries=64)
    nq, max_len = 64, 4096
    issued = []
    for b in range(2):
        q = R.synth.astar_queries(nq, master, rows, cols, seed=20 + b)
        d_q, d_paths, d_res = hip.upload(q), hip.alloc(nq * max_len * 4), hip.alloc(nq * 24)
        e.astar_device(d_q, nq, d_paths, max_len, d_res)
        issued.append((q, d_q, d_paths, d_res))
    goal = int(issued[0][0]["goal"][0])
    info = e.goal_field(goal)                                   # while the two batches are in flight
    starts = issued[1][0]["start"].astype(np.int32)
    paths, results = e.goal_field_paths(starts, max_len)
    e.synchronize()
    for q, d_q, d_paths, d_res in issued:
        res = hip.download(d_res, R.capi.ASTAR_RESULT_DTYPE, nq)
        sp = hip.download(d_paths, np.int32, nq * max_len).reshape(nq, max_len)
        for k in range(nq):
            ores, opath, _ = O.astar_query(nbr, rows, cols, q["start"][k], q["goal"][k])
            assert (res["status"][k], res["path_len"][k], res["cost"][k]) == (ores.status, ores.path_len, ores.cost), k
            assert np.array_equal(sp[k][:ores.path_len], opath), k
        for p in (d_q, d_paths, d_res):
            hip.h.hipFree(p)
    field_ref, res = ref_field(nbr, rows, cols, goal, blocked)
    check_field(e, info, field_ref, res)
    assert check_paths(paths, results, starts, lambda s: ref_path(nbr, rows, cols, goal, s), max_len) >= 0.9 * nq
    e.close()


def test_bench_size_once(R):
    """the bench's map (4096 x 4096, config 3): the whole field and 256 paths; the device-pointer form gives the same bytes"""
    hip = Hip()
    n = 4096
    master = R.synth.obstacles_rect(n, n)
    e, g = make_engine_and_geom(R, n, n, master)
    blocked, nbr = O.astar_masks(master, n, n)
    q = R.synth.astar_queries(256, master, n, n)
    goal = int(q["goal"][0])
    info = e.goal_field(goal)
    print("4096^2 build:", info)
    field_ref, res = ref_field(nbr, n, n, goal, blocked)
    check_field(e, info, field_ref, res)
    assert 2 * info["reached"] >= int((blocked == 0).sum())
    starts = q["start"].astype(np.int32)
    max_len = 16384
    paths, results = e.goal_field_paths(starts, max_len)
    g_work = np.empty(n * n, np.int32)
    found = 0
    for k, s in enumerate(starts):
        ores, opath, _ = O.astar_query(nbr, n, n, goal, int(s), path_cap=max_len, g_work=g_work)
        assert (results["status"][k], results["path_len"][k], results["cost"][k]) == (ores.status, ores.path_len, ores.cost), k
        assert np.array_equal(paths[k][:ores.path_len], opath[::-1]), k
        found += int(ores.status == 0)
    assert found >= 0.9 * 256
    d_s, d_paths, d_res = hip.upload(starts), hip.alloc(256 * max_len * 4), hip.alloc(256 * 24)
    assert hip.h.hipMemset(d_paths, 0, 256 * max_len * 4) == 0
    e.goal_field_paths_device(d_s, 256, d_paths, max_len, d_res)
    e.synchronize_map()
    assert np.array_equal(hip.download(d_res, R.capi.ASTAR_RESULT_DTYPE, 256), results)
    assert np.array_equal(hip.download(d_paths, np.int32, 256 * max_len).reshape(256, max_len), paths)
    assert e.goal_field_ptr()
    f_dev = hip.download(e.goal_field_ptr(), np.int32, n * n)
    assert np.array_equal(f_dev, field_ref)
    for p in (d_s, d_paths, d_res):
        hip.h.hipFree(p)
    e.close()


def test_error_paths_on_a_live_engine(R):
    rows, cols = 96, 80
    master = R.synth.obstacles_rect(rows, cols, density=0.1, seed=1)
    e, g = make_engine_and_geom(R, rows, cols, master)
    L, h = e._L, e.h
    assert e.goal_field_info()["goal"] == -1 and e.goal_field_ptr() is None
    buf = np.zeros(rows * cols, np.int32)
    s = np.zeros(4, np.int32)
    p = np.zeros(4 * 16, np.int32)
    r = np.zeros(4, R.capi.ASTAR_RESULT_DTYPE)
    ESTATE, EINVAL = -5, -1
    assert L.rna_goal_field_download(h, buf.ctypes.data, None, buf.size) == ESTATE
    assert L.rna_goal_field_paths(h, s.ctypes.data, 4, p.ctypes.data, 16, r.ctypes.data) == ESTATE
    assert L.rna_goal_field_paths_device(h, s.ctypes.data, 4, p.ctypes.data, 16, r.ctypes.data) == ESTATE
    for bad in (-1, rows * cols):
        assert L.rna_goal_field_build(h, bad, None) == EINVAL
    assert e.goal_field_info()["goal"] == -1
    goal = int(np.flatnonzero(blocked_of(master))[40])
    info = e.goal_field(goal)
    assert (info["goal"], info["status"], info["reached"], info["tiles_reached"]) == (goal, 2, 0, 0)
    field, nx = e.goal_field_download(want_next=True)
    assert (field == UNREACHED).all() and (nx == 255).all()
    free = np.flatnonzero(blocked_of(master) == 0)[:30].astype(np.int32)
    paths, results = e.goal_field_paths(np.concatenate([free, [goal]]).astype(np.int32), 64)
    assert (results["status"] == 1).all() and (results["path_len"] == 0).all()
    assert L.rna_goal_field_download(h, buf.ctypes.data, None, buf.size - 1) == EINVAL
    assert L.rna_goal_field_download(h, None, None, buf.size) == EINVAL
    assert L.rna_goal_field_paths(h, s.ctypes.data, -1, p.ctypes.data, 16, r.ctypes.data) == EINVAL
    assert L.rna_goal_field_paths(h, s.ctypes.data, 4, p.ctypes.data, 0, r.ctypes.data) == EINVAL
    assert L.rna_goal_field_paths(h, None, 4, p.ctypes.data, 16, r.ctypes.data) == EINVAL
    e.close()


def test_goal_on_a_tile_corner_with_its_in_tile_neighbours_blocked(R):
    """the goal's 0 reaches the neighbouring tiles although no cell of the goal's own tile can improve (found by
    scripts/fuzz_goal_field.py on a 3 x 391 map: the seed has to make the goal tile's ring pending too)"""
    rows, cols = 130, 135
    m = np.zeros((cols, rows), np.float32)
    m[0, 0] = 180.0
    m[64, 65] = m[65, 64] = m[65, 65] = 180.0            # (i, j) = (65, 64), (64, 65), (65, 65)
    master = m.reshape(-1)
    e, g = make_engine_and_geom(R, rows, cols, master)
    blocked, nbr = O.astar_masks(master, rows, cols)
    goal = 64 + 64 * rows
    info = e.goal_field(goal)
    field_ref, res = ref_field(nbr, rows, cols, goal, blocked)
    check_field(e, info, field_ref, res)
    assert info["reached"] == rows * cols - 4
    e.close()
