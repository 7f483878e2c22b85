"""GPU tests against the REFERENCE directly: the kernels behind rna_himm_update, rna_get_submap / rna_get_submap_device
and rna_move, fed the adversarial cases of tests/test_oracle_refpin.py (maps of 40 x 26 ... 31 x 47 cells, no side a
multiple of the rasteriser's tiles, unmoved and moved), compared bit for bit with the reference's own grid_map_core and
MapUpdater::lineOnMap in oracle/_ref/libref_gridmap.so -- not with the oracle.

RRT stays a transitive check: the kernel equals og_rrt_plan_steer(steer=1) bit for bit (test_gpu_parity.py),
steer=0 equals RrtPlanner::makePlan through test_oracle_refpin.py::test_rrt_steer0_matches_make_plan, and the gap
between 0 and 1 is measured in test_oracle_misc.py::test_rrt_steering_formulations_part_only_in_the_last_bits."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import test_oracle_refpin as T
from _gpu import R, same_f32  # noqa: F401  (R: the fixture)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(O.ref_gridmap() is None,
                                 reason="oracle/_ref/libref_gridmap.so is not built (make -C oracle ref where the "
                                        "reference sources are present)")]


def engines(R):
    """(geometry index, engine) for every geometry of T.geometries(): each base map, then moved by T.MOVES in turn"""
    gi = 0
    for lx, ly, res, pos in T.BASES:
        e = R.Engine(lx, ly, res, *pos)
        for k in range(len(T.MOVES) + 1):
            if k:
                a, b = T.MOVES[k - 1]
                g0 = e.geometry()
                d = (a * g0.length[0], b * g0.length[1]) if k == len(T.MOVES) else (a * res, b * res)
                e.move(g0.position[0] + d[0], g0.position[1] + d[1])
            g, want = e.geometry(), T.geometries()[gi]
            assert tuple(g.size) == tuple(want.size) and tuple(g.start_index) == tuple(want.start)
            assert tuple(g.position) == tuple(want.pos) and tuple(g.length) == tuple(want.len)
            yield gi, e
            gi += 1
        e.close()


def test_himm_update_matches_line_on_map(R):
    """rna_himm_update on unmoved and moved maps against the reference's lineOnMap, ray by ray, on the whole layer"""
    himm = {gi: (layer, rays) for gi, layer, rays in T.cases()["himm"]}
    n_rays = 0
    for gi, e in engines(R):
        layer, rays = himm[gi]
        want = layer.copy()
        O.ref_himm_update(T.geometries()[gi], want, rays)
        e.upload(R.capi.LAYER_LASER, layer)
        e.himm_update(R.capi.LAYER_LASER, rays)
        assert same_f32(e.download(R.capi.LAYER_LASER), want), gi
        n_rays += len(rays)
    assert n_rays > 1000


def test_get_submap_matches_the_reference(R):
    """rna_get_submap (host copy) and rna_get_submap_device against GridMap::getSubmap: success, geometry, top-left
    buffer index and every cell"""
    import torch
    wins = {gi: (layer, w) for gi, layer, w in T.cases()["window"]}
    checked = failed = 0
    for gi, e in engines(R):
        g = T.geometries()[gi]
        layer, ws = wins[gi]
        e.upload(R.capi.LAYER_LASER, layer)
        t = torch.empty(g.size[0] * g.size[1], dtype=torch.float32, device="cuda")
        for c, ln in ws:
            ok, sub, data = O.get_submap(g, layer, c, ln, reference=True)
            got = e.get_submap(R.capi.LAYER_LASER, c[0], c[1], ln[0], ln[1])
            assert (got is not None) == ok, (gi, c, ln)
            if not ok:
                failed += 1
                continue
            info, host = got
            inf = O.SubmapInfo()
            assert O.ref_gridmap().refgm_submap_information(C.byref(g), O.d2(*c), O.d2(*ln), C.byref(inf)) == 1
            assert tuple(info.size) == tuple(sub.size) and tuple(info.top_left) == tuple(inf.top_left), (gi, c, ln)
            assert tuple(info.position) == tuple(sub.pos) and tuple(info.length) == tuple(sub.len), (gi, c, ln)
            assert same_f32(host, data), (gi, c, ln)
            t.fill_(-7.0)
            torch.cuda.synchronize()   # the fill runs on torch's stream, the copy on the engine's (include/rna.h)
            dinfo = R.capi.SubmapInfo()
            rc = R.capi.lib().rna_get_submap_device(e.h, R.capi.LAYER_LASER, c[0], c[1], ln[0], ln[1], t.data_ptr(),
                                                    t.numel(), C.byref(dinfo))
            e.synchronize()
            assert rc == 1 and tuple(dinfo.size) == tuple(sub.size)
            assert same_f32(t[:len(data)].cpu().numpy(), data), (gi, c, ln)
            checked += 1
    assert checked > 200 and failed > 10


def test_submap_far_edge_regression_case(R):
    """the window centred on the map's far edge that the oracle once refused (tests/golden/submap_far_edge_case.npz)"""
    z = np.load(T.REGRESSION)
    e = R.Engine(*z["geometry"], *z["position"])
    e.upload(R.capi.LAYER_LASER, z["layer"])
    got = e.get_submap(R.capi.LAYER_LASER, *z["center"], *z["length"])
    assert got is not None
    info, data = got
    assert np.array(list(info.length) + list(info.position), np.float64).tobytes() == z["ref_geom"][:4].tobytes()
    assert tuple(info.size) == tuple(z["ref_geom"][5:7].astype(int)) and data.tobytes() == z["ref_data"].tobytes()
    e.close()


def test_move_matches_the_reference_whole_layers(R):
    """rna_move against GridMap::move on all three layers: moved flag, start index, position and every cell, the NaN
    it resets included"""
    for bi, layer in T.cases()["move"]:
        lx, ly, res, pos = T.BASES[bi]
        e = R.Engine(lx, ly, res, *pos)
        g = O.make_geom(lx, ly, res, *pos)
        ref = [layer.copy(), layer[::-1].copy(), np.roll(layer, 7)]
        for l in range(3):
            e.upload(l, ref[l])
        for k, (sx, sy) in enumerate(T.MOVES + [(-0.5, 0.0), (0.0, 0.0)]):
            d = (sx * g.len[0], sy * g.len[1]) if k == len(T.MOVES) - 1 else (sx * res, sy * res)
            target = (g.pos[0] + d[0], g.pos[1] + d[1])
            _, moved = O.move(g, ref, target, reference=True)
            assert e.move(*target) == bool(moved), (bi, k)
            gg = e.geometry()
            assert tuple(gg.start_index) == tuple(g.start) and tuple(gg.position) == tuple(g.pos), (bi, k)
            for l in range(3):
                assert same_f32(e.download(l), ref[l]), (bi, k, l)
        e.close()
