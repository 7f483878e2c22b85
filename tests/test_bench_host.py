"""CPU-only: the parts of bench.py that need no GPU -- what the result line says about the committed profile files it quotes,
and the work figures it derives from the search kernels' own job counters (rna_astar_job_counters)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_committed_profiles_describe_the_committed_search_kernel():
    """bench.py quotes HBM traffic (PMC passes) and instruction counts (SQ counter pass) from files under profiles/; each carries
    the sha256[:12] of ros_navigation_amd/csrc/astar_tile.hip it was taken at, and the line says `stale` when that is not the
    source in the tree.  The committed ones must not be stale: a kernel change goes with scripts/profile_r06.sh."""
    sha = bench.kernel_source_sha()
    for path in (bench.PMC_SUMMARY, bench.SQ_COUNTERS):
        p = bench.profile_provenance(path)
        assert p["kernel_source_sha"] == sha and p["stale"] is False, p
    d = json.load(open(bench.PMC_SUMMARY))
    assert d["config"]["pipeline"] == bench.DEFAULT_PIPELINE      # the passes were taken at the depth the bench runs by default


def test_work_inflation_from_job_counters():
    args = argparse.Namespace(grid=4096, queries=256, pipeline=bench.DEFAULT_PIPELINE, tiled=False)
    c = dict(searches=1000, tiles_touched=669000, jobs=2709000, jobs_noop=910000, sticky_turns=975000, rows_written=24000000,
             buckets=1300, bucket_reruns=11)
    w = bench.work_inflation(args, 1, 1.0e8, c, passes=1000 // 256 + 1)
    assert abs(w["jobs_per_touched_tile"] - 2709000 / 669000) < 1e-12 and abs(w["noop_job_frac"] - 910 / 2709) < 1e-12
    assert abs(w["sticky_turn_frac"] - 975 / 2709) < 1e-12 and abs(w["rows_written_per_job"] - 24000 / 2709) < 1e-9
    assert w["observed_in"].startswith("the timed region") and w["instructions_provenance"]["stale"] is False
    assert 8.0 < w["instructions_per_settled_cell"] < 10.0      # the committed SQ counter pass: 8.88
    # another configuration: the job figures are still the run's own, the committed instruction counts are not quoted
    w2 = bench.work_inflation(argparse.Namespace(grid=1024, queries=64, pipeline=4, tiled=False), 1, 1.0e6, c, passes=10)
    assert "jobs_per_touched_tile" in w2 and "instructions_per_settled_cell" not in w2
    # an older library without the counters (developer switch RNA_LIB): nothing invented
    assert bench.work_inflation(argparse.Namespace(grid=1024, queries=64, pipeline=4, tiled=False), 1, 1.0e6, None, passes=10) is None


def test_dump_outputs_are_float_arrays_within_64_mb(tmp_path):
    import numpy as np
    import pytest
    arrays = {"a": np.arange(6, dtype=np.float64).reshape(2, 3), "b": np.array([1.5, np.nan], np.float32)}
    info = bench.write_outputs(str(tmp_path / "out"), arrays)
    assert info == {"dir": str(tmp_path / "out"), "files": 2, "bytes": 6 * 8 + 2 * 4}
    for name, a in arrays.items():
        b = np.load(tmp_path / "out" / (name + ".npy"))
        assert b.dtype == a.dtype and np.array_equal(a, b, equal_nan=True)
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "int"), {"i": np.zeros(3, np.int32)})
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "big"), {"f": np.broadcast_to(np.zeros(1), (bench.DUMP_LIMIT_BYTES // 8 + 1,))})


def test_dump_of_the_default_configuration_fits_even_with_every_path_at_its_longest():
    """bench.last_step_outputs on CPU tensors shaped like the default run's buffers (256 queries, 20 passes per step, 32768-cell
    path buffers, a 4096 x 4096 map), every query found with a path as long as the buffer: the dump stays within 64 MB, and
    the samples are the same from call to call."""
    import numpy as np
    import torch
    import ros_navigation_amd as R
    nq, depth, max_path, n = 256, bench.DEFAULT_PIPELINE, 32768, 4096
    args = argparse.Namespace(pipeline=depth, max_path=max_path)
    res = torch.zeros(nq, 6, dtype=torch.int32)
    res[:, 1] = max_path
    paths = torch.arange(nq * max_path, dtype=torch.int32)
    vfh = torch.zeros(nq * R.capi.VFH_OUT_DTYPE.itemsize, dtype=torch.uint8)

    class FakeEngine:
        ncell = n * n

        def download(self, layer):
            return np.full(n * n, float(layer), np.float32)

    def dump():
        return bench.last_step_outputs(FakeEngine(), R, args, nq, 3 * depth, 1, [res.view(-1)], [paths], vfh, False)
    a, b = dump(), dump()
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_LIMIT_BYTES
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert a["astar_status"].shape == (depth, nq) and a["astar_paths_sample_index"].shape == (bench.DUMP_PATHS, 4)
    idx = a["astar_paths_sample_index"].astype(np.int64)
    assert idx[0, 3] == max_path and (idx[:, 2] + idx[:, 3]).max() == a["astar_paths_sample"].size
    p, q = idx[0, :2]
    assert np.array_equal(a["astar_paths_sample"][:max_path], np.arange(q * max_path, (q + 1) * max_path))
    assert a["map_master_sample"].size == bench.DUMP_MAP_CELLS and (a["map_laser_sample"] == R.capi.LAYER_LASER).all()
