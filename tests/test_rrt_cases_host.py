"""CPU: the RRT case table of tests/_rrt_cases.py held to its own conditions with the oracle alone -- so that a later edit of
synth or of a case cannot silently turn the GPU tests of tests/test_gpu_rrt.py into easy ones -- and the argument checks of
rna_rrt_batch / rna_rrt_batch_device that need no device."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import _rrt_cases as T
from _build import capi  # noqa: F401  (the fixture)

RNA_EINVAL = -1


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_hard_cases_reach_abort_and_sample(name):
    c = T.conditions(name)
    print(name, tuple(T.case(name).g.start), c)
    assert c["reached"] >= 3, c
    assert c["aborted_1000"] >= 2, c          # out of a budget of at least 1000 samples
    assert c["samples"] >= 2000, c
    assert len(T.case(name).q) <= 16 and T.case(name).q["max_samples"].max() <= 3000


def test_geometry_is_what_the_cases_are_for():
    """start indices off zero where the case says moved; disc bounding boxes of 1-2 cells (D) and 25 (E) a side"""
    assert tuple(T.case("A").g.start) == (0, 0) and tuple(T.case("B").g.start) == (53, 4)
    for n in "CDEH":
        assert T.case(n).g.start[0] != 0 and T.case(n).g.start[1] != 0, n
    pc = T.case("C").g.pos      # (GridMap::move aligns the position to the grid)
    assert abs(pc[0] + 0.52) < 0.05 and abs(pc[1] - 0.4) < 0.05 and np.isnan(T.case("C").master).mean() > 0.03
    assert T.case("E").g.pos[0] > 1500.0 and T.case("D").res > 0.3 and 0.02 <= T.case("E").res < 0.047
    assert round(0.6 / T.case("E").res) + 1 == 25 and 25 * 25 > 3 * 192     # the fourth trip of wave_if_blocked's cell loop
    assert np.array_equal(T.case("H").ref, T.case("B").ref, equal_nan=True)
    assert tuple(T.case("H").q["max_samples"]) == T.H_BUDGETS and set(T.H_SEEDS) <= set(T.case("H").q["seed"].tolist())


def test_starts_are_free_cell_centres():
    for n in T.BUILDERS:
        c = T.case(n)
        for s in c.q["start"]:
            assert not c.blocked(tuple(s)), n
            assert c.centre(*[(a + b) % m for a, b, m in zip(c.map_index(tuple(s)), c.g.start, (c.rows, c.cols))]) == tuple(s), n


def test_lattice_case_sits_in_the_snap_window_and_rescans_the_band():
    c = T.conditions("A")
    print(c)
    assert c["window"] >= 50, c               # hypot < 0.4 decided inside the kernel's 0.1599-0.1601 window
    assert c["band"] >= 100, c                # equal nearest-node distances: rrt_evaluate's band rescan


def test_full_tree_case_fills_the_tree():
    res, _ = T.answers("F")
    assert (res[:, 0] == 0).all() and (res[:, 2] == 2000).all(), res
    assert res[:, 1].max() > 8                # truncation at 8 way points cuts every one of them ...
    assert res[:, 1].min() > 8


def test_truncation_case_has_long_paths():
    assert T.conditions("D")["longest_path"] > 3 * 8


def test_far_target_case_meets_the_9999_rule():
    c = T.conditions("G")
    print(c)
    assert c["far"] >= 100, c                 # samples whose nearest squared distance is >= 9e7
    res, _ = T.answers("G")
    assert set(res[:, 0].tolist()) >= {1, -1}
    q = T.case("G").q
    d = np.hypot(*(q["target"][1] - q["start"][1]))
    assert d == 9999.0                        # tree nodes on both sides of 9999 m from this target
    assert not O.lib().og_position_within_map(O.d2(*q["target"][2]), T.case("G").g.len, T.case("G").g.pos)


@pytest.mark.parametrize("name", sorted(T.BUILDERS))
def test_both_steering_formulations_agree_on_the_counts(name):
    """steer = 0 and steer = 1 give the same status, tree size and sample count: no query of the table meets a last-bit tie"""
    c = T.case(name)
    res, _ = T.answers(name)
    for k in range(len(c.q)):
        r, _ = T.oracle_plan(c.g, c.ref, c.q, k, steer=0)
        assert (r.status, r.path_len, r.tree_size, r.samples) == tuple(res[k]), (name, k)


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "G"])
def test_table_is_deterministic(name):
    """a second build of the case and a second run of the oracle give the same queries and the same answers"""
    c, (res, paths) = T.case(name), T.answers(name)
    c2 = T.BUILDERS[name]()
    assert c2.q.tobytes() == c.q.tobytes() and c2.ref.tobytes() == c.ref.tobytes() and tuple(c2.g.start) == tuple(c.g.start)
    for k in range(len(c2.q)):
        r, p = T.oracle_plan(c2.g, c2.ref, c2.q, k)
        assert (r.status, r.path_len, r.tree_size, r.samples) == tuple(res[k]) and np.array_equal(p, paths[k]), (name, k)


def test_check_rrt_query_accepts_the_oracle_and_refuses_a_changed_bit():
    c, (res, paths) = T.case("B"), T.answers("B")
    rec = np.zeros(len(c.q), [("status", "<i4"), ("path_len", "<i4"), ("tree_size", "<i4"), ("samples", "<i4")])
    for f, col in zip(rec.dtype.names, res.T):
        rec[f] = col
    arr = np.zeros((len(c.q), 64, 2))
    for k, p in enumerate(paths):
        arr[k, :len(p)] = p
    k = int(np.argmax(res[:, 1]))
    assert T.check_rrt_query(rec, arr, c.q, k, c.g, c.ref, tol=float(c.q["close_tolerance"][k])) == 1
    arr[k, 1, 0] = np.nextafter(arr[k, 1, 0], 10.0)
    with pytest.raises(AssertionError):
        T.check_rrt_query(rec, arr, c.q, k, c.g, c.ref, tol=float(c.q["close_tolerance"][k]))


def test_null_engine_and_bad_arguments_are_einval(capi):  # noqa: F811
    L = capi.lib()
    q = np.zeros(1, capi.RRT_QUERY_DTYPE)
    paths = np.zeros((1, 4, 2))
    res = np.zeros(1, capi.RRT_RESULT_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for fn in (L.rna_rrt_batch, L.rna_rrt_batch_device):
        assert fn(None, vp(q), 1, vp(paths), 4, vp(res)) == RNA_EINVAL
        assert fn(None, vp(q), 0, vp(paths), 4, vp(res)) == RNA_EINVAL
        assert fn(None, None, 1, None, 0, None) == RNA_EINVAL
    assert not paths.any() and not res.view(np.int32).any()
