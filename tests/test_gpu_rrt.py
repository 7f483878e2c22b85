"""GPU: rrt_kernel (csrc/planners.hip) on the case table of tests/_rrt_cases.py -- moved buffers, resolutions 0.025-0.5 m, the three
close tolerances, full trees, the 9999 m rule, budgets round the speculation round size -- against oracle/rrt.c: bit for bit in
the kernel's formulation of the steering step, counts and 1e-9 m in the reference's (check_rrt_query).  And what the two entry
points promise about the caller's buffers (include/rna.h): nothing is written behind min(path_len, max_path_len) way points,
nothing at all for a query that ran out of its budget, path_len is the full length when the path is cut, and the device form
answers byte for byte as the host form does.

tests/test_rrt_cases_host.py holds the table to the conditions that make these the hard cases, with the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import _rrt_cases as T
from _gpu import R, SENTINEL, dev  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu

ROOM = 64                    # way points a row holds where nothing is to be cut: longer than any path of the table
RNA_OK, RNA_EINVAL = 0, -1   # include/rna.h


@pytest.fixture(scope="module")
def engines(R):  # noqa: F811
    """case name -> engine, made on first use (engine_for asserts start index and master layer against the oracle's)"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = T.engine_for(R, T.case(name))
        return made[name]
    yield get
    for e in made.values():
        e.close()


def sentinel_paths(n, max_path_len):
    return np.full(n * max_path_len * 2 * 8, SENTINEL, np.uint8).view(np.float64).reshape(n, max_path_len, 2)


def expected(R, name, max_path_len, order=None):  # noqa: F811
    """the oracle's answer in the shape of the call's outputs: results, and a sentinel-filled paths array with the first
    min(path_len, max_path_len) way points of every query that did not abort"""
    ores, opaths = T.answers(name)
    order = range(len(ores)) if order is None else order
    res = np.zeros(len(order), R.capi.RRT_RESULT_DTYPE)
    paths = sentinel_paths(len(order), max_path_len)
    for row, k in enumerate(order):
        res[row] = tuple(ores[k])
        w = min(int(ores[k, 1]), max_path_len)
        paths[row, :w] = opaths[k][:w]
    return res, paths


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("name", sorted(T.BUILDERS))
def test_case_matches_oracle(R, engines, name):  # noqa: F811
    c, e = T.case(name), engines(name)
    res, paths = e.rrt(c.q)
    for k in range(len(c.q)):
        T.check_rrt_query(res, paths, c.q, k, c.g, c.ref, tol=float(c.q["close_tolerance"][k]))
    assert np.array_equal(res, expected(R, name, ROOM)[0])
    if name == "F":
        assert (res["status"] == 0).all() and (res["tree_size"] == 2000).all()


@pytest.mark.parametrize("name", sorted(T.BUILDERS))
def test_host_form_leaves_the_rest_of_the_callers_buffer(R, engines, name):  # noqa: F811
    """behind a row's way points, and in the whole row of an aborted query, the caller's array is as it was"""
    c, e = T.case(name), engines(name)
    want_res, want_paths = expected(R, name, ROOM)
    assert want_res["path_len"].max() < ROOM
    res, paths = e.rrt(c.q, ROOM, paths=sentinel_paths(len(c.q), ROOM))
    assert np.array_equal(res, want_res)
    for k in range(len(c.q)):
        w = int(want_res["path_len"][k])
        assert same_bytes(paths[k, :w], want_paths[k, :w]), (k, "way points")
        assert (paths[k, w:].view(np.uint8) == SENTINEL).all(), (k, int(want_res["status"][k]), "written behind the path")
    assert same_bytes(paths, want_paths)


@pytest.mark.parametrize("max_path_len", [1, 3, 8])
@pytest.mark.parametrize("name", ["D", "F"])
def test_truncated_paths(R, engines, name, max_path_len):  # noqa: F811
    """max_path_len below the path: path_len still the full length, the first max_path_len way points (goal side first), every
    other result field as in the untruncated run, nothing written elsewhere -- the next row's head included"""
    c, e = T.case(name), engines(name)
    want_res, want_paths = expected(R, name, max_path_len)
    assert (want_res["path_len"] > max_path_len).sum() >= 4        # the guard of the back-trace decides something
    res, paths = e.rrt(c.q, max_path_len, paths=sentinel_paths(len(c.q), max_path_len))
    assert np.array_equal(res, want_res)
    assert same_bytes(paths, want_paths)
    reached = np.nonzero(want_res["status"] == 1)[0]
    for k in reached[:1]:        # goal -> start: the first way point is the node that finished the plan
        assert np.hypot(*(paths[k, 0] - c.q["target"][k])) < c.q["close_tolerance"][k]


def device_form(R, e, q, max_path_len):  # noqa: F811
    """rna_rrt_batch_device on torch tensors, both outputs sentinel-filled and 64 bytes longer than the call may write"""
    import torch
    n = len(q)
    d_q = dev(q)
    d_paths = torch.full((n * max_path_len * 16 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_res = torch.full((n * 16 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e.rrt_device(d_q.data_ptr(), n, d_paths.data_ptr(), max_path_len, d_res.data_ptr())
    e.synchronize()
    paths, res = d_paths.cpu().numpy(), d_res.cpu().numpy()
    assert (paths[-64:] == SENTINEL).all() and (res[-64:] == SENTINEL).all()
    return res[:-64].view(R.capi.RRT_RESULT_DTYPE), paths[:-64].view(np.float64).reshape(n, max_path_len, 2)


@pytest.mark.parametrize("name", ["B", "H"])
def test_device_form_answers_as_the_host_form(R, engines, name):  # noqa: F811
    c, e = T.case(name), engines(name)
    host_res, host_paths = e.rrt(c.q, ROOM, paths=sentinel_paths(len(c.q), ROOM))
    want_res, want_paths = expected(R, name, ROOM)
    res, paths = device_form(R, e, c.q, ROOM)
    assert same_bytes(res, host_res) and same_bytes(res, want_res)
    assert same_bytes(paths, host_paths) and same_bytes(paths, want_paths)     # unwritten elements still the sentinel
    # again on the same engine in reverse order: the answers follow the queries, the engine keeps nothing
    order = list(range(len(c.q)))[::-1]
    res, paths = device_form(R, e, c.q[order], ROOM)
    want_res, want_paths = expected(R, name, ROOM, order)
    assert same_bytes(res, want_res) and same_bytes(paths, want_paths)
    res, paths = device_form(R, e, c.q, 3)                                     # and cut short
    want_res, want_paths = expected(R, name, 3)
    assert same_bytes(res, want_res) and same_bytes(paths, want_paths)


def test_batch_shape_does_not_change_an_answer(R, engines):  # noqa: F811
    """one query alone, and B's and H's queries in one call (they share a map): every query answers as in its own batch"""
    b, h, e = T.case("B"), T.case("H"), engines("B")
    bres, bpaths = expected(R, "B", ROOM)
    hres, hpaths = expected(R, "H", ROOM)
    for k in (0, int(np.argmax(bres["path_len"])), int(np.nonzero(bres["status"] == -1)[0][0])):
        res, paths = e.rrt(b.q[k:k + 1], ROOM, paths=sentinel_paths(1, ROOM))
        assert same_bytes(res, bres[k:k + 1]) and same_bytes(paths, bpaths[k:k + 1]), k
    both = np.concatenate([b.q, h.q])
    res, paths = e.rrt(both, ROOM, paths=sentinel_paths(len(both), ROOM))
    assert same_bytes(res, np.concatenate([bres, hres])) and same_bytes(paths, np.concatenate([bpaths, hpaths]))


def test_arguments(R, engines):  # noqa: F811
    """max_path_len <= 0 and null pointers with n > 0 are RNA_EINVAL and write nothing; n = 0 is a no-op"""
    import torch
    e, q = engines("B"), T.case("B").q[:2]
    L = R.capi.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    paths = sentinel_paths(2, 4)
    res = np.full(2 * 16, SENTINEL, np.uint8)
    d_q = dev(q)
    d_paths = torch.full((2 * 4 * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_res = torch.full((2 * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    host = (L.rna_rrt_batch, vp(q), vp(paths), vp(res))
    device = (L.rna_rrt_batch_device, d_q.data_ptr(), d_paths.data_ptr(), d_res.data_ptr())
    for fn, pq, pp, pr in (host, device):
        for bad in (0, -1, -2048):
            assert fn(e.h, pq, 2, pp, bad, pr) == RNA_EINVAL, bad
        assert fn(e.h, None, 2, pp, 4, pr) == RNA_EINVAL
        assert fn(e.h, pq, 2, None, 4, pr) == RNA_EINVAL
        assert fn(e.h, pq, 2, pp, 4, None) == RNA_EINVAL
        assert fn(e.h, pq, -1, pp, 4, pr) == RNA_EINVAL
        assert fn(e.h, pq, 0, pp, 4, pr) == RNA_OK
        assert fn(e.h, None, 0, None, 4, None) == RNA_OK
    e.synchronize()
    assert (paths.view(np.uint8) == SENTINEL).all() and (res == SENTINEL).all()
    assert (d_paths.cpu().numpy() == SENTINEL).all() and (d_res.cpu().numpy() == SENTINEL).all()
    r2, p2 = e.rrt(T.case("B").q, ROOM, paths=sentinel_paths(16, ROOM))        # the engine is as usable as before
    assert same_bytes(r2, expected(R, "B", ROOM)[0]) and same_bytes(p2, expected(R, "B", ROOM)[1])
