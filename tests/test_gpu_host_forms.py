"""GPU: what the host-pointer forms of the C ABI promise apart from their results (csrc/engine.hpp, Staging): a refused
allocation of a call's device temporaries is RNA_ENOMEM and leaves the engine as it was, and the outputs documented as
"0 behind the end" are written by the call, not inherited from the caller's buffer.

The entry points are called through ctypes directly: the Engine wrappers hand in zeroed buffers of the right size, which
hides both."""
import ctypes as C

import numpy as np
import pytest

from _gpu import R, make_engine  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu

ROWS = COLS = 64
MAX_LEN = 160            # longer than any path of the map below
FILL = 0x7f7f7f7f
RNA_OK, RNA_ENOMEM = 0, -2   # include/rna.h


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def case(R):  # noqa: F811
    """a 64 x 64 map, two walls with a door each, the field of a goal in the far corner; four starts whose paths have
    different lengths, one blocked start (status 1, no path), and the wrapper's answer for them"""
    m = np.zeros((COLS, ROWS), np.float32)
    m[20, 0:50] = 180.0
    m[44, 14:64] = 180.0
    e = make_engine(R, ROWS, COLS, m.reshape(-1))
    e.goal_field(60 + 60 * ROWS)
    starts = np.array([2 + 2 * ROWS, 40 + 30 * ROWS, 58 + 50 * ROWS, 5 + 20 * ROWS, 10 + 10 * ROWS], np.int32)
    paths, res = e.goal_field_paths(starts, MAX_LEN)
    assert res["status"].tolist() == [0, 0, 0, 1, 0] and len(set(res["path_len"].tolist())) == 5
    assert res["path_len"].max() < MAX_LEN
    yield e, starts, paths, res
    e.close()


def test_refused_allocation_is_enomem_and_leaves_the_engine_usable(R, case):  # noqa: F811
    e, starts, paths, res = case
    # 2^20 starts x 2^24 cells x 4 B = 64 TiB of path buffer: hipMalloc refuses it before anything is enqueued, so
    # the output arrays are never written and need not have that size
    n, max_len = 1 << 20, 1 << 24
    many = np.resize(starts[[0, 1, 2, 4]], n).astype(np.int32)
    out_paths = np.zeros(16, np.int32)
    out_res = np.zeros(n, R.capi.ASTAR_RESULT_DTYPE)
    L = R.capi.lib()
    rc = L.rna_goal_field_paths(e.h, ptr(many), n, ptr(out_paths), max_len, ptr(out_res))
    msg = L.rna_last_error(e.h)
    print("refused allocation: rc", rc, "last error", msg)
    assert rc == RNA_ENOMEM, (rc, msg)
    assert msg
    assert not out_paths.any() and not out_res.view(np.int32).any()
    # the refusal is not what the next calls' launch checks report
    paths2, res2 = e.goal_field_paths(starts[[0, 1, 2, 4]], MAX_LEN)
    assert np.array_equal(paths2, paths[[0, 1, 2, 4]]) and np.array_equal(res2, res[[0, 1, 2, 4]])
    assert e.astar_blocked_mask().sum() == 50 + 50


def test_goal_field_paths_zero_behind_the_path(R, case):  # noqa: F811
    e, starts, paths, res = case
    got = np.full((len(starts), MAX_LEN), FILL, np.int32)
    got_res = np.zeros(len(starts), R.capi.ASTAR_RESULT_DTYPE)
    assert R.capi.lib().rna_goal_field_paths(e.h, ptr(starts), len(starts), ptr(got), MAX_LEN, ptr(got_res)) == RNA_OK
    assert np.array_equal(got_res, res)
    for k, ln in enumerate(res["path_len"]):
        assert np.array_equal(got[k, :ln], paths[k, :ln]), k
        assert not got[k, ln:].any(), k
    assert res["path_len"][3] == 0   # the blocked start's row is zero throughout


def test_shortcut_paths_zero_behind_the_way_points(R, case):  # noqa: F811
    e, starts, paths, res = case
    want_wp, want_out = e.shortcut_paths(paths, res)
    assert want_out["status"].tolist() == [0, 0, 0, 1, 0] and 2 <= want_out["n_waypoints"][0] < MAX_LEN
    got = np.full((len(starts), MAX_LEN), FILL, np.int32)
    got_out = np.zeros(len(starts), R.capi.SHORTCUT_RESULT_DTYPE)
    rc = R.capi.lib().rna_shortcut_paths(e.h, ptr(paths), ptr(res), len(starts), MAX_LEN, 0, 0, ptr(got), MAX_LEN, ptr(got_out))
    assert rc == RNA_OK
    assert np.array_equal(got_out, want_out)
    for k, nw in enumerate(want_out["n_waypoints"]):
        assert np.array_equal(got[k, :nw], want_wp[k, :nw]), k
        assert not got[k, nw:].any(), k
