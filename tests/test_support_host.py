"""CPU-only checks of the helpers the other tests stand on (tests/_gpu.py, tests/_build.py): the change between buffer order
and map order is the kernels' own index formula, map_nbr takes neighbours in map space, same_f32 is bitwise up to NaN
payloads, and the kernel resources come from the Makefile's own compile line, once per session."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _build
import _oracle as O
from _gpu import bits, map_nbr, same_f32, to_buffer, to_map

ROWS, COLS = 5, 3
STARTS = [(2, 1), (0, 0), (4, 2)]


@pytest.mark.parametrize("s0,s1", STARTS)
def test_to_map_is_the_kernels_buffer_index_and_to_buffer_its_inverse(s0, s1):
    a = np.arange(ROWS * COLS, dtype=np.int32)
    m = to_map(a, ROWS, COLS, s0, s1)
    assert m.shape == (COLS, ROWS)
    for j in range(COLS):
        for i in range(ROWS):
            assert m[j, i] == a[((j + s1) % COLS) * ROWS + (i + s0) % ROWS], (i, j)
    back = to_buffer(m, ROWS, COLS, s0, s1)
    assert back.shape == a.shape and np.array_equal(back, a)


def nbr_mask(blocked):
    """og_astar_nbr_mask of a [j, i] array that is in map order already"""
    b = np.ascontiguousarray(blocked.reshape(-1).astype(np.uint8))
    nbr = np.zeros(b.size, np.uint8)
    u8 = C.POINTER(C.c_uint8)
    O.lib().og_astar_nbr_mask(b.ctypes.data_as(u8), ROWS, COLS, nbr.ctypes.data_as(u8))
    return nbr.reshape(COLS, ROWS)


@pytest.mark.parametrize("s0,s1", STARTS)
def test_map_nbr_takes_the_neighbours_in_map_space(s0, s1):
    g = O.make_geom(ROWS * 0.05, COLS * 0.05, 0.05)
    assert (g.size[0], g.size[1]) == (ROWS, COLS)
    g.start[0], g.start[1] = s0, s1
    in_map = np.zeros((COLS, ROWS), np.uint8)
    in_map[1, 0] = 1                                   # on the map's edge i = 0: for (2, 1) that is buffer column 2, inside the buffer
    want_map = nbr_mask(in_map)
    blocked = np.zeros(ROWS * COLS, np.uint8)
    for j in range(COLS):                              # rotated into the buffer by hand, cell by cell
        for i in range(ROWS):
            blocked[((j + s1) % COLS) * ROWS + (i + s0) % ROWS] = in_map[j, i]
    got = map_nbr(g, blocked)
    assert got.shape == (ROWS * COLS,) and got.dtype == np.uint8
    for j in range(COLS):
        for i in range(ROWS):
            assert got[((j + s1) % COLS) * ROWS + (i + s0) % ROWS] == want_map[j, i], (i, j)
    # the cell across the wrap: map (ROWS - 1, 1) is the blocked cell's neighbour in the BUFFER of a moved map, not in the map --
    # its mask is that of a cell with no blocked cell near it (the same cell of an empty map)
    assert want_map[1, ROWS - 1] == nbr_mask(np.zeros((COLS, ROWS), np.uint8))[1, ROWS - 1]
    assert got[((1 + s1) % COLS) * ROWS + (ROWS - 1 + s0) % ROWS] == want_map[1, ROWS - 1]
    assert want_map[1, 1] != nbr_mask(np.zeros((COLS, ROWS), np.uint8))[1, 1]     # while the neighbour inside the map sees it


def test_same_f32_is_bitwise_up_to_nan_payloads():
    nans = np.array([0x7fc00000, 0x7fc00001, 0xffc00000, 0x7f800001], np.uint32).view(np.float32)
    assert np.isnan(nans).all() and len(set(bits(nans).tolist())) == 4
    assert same_f32(nans, nans[::-1].copy())
    assert same_f32(np.array([1.5, np.nan, -0.0], np.float32), np.array([1.5, nans[3], -0.0], np.float32))
    assert not same_f32(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    assert not same_f32(np.array([np.nan], np.float32), np.array([1.0], np.float32))
    assert not same_f32(np.array([1.0, np.nan], np.float32), np.array([np.nan, 1.0], np.float32))


@_build.needs_hipcc
def test_resources_come_from_the_makefiles_compile_line_once(monkeypatch):
    res = _build.resources("frontier.hip")
    want = {"fr_classify_kernel", "fr_seam_kernel", "fr_flatten_kernel", "fr_init_kernel", "fr_stats_kernel", "fr_compact_kernel"}
    assert len(res) == len(want) and all(any(w in k for k in res) for w in want), list(res)
    for k, v in res.items():
        assert set(v) == {"VGPRs", "AGPRs", "LDS", "ScratchSize"}, (k, v)
    cmd = _build.commands["frontier.hip"]
    assert all(flag in cmd for flag in "-ffp-contract=off --offload-arch=gfx950".split()), cmd     # the product's flags
    assert "-amdgpu-atomic-optimizer-strategy=None" not in cmd

    def no_compiler(*a, **k):
        raise AssertionError("a cached source was compiled again: %r" % (a,))
    monkeypatch.setattr(subprocess, "run", no_compiler)
    assert _build.resources("frontier.hip") is res


@_build.needs_hipcc
def test_the_search_kernels_resources_are_compiled_with_its_per_file_flags():
    assert _build.resources("astar_tile.hip")
    assert "-amdgpu-atomic-optimizer-strategy=None" in _build.commands["astar_tile.hip"]
