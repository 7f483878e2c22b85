"""CPU: what the fixed operation sequences of tests/test_gpu_map_sequences.py are worth, from the model alone (tests/_mapmodel.py,
no engine).  The GPU test is only as good as the histories it walks: these conditions fail when a change of the generator or of
the seeds leaves a way through rna_compose_master unvisited, a map that never changes, searches that find nothing, or stale
flags that are never tried.  Run with -s for the counts.

(Blocked sets of a robot radius are counted here with the fixed stencil of MapModel.stencil_blocked, not with the reference's
cell-by-cell predicate: they decide how many queries have a path and whether an operation changed the set, never an expected
value.)"""
import numpy as np
import pytest

import _mapmodel as M

CASES = [(shape, seed) for shape in M.SHAPES for seed in M.SEEDS[shape]]


@pytest.fixture(scope="module")
def surveys():
    out = {}
    for shape, seed in CASES:
        ops = M.generate(shape, seed)
        out[shape, seed] = (ops, M.survey(shape, seed, ops))
    return out


def total(surveys, key, sub=None):
    return sum(s[key][sub] if sub else s[key] for _, s in surveys.values())


def test_sixteen_sequences_of_fourteen_operations(surveys):
    assert len(CASES) == 16 and all(len(M.SEEDS[shape]) == 8 for shape in M.SHAPES)
    for (shape, seed), (ops, _) in surveys.items():
        assert sum(op[1] != "features" for op in ops) == M.N_OPS and sum(op[1] == "features" for op in ops) == 1
        assert ops == M.generate(shape, seed)                                   # the same draw every time
        scope = {}
        exec(M.replay_literal(shape, seed, ops), scope)                         # what a failure prints replays the sequence
        assert scope["REPLAY"] == (shape, seed, ops)
        radii = {op[2][0] for op in ops if op[1] == "radius"}
        assert radii <= set(M.RADII)


def test_compose_paths_moves_radius_changes_and_clones(surveys):
    paths = {k: total(surveys, "paths", k) for k in M.PATHS + ("pending",)}
    moves = {k: total(surveys, "moves", k) for k in M.MOVE_KINDS}
    after, clones = total(surveys, "radius_after_incremental"), total(surveys, "clones")
    print("\ncomposes by expected path:", paths, "\nmoves:", moves, "\nradius changes right after an incremental refresh:", after,
          "\nclones:", clones)
    assert all(paths[k] >= 3 for k in M.PATHS), paths
    assert all(moves[k] >= 2 for k in M.MOVE_KINDS), moves
    assert after >= 3 and clones >= 2
    same_twice = sum(1 for ops, _ in surveys.values() for a, b in zip(ops, ops[1:])
                     if a[1] == b[1] == "radius" and a[0] == b[0] and a[2] == b[2])
    layers = {(op[1], op[2][0]) for ops, _ in surveys.values() for op in ops if op[1] in ("himm", "upload", "fill")}
    print("the same radius set twice in a row:", same_twice, "\nlayers written:", sorted(layers))
    assert same_twice >= 1 and total(surveys, "zero_moves") >= 1          # (rna_move to the current position)
    assert {("himm", layer) for layer in (0, 1, 2)} <= layers and {("upload", layer) for layer in (0, 1, 2)} <= layers
    assert {layer for kind, layer in layers if kind == "fill"} == {0, 1, 2}
    unchecked = sum(not op[3] for ops, _ in surveys.values() for op in ops)
    assert paths["pending"] >= 3 and unchecked >= 16          # histories in which the masks wait across several operations


def test_most_composes_change_the_master(surveys):
    n, changing = total(surveys, "composes"), total(surveys, "composes_changing")
    print("\ncomposes:", n, "of which change a cell of the master:", changing)
    assert changing >= 0.6 * n


@pytest.mark.parametrize("shape,seed", CASES)
def test_searches_find_paths_and_stale_flags_are_tried(surveys, shape, seed):
    _, s = surveys[shape, seed]
    print("\n%dx%d seed %d: %d queries, %d with a path, %d longer than 30 cells; with snapshots whose flags read 0, %d operations each "
          "change the state the flags answer for, %d change nothing" % (shape[0], shape[1], seed, s["queries"], s["found"], s["long"], s["stale_changed"],
                                              s["stale_unchanged"]))
    assert s["queries"] >= 8 * 16
    assert 2 * s["found"] >= s["queries"] and 4 * s["long"] >= s["queries"]
    # (the GPU test rebuilds the snapshots after every checked step, so each of these operations starts from flags that read 0:
    # one change followed by operations that change nothing counts once)
    assert s["stale_changed"] >= 3 and s["stale_unchanged"] >= 1


def test_every_kind_of_change_is_tried_from_flags_that_read_zero(surveys):
    """the kinds of operation that, with snapshots built and all three flags 0, change what the flags answer for: the fixed
    seeds and sequence (e) together try each kind the stale flags had no test after"""
    kinds = set()
    runs = [(shape, seed, ops) for (shape, seed), (ops, _) in surveys.items()] + [M.HAND_WRITTEN["e"]]
    for shape, seed, ops in runs:
        m, built, fresh = M.MapModel(shape[0], shape[1], seed), None, False
        for who, kind, args, checked in ops:
            if who != 0:
                continue
            m.apply(kind, args)
            if not checked:
                fresh = False
                continue
            key = m.state_key(m.stencil_blocked())
            if kind != "features" and built is not None and fresh and key != built:
                kinds.add((kind, args[0]) if kind in ("himm", "upload", "fill") else (kind,))
            if kind == "features" or built is not None:
                built, fresh = key, True
    print("\nkinds of change tried from flags 0 0 0:", sorted(kinds))
    assert {("move",), ("radius",), ("update",), ("compose",), ("upload", M.MASTER), ("fill", M.MASTER), ("himm", M.MASTER)} <= kinds
    shape, seed, ops = M.HAND_WRITTEN["e"]
    s = M.survey(shape, seed, ops)
    assert (s["stale_changed"], s["stale_unchanged"], s["zero_moves"]) == (8, 2, 1)


def test_expected_path_on_the_hand_written_sequences():
    want = {"a": ["footprint", "footprint", "fused", "fused", "footprint"], "b": ["pending", "moved", "fused", "fused"],
            "c": ["whole", "fused", "whole"]}
    for name, (shape, seed, ops) in M.HAND_WRITTEN.items():
        if name not in want:
            continue
        assert M.expected_path(M.lineage(ops, 0), shape) == want[name], name
    # a clone's first compose is a whole-layer copy whatever the original had done, and the original's is not
    ops = [(0, "update", ((1, 200, None), 0), True), (0, "clone", (), True), (1, "compose", (0,), True), (0, "compose", (0,), True)]
    assert M.expected_path(M.lineage(ops, 1), (140, 96)) == ["pending", "whole"]
    assert M.expected_path(M.lineage(ops, 0), (140, 96)) == ["pending", "fused"]


def test_model_operations():
    m = M.MapModel(140, 96, 5)
    assert np.array_equal(m.layers[M.MASTER], m.layers[M.LASER], equal_nan=True) and np.isnan(m.layers[M.RANGE]).all()
    m.apply("himm", (M.LASER, (7, 300, None)))
    assert not np.array_equal(m.layers[M.MASTER], m.layers[M.LASER], equal_nan=True)
    c = m.clone()
    m.apply("compose", (0,))
    assert np.array_equal(m.layers[M.MASTER], m.layers[M.LASER], equal_nan=True)
    assert not np.array_equal(c.layers[M.MASTER], c.layers[M.LASER], equal_nan=True)       # the clone went its own way
    m.apply("move", (70, -3))
    assert m.moved() and not c.moved()
    home = M._move(np.random.default_rng(0), m, "home")
    m.apply("move", home)
    assert not m.moved()
    m.apply("move", (150, 0))
    assert all(np.isnan(a).all() for a in m.layers)
    m.apply("fill", (M.MASTER, 0.0))
    m.apply("radius", (0.125,))
    assert m.r == 0.125 and (m.layers[M.MASTER] == 0).all() and m.stencil_blocked().sum() == 0
    # the stencil against the reference's predicate where no tie can arise: 2 1/2 cells
    import test_gpu_footprint as F
    assert np.array_equal(c.stencil_blocked(), c.point_blocked())
    c.apply("radius", (0.125,))
    assert np.array_equal(c.stencil_blocked(), F.ref_blocked(c.g, c.master, 0.125))
    # a box of rays stays in its box: tile (0, 0) of the unmoved map
    before = c.layers[M.LASER].copy()
    c.apply("himm", (M.LASER, (3, 300, M._T)))
    diff = ~((before == c.layers[M.LASER]) | (np.isnan(before) & np.isnan(c.layers[M.LASER])))
    jj, ii = np.nonzero(diff.reshape(96, 140))
    assert diff.any() and ii.max() < 64 and jj.max() < 64
