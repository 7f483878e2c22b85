"""CPU: the map-state record of the library (csrc/map_state.hpp: what the next compose or search has to redo, and the epoch)
against the independent statement of the same rule, expected_path() of tests/_mapmodel.py.  tests/cpp/map_state_test.cpp
drives the record alone, no engine and no GPU, through histories read from standard input and prints the epoch after every
operation and, for a compose, which way through rna_compose_master its plan amounts to.

Two sets of histories: the lineage of every engine of the fixed sequences of tests/test_gpu_map_sequences.py (sixteen seeds
and the hand-written ones), and EVERY history of at most four operations over an alphabet that holds each kind of event."""
import itertools
import subprocess

import _build as B
import _mapmodel as M


def lines_of(history):
    """the program's input for one history (lineage()): one line per event, a "search" after every checked step (the GPU test
    reads the masks there).  A "clone" is an event of the child alone: the parent's record is untouched."""
    out = []
    for who, kind, args, checked in history:
        if kind == "update":
            out += ["himm %d" % M.LASER, "compose %d" % args[1]]
        elif kind == "compose":
            out.append("compose %d" % args[0])
        elif kind in ("himm", "upload", "fill"):
            out.append("%s %d" % ("himm" if kind == "himm" else "upload", args[0]))
        elif kind == "move":
            out.append("move %d %d" % (args[0], args[1]))
        elif kind == "radius":
            out.append("radius %r" % float(args[0]))
        elif kind == "cloned":
            out.append("cloned")
        else:
            assert kind in ("clone", "search", "features"), kind
        if checked or kind in ("search", "features"):
            out.append("search")
    return out


def run(histories, shape):
    """[(lines, [(epoch, name)] per line)] of the histories, all in one process"""
    all_lines = [lines_of(h) for h in histories]
    text = "".join("map %d %d\n%s\n\n" % (shape[0], shape[1], "\n".join(lines)) for lines in all_lines)
    out = subprocess.run([B.cpp("map_state_test")], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [(int(l.split(" ")[0]), l.split(" ")[1]) for l in out.stdout.splitlines()]
    got, at = [], 0
    for lines in all_lines:
        got.append((lines, rows[at:at + len(lines)]))
        at += len(lines)
    assert at == len(rows)
    return got


def check(histories, shape):
    disagree = []
    for h, (lines, rows) in zip(histories, run(histories, shape)):
        names = [name for line, (_, name) in zip(lines, rows) if line.startswith("compose")]
        assert all(name == "" for line, (_, name) in zip(lines, rows) if not line.startswith("compose"))
        if names != M.expected_path(h, shape):
            disagree.append((h, names, M.expected_path(h, shape)))
        epoch = 2                                     # the creation steps: an upload and a compose
        for line, (e, _) in zip(lines, rows):
            if line == "search":
                assert e == epoch, (h, line)          # the masks are rebuilt from what is there: nothing changed
            elif line == "cloned":
                assert e == 0, (h, line)              # a new engine's count; the parent's is untouched
            else:
                assert e > epoch, (h, line)           # every other call counts, whether or not it changed anything
            epoch = e
    assert not disagree, "%d histories, the first: %r\n  record: %r\n  expected_path: %r" % ((len(disagree),) + disagree[0])


def fixed_histories():
    out = [(shape, M.generate(shape, seed)) for shape in M.SHAPES for seed in M.SEEDS[shape]]
    out += [(shape, ops) for shape, _, ops in M.HAND_WRITTEN.values()]
    return [(shape, M.lineage(ops, who)) for shape, ops in out for who in range(1 + sum(op[1] == "clone" for op in ops))]


def test_fixed_sequences_every_engine():
    hist = fixed_histories()
    assert len(hist) >= 16 + len(M.HAND_WRITTEN) and len(M.HAND_WRITTEN) == 5
    reached = set()
    for shape in M.SHAPES:
        mine = [h for s, h in hist if s == shape]
        check(mine, shape)
        reached |= {name for h in mine for name in M.expected_path(h, shape)}
    assert reached == set(M.PATHS) | {"pending"}


ALPHABET = [("compose", (0,)), ("compose", (1,)), ("himm", (M.LASER, None)), ("himm", (M.MASTER, None)), ("himm", (M.RANGE, None)),
            ("upload", (M.LASER, 0, 0.0)), ("upload", (M.MASTER, 0, 0.0)), ("move", (0, 0)), ("move", (1, 0)), ("move", (-1, 0)),
            ("radius", (0.3,)), ("radius", (0.0,)), ("search", ())]


def test_every_history_of_at_most_four_operations(shape=M.SHAPES[0]):
    """unchecked steps throughout: the only mask consumer is the "search" of the alphabet; "cloned" may come first.  (One shape:
    the moves of the alphabet are by a cell and back.)"""
    hist = []
    for n in range(5):
        for seq in itertools.product(ALPHABET, repeat=n):
            hist.append([(0, kind, args, False) for kind, args in seq])
            if n < 4:
                hist.append([(0, "cloned", (), False)] + hist[-1])
    assert len(hist) == 33321
    check(hist, shape)
