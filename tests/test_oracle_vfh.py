"""Pins oracle/vfh.c: (a) against committed golden vectors produced by the reference's own
vfh.cpp (tests/golden/gen_vfh_golden.py), (b) on a fixed-seed fuzz and the precomputed tables, live against oracle/_ref
when it is built here and against the reference's recorded answers (tests/golden/gen_vfh_ref_recorded.py) where it is not.
Bit-exact on every output (OriginHist, Hist, picked angle, speed, turnrate)."""
import hashlib
import os

import numpy as np
import pytest

import _oracle as O

GOLD = os.path.join(os.path.dirname(__file__), "golden", "vfh_golden.npz")
RECORDED = os.path.join(os.path.dirname(__file__), "golden", "vfh_ref_recorded.npz")


def params_from_array(a):
    p = O.VfhParams()
    for (name, ctype), v in zip(p._fields_, a):
        setattr(p, name, int(v) if "int" in ctype.__name__ else float(v))
    return p


@pytest.mark.parametrize("pi", [0, 1])
def test_oracle_matches_reference_golden(pi):
    z = np.load(GOLD)
    pre = "p%d_" % pi
    p = params_from_array(z[pre + "params"])
    R = z[pre + "ranges_even"]
    n_seq, n_step = R.shape[:2]
    for s in range(n_seq):
        v = O.OracleVfh(p)
        for k in range(n_step):
            full = np.full(361, 5000.0)
            full[0::2] = R[s, k]
            cs, ct = v.update(full, int(z[pre + "speed"][s, k]), z[pre + "goal_dir"][s, k],
                              z[pre + "goal_dist"][s, k], z[pre + "goal_tol"][s, k], float(z[pre + "dt"][s, k]))
            assert cs == z[pre + "chosen_speed"][s, k] and ct == z[pre + "chosen_turnrate"][s, k], (s, k)
            assert v.hist().tobytes() == z[pre + "hist"][s, k].tobytes(), (s, k)
            assert v.origin_hist().tobytes() == z[pre + "origin_hist"][s, k].tobytes(), (s, k)
            assert np.float32(v.picked_angle()).tobytes() == z[pre + "picked"][s, k].tobytes(), (s, k)


def fuzz_sequences():
    """40 sequences of 15 Update_VFH calls (seed 7): per step the 361 x 2 ranges and (speed, goal direction, goal distance,
    goal tolerance, dt)"""
    rng = np.random.default_rng(7)
    for s in range(40):
        steps = []
        for k in range(15):
            ranges = np.full(361, 5000.0)
            n = rng.integers(0, 60)
            ranges[rng.integers(0, 181, n) * 2] = rng.uniform(150, 3000, n)
            args = (int(rng.integers(0, 200)), np.float32(rng.uniform(0, 360)), np.float32(rng.uniform(100, 4000)),
                    np.float32(250), [0.2, 0.5, 0.125][rng.integers(0, 3)])
            steps.append((ranges, args))
        yield steps


def fuzz_inputs_digest():
    """sha256 of every input of fuzz_sequences(): the recorded answers belong to exactly these inputs"""
    h = hashlib.sha256()
    for steps in fuzz_sequences():
        for ranges, args in steps:
            h.update(ranges.tobytes())
            h.update(repr([float(a) for a in args]).encode())
    return h.hexdigest()


def reference_fuzz_answers():
    """(chosen speed, chosen turnrate, Hist, OriginHist, picked angle) of the reference's VFH per step of fuzz_sequences()"""
    p = O.default_vfh_params()
    out = []
    for steps in fuzz_sequences():
        r = O.RefVfh(p)
        for ranges, args in steps:
            cs, ct = r.update(ranges, *args)
            out.append((cs, ct, r.hist(), r.origin_hist(), np.float32(r.picked_angle())))
    return out


def recorded():
    z = np.load(RECORDED)
    return {k: z[k] for k in z.files}


def test_oracle_matches_reference_live_fuzz():
    """live against oracle/_ref where it is built, else against its recorded answers to the same inputs"""
    if O.ref() is not None:
        answers = reference_fuzz_answers()
    else:
        z = recorded()
        assert str(z["fuzz_inputs_sha256"]) == fuzz_inputs_digest(), "the fuzz inputs are not the ones the answers were recorded for"
        answers = list(zip(z["fuzz_chosen_speed"], z["fuzz_chosen_turnrate"], z["fuzz_hist"], z["fuzz_origin_hist"], z["fuzz_picked"]))
    assert len(answers) == 40 * 15
    p = O.default_vfh_params()
    i = 0
    for steps in fuzz_sequences():
        o = O.OracleVfh(p)
        for ranges, args in steps:
            cs, ct, hist, origin, picked = answers[i]
            i += 1
            assert o.update(ranges, *args) == (cs, ct), i
            assert o.hist().tobytes() == hist.tobytes(), i
            assert o.origin_hist().tobytes() == origin.tobytes(), i
            assert np.float32(o.picked_angle()).tobytes() == np.float32(picked).tobytes(), i


TABLE_IDS = (0, 7, 19)


def reference_tables(p=None):
    """the reference VFH's precomputed tables: cell direction (W x W), sector counts and lists of tables TABLE_IDS
    (lists padded with -1), minimum turning radius per speed, and the number of tables"""
    R = O.ref()
    p = p or O.default_vfh_params()
    r = O.RefVfh(p)
    W = p.window_diameter
    cd = np.array([[R.refvfh_cell_direction(r.h, x, y) for y in range(W)] for x in range(W)], np.float32)
    counts = np.array([[[R.refvfh_cell_sector_count(r.h, t, x, y) for y in range(W)] for x in range(W)] for t in TABLE_IDS], np.int32)
    lists = np.full(counts.shape + (max(1, int(counts.max())),), -1, np.int32)
    for ti, t in enumerate(TABLE_IDS):
        for x in range(W):
            for y in range(W):
                for k in range(counts[ti, x, y]):
                    lists[ti, x, y, k] = R.refvfh_cell_sector(r.h, t, x, y, k)
    radius = np.array([R.refvfh_min_turning_radius(r.h, s) for s in range(p.max_speed + 1)], np.int32)
    return {"num_tables": np.int32(R.refvfh_num_tables(r.h)), "cell_direction": cd, "sector_count": counts,
            "sector_list": lists, "min_turning_radius": radius}


def test_oracle_tables_match_reference():
    """live against oracle/_ref where it is built, else against its recorded tables"""
    ref = reference_tables() if O.ref() is not None else {k[len("tables_"):]: v for k, v in recorded().items() if k.startswith("tables_")}
    check_oracle_tables(O.default_vfh_params(), ref)


def check_oracle_tables(p, ref):
    """the oracle's tables for parameters p against the reference's (reference_tables(p), live or recorded)"""
    L = O.lib()
    o = O.OracleVfh(p)
    W = p.window_diameter
    T = L.og_vfh_num_tables(o.h)
    assert T == int(ref["num_tables"]) == 20
    cd = np.ctypeslib.as_array(L.og_vfh_cell_direction(o.h), (W * W,))
    for x in range(W):
        for y in range(W):
            assert cd[x * W + y] == ref["cell_direction"][x, y] or (x == y == W // 2)
            for ti, t in enumerate(TABLE_IDS):
                n = L.og_vfh_cell_sector_count(o.h, t, x, y)
                assert n == ref["sector_count"][ti, x, y]
                lst = L.og_vfh_cell_sector_list(o.h, t, x, y)
                assert [lst[k] for k in range(n)] == ref["sector_list"][ti, x, y, :n].tolist()
    assert len(ref["min_turning_radius"]) == p.max_speed + 1
    for s in range(p.max_speed + 1):
        assert L.og_vfh_min_turning_radius(o.h, s) == ref["min_turning_radius"][s]


def test_emergency_stop_branch():
    """Obstacle inside the safety radius => histogram all 1, speed 0, spin (vfh.cpp:533-540,1070-1077)."""
    v = O.OracleVfh()
    ranges = np.full(361, 5000.0)
    ranges[180] = 120.0  # straight ahead, closer than robot_radius + safety
    cs, ct = v.update(ranges, 0, np.float32(90), np.float32(2000), np.float32(250), 0.2)
    assert cs == 0 and ct == 40
    assert np.all(v.origin_hist() == 1.0)
