"""Pins oracle/vfh.c to the reference's own vfh.cpp at the parameter sets of tests/_vfh_cases.py -- window diameters 2..64 odd
and even, 1..120 sectors, sector angles that do not divide 360, max_speed 50..1000, speed-dependent cut-offs, turn rates,
weights, cell size, robot radius -- on the three input families of that module, and asserts that those inputs reach the
branches they are there for (the coverage floors).  Live against oracle/_ref where it is built, else against the reference's
recorded answers to the same inputs (tests/golden/gen_vfh_params_recorded.py).  Bit-exact on chosen speed, turn rate, Hist,
OriginHist and the picked angle.  The current speed stays at or below max_speed here: above it the reference reads past
Min_Turning_Radius (oracle/vfh.c, build_masked_polar_histogram); the centre cell of an odd window, for which the reference
reads in front of the scan, sees "no return" (tests/_oracle.py, ranges_array)."""
import os

import numpy as np
import pytest

import _oracle as O
import _vfh_cases as V
import test_oracle_vfh as T

RECORDED = os.path.join(os.path.dirname(__file__), "golden", "vfh_params_recorded.npz")
TABLE_SETS = ("w31", "sa3", "ms1000")


@pytest.fixture(scope="module")
def recorded():
    z = np.load(RECORDED)
    return {k: z[k] for k in z.files}


def reference_answers(name):
    """per sequence of the set: the reference's chosen speeds, turn rates, picked angles and the sha256 of its histograms"""
    p = V.params(name)
    outs = [V.run(O.RefVfh, p, q) for q in V.sequences(name)]
    return {"cs": np.stack([o["cs"] for o in outs]), "ct": np.stack([o["ct"] for o in outs]),
            "picked": np.stack([o["picked"] for o in outs]), "hists_sha256": np.array([V.hists_digest(o) for o in outs])}


@pytest.mark.parametrize("name", V.SETS)
def test_oracle_matches_reference_at_set(name, recorded):
    if O.ref() is not None:
        ref = reference_answers(name)
    else:
        assert str(recorded[name + "_inputs_sha256"]) == V.inputs_digest(name), "not the inputs the answers were recorded for"
        ref = {k: recorded[name + "_" + k] for k in ("cs", "ct", "picked", "hists_sha256")}
    got = V.oracle_answers(name)
    assert len(got) == len(ref["cs"]) == sum(V.counts(name))
    for s, o in enumerate(got):
        for k in range(V.STEPS):
            assert (o["cs"][k], o["ct"][k]) == (ref["cs"][s, k], ref["ct"][s, k]), (s, k)
            assert np.float32(o["picked"][k]).tobytes() == np.float32(ref["picked"][s, k]).tobytes(), (s, k)
        assert V.hists_digest(o) == str(ref["hists_sha256"][s]), s


@pytest.mark.parametrize("name", V.SETS)
def test_inputs_reach_the_branches_they_are_there_for(name):
    cov, need = V.coverage(name), V.exists_for(name)
    print(name, cov)
    p = V.params(name)
    if V.hist_size(p) >= 9 and p.window_diameter >= 15:
        assert need >= set(V.ITEMS) - {"speed_fell", "first_table", "last_table"}    # every item is asked of an ordinary set
    short = {k: cov[k] for k in need if cov[k] < V.FLOOR}
    assert not short, (name, short)
    q = V.clamp_sequence(name)       # (the GPU test's extra sequence: a quarter of its speeds outside [0, max_speed])
    assert (q["speed"] > p.max_speed).sum() == 3 and q["speed"].max() == 3 * p.max_speed and (q["speed"] < 0).sum() == 3


def test_falling_speeds_of_the_goal_family():
    """family b makes the chosen speed fall while it stays positive (Cant_Turn_To_Goal with a speed to lose)"""
    for name in ("default", "turn", "ms1000"):
        assert V.coverage(name)["speed_fell"] >= V.FLOOR, name


@pytest.mark.parametrize("name", TABLE_SETS)
def test_oracle_tables_match_reference_at_set(name, recorded):
    p = V.params(name)
    if O.ref() is not None:
        ref = T.reference_tables(p)
    else:
        pre = name + "_tables_"
        ref = {k[len(pre):]: v for k, v in recorded.items() if k.startswith(pre)}
    T.check_oracle_tables(p, ref)
