"""vfh_step_kernel against the CPU oracle across the VFH parameters rna_vfh_init accepts (tests/_vfh_cases.py: window diameters
2..64 odd and even, 1..120 sectors, sector angles that do not divide 360, max_speed 50..1000, speed-dependent cut-offs, turn
rates, weights, cell size, robot radius), on inputs that reach the emergency stop and the step after it, narrow and wide
valleys either side of the 10 and 80 degree limits, equal candidate weights, Cant_Turn_To_Goal, the hysteresis band and the
first and last per-speed table (the floors are asserted on the CPU, tests/test_oracle_vfh_params.py, where the oracle is also
pinned to the reference's own vfh.cpp at the same sets).  Bit for bit: chosen speed, turn rate, emergency flag, picked angle,
OriginHist, Hist.  Also the histogram message at 120, 45 and 5 sectors, the robots' state across reset, re-init, partial
batches and a refused init, and the step on the side stream."""

import numpy as np
import pytest

import _oracle as O
import _vfh_cases as V
from _gpu import R, Hip, bits  # noqa: F401
from test_gpu_parity import check_vfh_vs_oracle

pytestmark = pytest.mark.gpu


def poses_of(R, seqs, k):
    """step k of sequences `seqs`, one robot each: (ranges (n, 361, 2), poses)"""
    n = len(seqs)
    ranges = np.zeros((n, 361, 2))
    ranges[:, :, 0] = np.stack([q["ranges"][k] for q in seqs])
    poses = np.zeros(n, R.capi.POSE_DTYPE)
    poses["dt"] = [q["dt"][k] for q in seqs]
    poses["current_speed"] = [q["speed"][k] for q in seqs]
    poses["goal_direction"] = [q["gdir"][k] for q in seqs]
    poses["goal_distance"] = [q["gdist"][k] for q in seqs]
    poses["goal_tolerance"] = [q["gtol"][k] for q in seqs]
    return ranges, poses


def assert_step(got, want, k, where):
    """got: (out, origin, hist) of the engine for some robots; want: the oracle's per-sequence answers (V.run) of the same robots"""
    out, origin, hist = got
    for r, o in enumerate(want):
        at = (where, "robot", r, "step", k)
        assert (out["chosen_speed"][r], out["chosen_turnrate"][r]) == (o["cs"][k], o["ct"][k]), at
        assert bits(origin[r]).tobytes() == bits(o["origin"][k]).tobytes(), at
        assert bits(hist[r]).tobytes() == bits(o["hist"][k]).tobytes(), at
        assert bits(np.float32(out["picked_angle"][r])) == bits(np.float32(o["picked"][k])), at
        assert out["emergency"][r] == int(np.all(o["origin"][k] == 1.0)), at


def run_engine(R, e, seqs, want, where, steps=range(V.STEPS)):
    for k in steps:
        ranges, poses = poses_of(R, seqs, k)
        assert_step(e.vfh_update(ranges, poses), want, k, where)


@pytest.mark.parametrize("name", V.SETS)
def test_vfh_update_matches_oracle_at_set(R, name):
    """every sequence of the set's three families as one robot; then, after a reset, robot 0 alone through a sequence with current
    speeds above max_speed and below zero, which the oracle defines and the reference does not"""
    p = V.params(name)
    seqs = V.sequences(name)
    e = R.Engine(4.0, 4.0, 0.05)
    e.vfh_init(len(seqs), V.capi_params(R, p))
    assert e.hist_size == V.hist_size(p)
    run_engine(R, e, seqs, V.oracle_answers(name), name)
    q = V.clamp_sequence(name)
    e.vfh_reset()
    run_engine(R, e, [q], [V.run(O.OracleVfh, p, q)], name + " clamp")
    e.close()


@pytest.mark.parametrize("name", ["w31", "w64", "sa3", "ms1000", "cut", "turn", "mix"])
def test_vfh_step_through_the_map_at_set(R, name):
    """getRangesFromSubmap + Update_VFH on a map, on an unmoved buffer and on a moved one"""
    p = V.params(name)
    e = R.Engine(12.0, 12.0, 0.05)
    g = O.make_geom(12.0, 12.0, 0.05)
    master = R.synth.obstacles_rect(e.rows, e.cols, density=0.12, seed=7, side=(2, 12))
    e.upload(R.capi.LAYER_MASTER, master)
    poses = R.synth.poses(16, 12.0, 12.0, seed=5, margin=0.3, speed=p.max_speed // 3)
    e.vfh_init(len(poses), V.capi_params(R, p))
    check_vfh_vs_oracle(R, e, g, master, poses.copy(), steps=4, params=p)
    ref = master.copy()
    dx, dy = 0.73, -0.41
    O.move(g, [ref], (dx, dy))
    assert e.move(dx, dy) and tuple(e.geometry().start_index) == tuple(g.start) != (0, 0)
    e.upload(R.capi.LAYER_MASTER, ref)
    poses["x"] += dx
    poses["y"] += dy
    e.vfh_reset()
    check_vfh_vs_oracle(R, e, g, ref, poses, steps=4, params=p)
    e.close()


@pytest.mark.parametrize("name", ["sa3", "sa8", "sa72"])
def test_hist_msg_at_other_sector_counts(R, name):
    p = V.params(name)
    seqs = V.sequences(name)
    e = R.Engine(4.0, 4.0, 0.05)
    e.vfh_init(len(seqs), V.capi_params(R, p))
    assert e.hist_size in (120, 45, 5)
    for k in range(3):
        out, origin, hist = e.vfh_update(*poses_of(R, seqs, k))
    x, y, yb, th = e.vfh_hist_msg(len(seqs))
    assert origin.max() > 65535.0
    for r in range(len(seqs)):
        ox, oy, oyb, oth = O.hist_msg(hist[r], origin[r], p.sector_angle)
        assert np.array_equal(x, ox) and np.array_equal(y[r], oy) and np.array_equal(yb[r], oyb) and th == oth, r
    e.close()


def test_reset_makes_fresh_instances(R):
    """after k steps rna_vfh_reset puts every robot back where fresh oracles start"""
    name = "turn"
    seqs = V.sequences(name)
    e = R.Engine(4.0, 4.0, 0.05)
    e.vfh_init(len(seqs), V.capi_params(R, V.params(name)))
    run_engine(R, e, seqs, V.oracle_answers(name), name, steps=range(7))
    e.vfh_reset()
    run_engine(R, e, seqs, V.oracle_answers(name), name + " after reset", steps=range(7))
    # ... and the sequences in another order: a robot's state is its own
    order = list(range(len(seqs)))[::-1]
    e.vfh_reset()
    run_engine(R, e, [seqs[i] for i in order], [V.oracle_answers(name)[i] for i in order], name + " reversed", steps=range(7))
    e.close()


def test_second_init_with_another_sector_count(R):
    e = R.Engine(4.0, 4.0, 0.05)
    for name in ("sa3", "sa24", "w64", "w2"):     # H 120 -> 15 -> 72, windows 30 -> 64 -> 2: the tables and the state are rebuilt
        seqs = V.sequences(name)
        e.vfh_init(len(seqs), V.capi_params(R, V.params(name)))
        run_engine(R, e, seqs, V.oracle_answers(name), name, steps=range(5))
    e.close()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ["sa360", "sa8", "w2"])
def test_few_robots_keep_their_state_apart(R, name, n):
    """one and three robots at H 1, 45 and 72: the per-robot arrays are 4 to 864 bytes and lie side by side in the state block, so
    an overlap or a swapped offset changes a histogram at the second step; before and after a reset"""
    seqs, want = V.sequences(name)[:n], V.oracle_answers(name)[:n]
    e = R.Engine(4.0, 4.0, 0.05)
    e.vfh_init(n, V.capi_params(R, V.params(name)))
    run_engine(R, e, seqs, want, name, steps=range(6))
    e.vfh_reset()
    run_engine(R, e, seqs, want, name + " after reset", steps=range(6))
    e.close()


def test_partial_batches_leave_the_other_robots_alone(R):
    """stepping the first m robots leaves the others' state untouched: they answer later as oracles that skipped those steps"""
    name = "cut"
    p = V.params(name)
    seqs = V.sequences(name)
    n, m = len(seqs), 5
    e = R.Engine(4.0, 4.0, 0.05)
    e.vfh_init(n, V.capi_params(R, p))
    oracles = [O.OracleVfh(p) for _ in range(n)]
    for k in range(12):
        active = m if k % 3 else n          # every third step all robots, else the first m
        ranges, poses = poses_of(R, seqs, k)
        out, origin, hist = e.vfh_update(ranges[:active], poses[:active])
        for r in range(active):
            cs, ct = oracles[r].update(seqs[r]["ranges"][k], *V.step_args(seqs[r], k))
            at = (r, k)
            assert (out["chosen_speed"][r], out["chosen_turnrate"][r]) == (cs, ct), at
            assert bits(origin[r]).tobytes() == bits(oracles[r].origin_hist()).tobytes(), at
            assert bits(hist[r]).tobytes() == bits(oracles[r].hist()).tobytes(), at
            assert bits(np.float32(out["picked_angle"][r])) == bits(np.float32(oracles[r].picked_angle())), at
    e.close()


REFUSED = [dict(window_diameter=1), dict(window_diameter=65), dict(window_diameter=0), dict(sector_angle=0), dict(sector_angle=2),
           dict(sector_angle=11), dict(sector_angle=100), dict(sector_angle=200), dict(sector_angle=720), dict(sector_angle=-5), dict(sector_angle=144),
           dict(sector_angle=150), dict(sector_angle=179),
           dict(max_speed=0), dict(max_speed=100001)]


def test_refused_init_keeps_the_instances_of_the_last_one(R):
    name = "sa8"
    seqs = V.sequences(name)
    want = V.oracle_answers(name)
    e = R.Engine(4.0, 4.0, 0.05)
    e.vfh_init(len(seqs), V.capi_params(R, V.params(name)))
    k = 0
    for bad in REFUSED:
        run_engine(R, e, seqs, want, name, steps=[k])
        k += 1
        rp = V.capi_params(R, V.params(name))
        for f, v in bad.items():
            setattr(rp, f, v)
        with pytest.raises(R.capi.RnaError):
            e.vfh_init(len(seqs), rp)
    run_engine(R, e, seqs, want, name, steps=range(k, V.STEPS))
    e.close()


def test_step_on_the_side_stream_at_a_non_default_set(R):
    """next to pipelined searches the step runs on the engine's side stream: the device entry point there against the host entry
    point of a twin engine, and both against the oracle"""
    name = "mix"
    p = V.params(name)
    H = V.hist_size(p)
    hip = Hip()
    master = None
    engines = []
    for _ in range(2):
        e = R.Engine(12.0, 12.0, 0.05)
        if master is None:
            master = R.synth.obstacles_rect(e.rows, e.cols, density=0.12, seed=11, side=(2, 12))
        e.upload(R.capi.LAYER_MASTER, master)
        engines.append(e)
    e, twin = engines
    g = O.make_geom(12.0, 12.0, 0.05)
    n = 24
    poses = R.synth.poses(n, 12.0, 12.0, seed=9, margin=0.3, speed=120)
    e.astar_pipeline_depth(4)
    e.vfh_init(n, V.capi_params(R, p))
    twin.vfh_init(n, V.capi_params(R, p))
    oracles = [O.OracleVfh(p) for _ in range(n)]
    d_out, d_origin, d_hist = hip.alloc(n * 16), hip.alloc(n * H * 4), hip.alloc(n * H * 4)
    for s in range(3):
        d_poses = hip.upload(poses)
        e.vfh_step_device(d_poses, n, d_out, d_origin, d_hist)
        e.synchronize()
        out = hip.download(d_out, np.uint8, n * 16).view(R.capi.VFH_OUT_DTYPE)
        origin = hip.download(d_origin, np.float32, n * H).reshape(n, H)
        hist = hip.download(d_hist, np.float32, n * H).reshape(n, H)
        hip.free(d_poses)
        tout, torigin, thist = twin.vfh_step(poses)
        assert out.tobytes() == tout.tobytes(), s
        assert bits(origin).tobytes() == bits(torigin).tobytes() and bits(hist).tobytes() == bits(thist).tobytes(), s
        for r in range(n):
            q = poses[r]
            cs, ct = oracles[r].step_pose(g, master, q["x"], q["y"], q["yaw"], int(q["current_speed"]), q["goal_direction"],
                                          q["goal_distance"], q["goal_tolerance"], float(q["dt"]))
            assert (out["chosen_speed"][r], out["chosen_turnrate"][r]) == (cs, ct), (s, r)
            assert bits(origin[r]).tobytes() == bits(oracles[r].origin_hist()).tobytes(), (s, r)
            assert bits(hist[r]).tobytes() == bits(oracles[r].hist()).tobytes(), (s, r)
        poses["current_speed"] = out["chosen_speed"]
        poses["yaw"] += 0.1
    for d in (d_out, d_origin, d_hist):
        hip.free(d)
    e.close()
    twin.close()
