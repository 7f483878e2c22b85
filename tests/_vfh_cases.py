"""VFH+ parameter sets, Update_VFH input sequences and coverage accounting, shared by tests/test_oracle_vfh_params.py (the
oracle against the reference's own vfh.cpp), tests/test_gpu_vfh_params.py (vfh_step_kernel against the oracle),
tests/golden/gen_vfh_params_recorded.py and scripts/fuzz_himm_vfh.py.  Test infrastructure, not a conftest.

SETS names the parameter sets as overrides of default_vfh_params(); each is there for one path of vfh_step_kernel or of
build_tables (ros_navigation_amd/csrc/vfh.hip), named in the comment beside it.

sequences(name) gives, from a fixed seed, three families of Update_VFH sequences of STEPS steps each:
  a  random scans, sparse (0-60 returns) and dense (0-200), 150-3000 mm on the even bins, speeds in [0, max_speed)
  b  goals beside the robot (0, 180, 2, 178, 359 degrees, 300-1500 mm, tolerances 10 / 50 / 250) at every dt branch:
     Cant_Turn_To_Goal becomes true, the speed increment takes both signs
  c  walls with gaps just under and over the 10 and 80 degree limits of Select_Direction in units of the sector angle, two
     equal gaps either side of the goal, goals on the half-sector grid the candidates live on (equal weights; with the goal
     straight behind a wide gap the least weight is shared by two different angles), an all-clear scan, a return inside
     robot_radius + safety distance, and the step after it

coverage(name) counts, from the ORACLE's outputs and the parameters alone, how often the sequences of a set reach each branch;
FLOOR is what every set has to reach of every item that exists for it (exists_for()).

The masked histogram opens a sector only between phi_right and 90 or between 90 and phi_left, with 0 <= phi_right and
phi_left <= 180 (vfh.cpp:1191-1210): every sector behind the robot is blocked, the first blocked sector the walk of
Select_Direction starts from lies in the front half, and no valley starts in a sector above 180 degrees -- for H <= 128 none
in the second ballot word of the kernel beyond sector 64 = 180 / 360 * 128.  No generator tries to make one.
"""
import ctypes as C
import functools
import hashlib

import numpy as np

import _oracle as O

STEPS = 24
FLOOR = 3

SETS = {
    "default": {},
    "sa3": dict(sector_angle=3),                         # H 120: the high ballot word is mostly populated
    "sa4": dict(sector_angle=4),                         # H 90
    "sa8": dict(sector_angle=8),                         # H 45, odd: half = H / 2 truncates
    "sa24": dict(sector_angle=24),                       # H 15
    "sa72": dict(sector_angle=72),                       # H 5
    "sa120": dict(sector_angle=120),                     # H 3: a front mask of one bit
    "sa360": dict(sector_angle=360),                     # H 1: a front mask of no bit
    "sa180": dict(sector_angle=180),                     # H 2: the one count at which a sector behind 90 degrees ends the ring
    "sa7": dict(sector_angle=7),                         # H 51, H SA = 357: accepted although H SA != 360
    "sa16": dict(sector_angle=16),                       # H 22, H SA = 352
    "sa50": dict(sector_angle=50),                       # H 7, H SA = 350
    "w31": dict(window_diameter=31),                     # odd W: the centre row is a front row; NW 17, the looped sector sums
    "w15": dict(window_diameter=15),                     # NW 5
    "w3": dict(window_diameter=3),                       # NW 1
    "w2": dict(window_diameter=2),                       # NW 1, nz[wl < NW ? wl : 0]
    "w64": dict(window_diameter=64),                     # NQ 2112: five trips of the magnitude loop, NW 66
    "w63_sa3_t1": dict(window_diameter=63, sector_angle=3, safety_dist_0ms=50.0, safety_dist_1ms=50.0),   # odd W, H 120, T 1
    "ms1000": dict(max_speed=1000, max_speed_narrow_opening=300, max_speed_wide_opening=600, max_acceleration=500),
    "ms50": dict(max_speed=50, max_speed_narrow_opening=20, max_speed_wide_opening=40),   # caps below current_max_speed
    "cut": dict(free_space_cutoff_0ms=1.5e6, free_space_cutoff_1ms=0.5e6, obs_cutoff_0ms=3e6, obs_cutoff_1ms=1e6),
    "turn": dict(max_turnrate_0ms=90, max_turnrate_1ms=20, min_turnrate=10, min_turn_radius_safety_factor=1.7),
    "wts": dict(weight_desired_dir=2.0, weight_current_dir=7.0),     # ties and order in the candidate minimum
    "cell50": dict(cell_size=50.0, window_diameter=60),
    "rad": dict(robot_radius=400.0, safety_dist_0ms=200.0, safety_dist_1ms=20.0),   # safety distance falling with speed
    "mix": dict(sector_angle=3, window_diameter=41, max_speed=400, safety_dist_0ms=30.0, safety_dist_1ms=120.0,
                max_turnrate_0ms=70, max_turnrate_1ms=25),
}
NAMES = tuple(n for n in SETS if n != "default")


def params(name):
    p = O.default_vfh_params()
    for k, v in SETS[name].items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def capi_params(R, p):
    """the engine's parameter record filled from the oracle's, field by field"""
    rp = R.capi.default_vfh_params()
    for f, _ in rp._fields_:
        setattr(rp, f, getattr(p, f))
    return rp


def hist_size(p):
    return int(np.rint(360.0 / p.sector_angle))


def num_tables(p):
    return 1 if np.float32(p.safety_dist_0ms) == np.float32(p.safety_dist_1ms) else 20


def oracle_bytes(p):
    """what one oracle instance allocates for its sector lists"""
    return num_tables(p) * p.window_diameter ** 2 * hist_size(p) * 4


def counts(name):
    """(sequences of family a, b, c): 26 robots, 13 where an oracle instance is large"""
    return (4, 3, 6) if oracle_bytes(params(name)) > 12e6 else (8, 6, 12)


def safety_dist(p, speed):
    val = int(np.float32(p.safety_dist_0ms) + np.float32(int(speed * (np.float32(p.safety_dist_1ms) - np.float32(p.safety_dist_0ms)) / 1000.0)))
    return max(val, 0)


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _new_seq(family):
    return dict(family=family, ranges=np.full((STEPS, 361), 5000.0), speed=np.zeros(STEPS, np.int32),
                gdir=np.full(STEPS, 90, np.float32), gdist=np.full(STEPS, 2000, np.float32), gtol=np.full(STEPS, 250, np.float32),
                dt=np.full(STEPS, 0.2))


def _speeds(rng, p, n):
    """speeds in [0, max_speed): uniform, with a share at the two ends so that the first and the last of the per-speed tables
    are reached"""
    s = rng.integers(0, p.max_speed, n)
    k = rng.random(n)
    s[k < 0.2] = rng.integers(0, max(1, p.max_speed // 20), int((k < 0.2).sum()))
    s[k > 0.8] = rng.integers(p.max_speed - max(1, p.max_speed // 20), p.max_speed, int((k > 0.8).sum()))
    return s.astype(np.int32)


def _family_a(rng, p, dense):
    q = _new_seq("a")
    for k in range(STEPS):
        n = int(rng.integers(0, 200 if dense else 60))
        q["ranges"][k, rng.integers(0, 181, n) * 2] = rng.uniform(150, 3000, n)
    q["speed"][:] = _speeds(rng, p, STEPS)
    # a robot that slows down: the last chosen speed holds the step's speed up otherwise, and the first table is never read
    q["speed"][STEPS // 2:] = np.minimum(q["speed"][STEPS // 2:], p.max_speed // 25)
    q["gdir"][:] = rng.uniform(0, 360, STEPS)
    q["gdist"][:] = rng.uniform(100, 4000, STEPS)
    q["dt"][:] = rng.choice([0.2, 0.5, 0.125], STEPS)
    return q


def _family_b(rng, p):
    q = _new_seq("b")
    for k in range(STEPS):
        n = int(rng.integers(0, 30))
        q["ranges"][k, rng.integers(0, 181, n) * 2] = rng.uniform(600, 3000, n)
    q["speed"][:] = _speeds(rng, p, STEPS)
    q["gdir"][:] = rng.choice(np.array([0, 180, 2, 178, 359], np.float32), STEPS)
    q["gdist"][:] = rng.uniform(300, 1500, STEPS)
    q["gtol"][:] = rng.choice(np.array([10, 50, 250], np.float32), STEPS)
    q["dt"][:] = rng.choice([0.2, 0, -1, 0.31, 0.3, 0.05], STEPS)
    return q


def _wall(p, dist, gaps):
    """a wall at `dist` on all 361 bins, open (5000) where the bin's direction lies inside one of gaps = [(centre, width)]"""
    deg = np.arange(361) / 2.0
    r = np.full(361, float(dist))
    for c, w in gaps:
        r[np.abs(deg - c) < w / 2.0] = 5000.0
    return r


def _family_c(rng, p, kind):
    q = _new_seq("c")
    SA = p.sector_angle
    reach = p.window_diameter * p.cell_size / 2.0                 # how far the window sees
    r0 = p.robot_radius + max(safety_dist(p, 0), safety_dist(p, p.max_speed))
    dist = min(1000.0, 0.75 * reach)
    dist = max(dist, min(r0 + 1.6 * p.cell_size, reach))          # (a wall inside the safety radius is an emergency stop)
    grow = 2.0 * np.degrees(np.arcsin(min(1.0, r0 / dist)))       # what the robot's radius takes off a gap, both sides
    q["speed"][:] = rng.integers(0, max(1, p.max_speed // 4), STEPS)
    near = 0.6 * p.cell_size                                      # a return in the cell next to the robot
    for k in range(STEPS):
        if kind in (0, 1):       # one gap around the 10 degree (kind 0) or the 80 degree (kind 1) limit, in steps of the sector angle
            c = float(rng.choice([90, 60, 120, 45, 135]))
            w = (10.0, 80.0)[kind] + grow + SA * ((k % 6) - 2) + (0.5 if k % 2 else -0.5)
            q["ranges"][k] = _wall(p, dist, [(c, w)])
            q["gdir"][k] = np.float32(c + SA / 2.0 * ((k // 2) % 5 - 2))
        elif kind == 2:          # two equal gaps either side of the goal; every other step the goal alone, so that the
            g = float(rng.choice([90, 80, 100]))          # last picked direction is the goal's and the weights are equal
            off = 30.0 + SA * (k % 3)
            w = 14.0 + grow + SA * (k % 4)
            if k % 2:
                q["ranges"][k] = _wall(p, dist, [(g - off, w), (g + off, w)])
            q["gdir"][k] = np.float32(g)
        elif kind == 3:          # all clear, a return inside the safety distance, the step after it
            ph = k % 4
            if ph == 1:
                q["ranges"][k, 180] = near
            elif ph == 2:
                q["ranges"][k] = _wall(p, dist, [(float(rng.choice([70, 110])), 40.0 + grow)])
            elif ph == 3:
                q["ranges"][k, int(rng.integers(0, 181)) * 2] = near
            q["gdir"][k] = np.float32(rng.choice([90, 30, 150, 270]))
        elif kind == 5:          # a wide gap and the goal straight behind its middle, on the half-sector grid, after an all-clear
            if k % 2:                                     # step with the same goal (the last picked direction is then the goal):
                q["ranges"][k] = _wall(p, dist, [(90.0, min(max(110.0, 80.0 + 2 * SA) + grow, 160.0))])   # the second and third
            # candidate weigh the same, less than the first.  (a valley's middle is a multiple of half a sector angle)
            q["gdir"][k] = np.float32((np.rint(90.0 / (SA / 2.0)) + (k // 2) % 4 - 2) * (SA / 2.0) + 180.0)
        else:                    # a wide gap with the goal inside it, on the half-sector grid around its middle: the fourth
            c = float(rng.choice([90, 75, 105]))          # candidate applies, and ties with the first
            w = 110.0 + grow + SA * (k % 3)
            q["ranges"][k] = _wall(p, dist, [(c, w)])
            q["gdir"][k] = np.float32(c + SA / 2.0 * (k % 7 - 3))
    return q


@functools.lru_cache(maxsize=None)
def sequences(name):
    """the set's sequences, family a first, then b, then c: a list of dicts of per-step arrays (read-only)"""
    p = params(name)
    na, nb, nc = counts(name)
    rng = np.random.default_rng([2024, sorted(SETS).index(name)])
    out = [_family_a(rng, p, dense=bool(k % 2)) for k in range(na)]
    out += [_family_b(rng, p) for _ in range(nb)]
    out += [_family_c(rng, p, k % 6) for k in range(nc)]
    for q in out:
        for v in q.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def clamp_sequence(name):
    """one more sequence per set in which a quarter of the steps carry a current speed above max_speed (up to three times) or a
    negative one: only the oracle defines these (oracle/vfh.c, build_masked_polar_histogram), the reference does not"""
    p = params(name)
    rng = np.random.default_rng([2025, sorted(SETS).index(name)])
    q = _family_a(rng, p, dense=False)
    s = q["speed"].copy()
    above, below = np.arange(1, STEPS, 8), np.arange(5, STEPS, 8)
    s[above] = rng.integers(p.max_speed + 1, 3 * p.max_speed + 1, len(above))
    s[below] = -rng.integers(1, p.max_speed + 1, len(below))
    s[1] = 3 * p.max_speed
    q["speed"] = s.astype(np.int32)
    q["family"] = "clamp"
    return q


def step_args(q, k):
    return (int(q["speed"][k]), np.float32(q["gdir"][k]), np.float32(q["gdist"][k]), np.float32(q["gtol"][k]), float(q["dt"][k]))


def inputs_digest(name):
    """sha256 of every input of sequences(name) and of the parameters: recorded answers belong to exactly these"""
    h = hashlib.sha256()
    h.update(bytes(params(name)))
    for q in sequences(name):
        for f in ("ranges", "speed", "gdir", "gdist", "gtol", "dt"):
            h.update(np.ascontiguousarray(q[f]).tobytes())
    return h.hexdigest()


def run(cls, p, q):
    """one instance of cls (O.OracleVfh or O.RefVfh) through sequence q -> dict of per-step outputs"""
    v = cls(p)
    H = v.H
    out = dict(cs=np.zeros(STEPS, np.int32), ct=np.zeros(STEPS, np.int32), picked=np.zeros(STEPS, np.float32),
               hist=np.zeros((STEPS, H), np.float32), origin=np.zeros((STEPS, H), np.float32))
    for k in range(STEPS):
        out["cs"][k], out["ct"][k] = v.update(q["ranges"][k], *step_args(q, k))
        out["picked"][k] = v.picked_angle()
        out["hist"][k] = v.hist()
        out["origin"][k] = v.origin_hist()
    return out


def hists_digest(out):
    return hashlib.sha256(out["hist"].tobytes() + out["origin"].tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def oracle_answers(name):
    """the oracle's outputs for sequences(name), computed once and shared (read-only)"""
    p = params(name)
    res = tuple(run(O.OracleVfh, p, q) for q in sequences(name))
    for o in res:
        for v in o.values():
            v.setflags(write=False)
    return res


# ------------------------------------------------------------------------------------------------
# coverage, from the oracle's outputs and the parameters
# ------------------------------------------------------------------------------------------------
def delta_angle(a1, a2):
    """k_delta_angle / VFH::Delta_Angle in float32"""
    d = np.float32(a2) - np.float32(a1)
    if d > 180:
        return np.float32(d - np.float32(360))
    if d < -180:
        return np.float32(d + np.float32(360))
    return np.float32(d)


def valleys(hist, SA):
    """Select_Direction's walk (vfh.cpp:755-800) over a masked histogram: None when the front half is empty, else the list of
    (border 1, border 2) in degrees"""
    H = len(hist)
    start = next((i for i in range(H // 2) if hist[i] == 1), -1)
    if start < 0:
        return None
    out, left, b1 = [], True, 0
    for i in range(start, start + H + 1):
        if hist[i % H] == 0 and left:
            b1, left = (i % H) * SA, False
        if hist[i % H] == 1 and not left:
            b2 = ((i % H) - 1) * SA
            out.append((b1, b2 + 360 if b2 < 0 else b2))
            left = True
    return out


def candidates(vals, p, desired):
    """the candidate angles of vfh.cpp:802-862 in order, and per valley its kind: 'narrow', 'wide', 'wide4' (the fourth
    candidate applies) or None (under 10 degrees)"""
    cand, kinds = [], []
    for b1, b2 in vals:
        a = abs(delta_angle(b1, b2))
        if a < 10:
            kinds.append(None)
        elif a < 80:
            cand.append(np.float32(b1 + (b2 - b1) / 2.0))
            kinds.append("narrow")
        else:
            cand.append(np.float32(b1 + (b2 - b1) / 2.0))
            c2 = np.float32((b1 + 40) % 360)
            c3 = np.float32(b2 - 40)
            if c3 < 0:
                c3 = np.float32(c3 + np.float32(360))
            cand += [c2, c3]
            if delta_angle(desired, c2) < 0 and delta_angle(desired, c3) > 0:
                cand.append(np.float32(desired))
                kinds.append("wide4")
            else:
                kinds.append("wide")
    return cand, kinds


ITEMS = ("emergency", "after_emergency", "empty_front", "narrow", "wide", "wide4", "tie", "tie_min", "cant_turn", "hysteresis",
         "first_table", "last_table", "speed_fell")


@functools.lru_cache(maxsize=None)
def coverage(name):
    p = params(name)
    SA, T = p.sector_angle, num_tables(p)
    U1, U2 = np.float32(p.weight_desired_dir), np.float32(p.weight_current_dir)
    probe = O.OracleVfh(p)
    mtr = np.array([O.lib().og_vfh_min_turning_radius(probe.h, s) for s in range(p.max_speed + 1)])
    bcr = np.array([np.float32(np.float32(mtr[s]) + np.float32(p.robot_radius)) + np.float32(safety_dist(p, s))
                    for s in range(p.max_speed + 1)], np.float32)
    n = dict.fromkeys(ITEMS, 0)
    for q, o in zip(sequences(name), oracle_answers(name)):
        last_speed, last_picked, blocked, was_emergency = 0, np.float32(90), np.float32(0), False
        for k in range(STEPS):
            speed = max(int(q["speed"][k]), 0, last_speed)
            assert speed <= p.max_speed        # the reference reads past Min_Turning_Radius above it
            hist, origin = o["hist"][k], o["origin"][k]
            emergency = bool(np.all(origin == 1.0))
            n["emergency"] += emergency
            n["after_emergency"] += was_emergency and not emergency
            if not emergency:
                blocked = bcr[speed]
                hi = np.float32(np.float32(p.obs_cutoff_0ms) - (speed * (np.float32(p.obs_cutoff_0ms) - np.float32(p.obs_cutoff_1ms)) / 1000.0))
                lo = np.float32(np.float32(p.free_space_cutoff_0ms) - (speed * (np.float32(p.free_space_cutoff_0ms) - np.float32(p.free_space_cutoff_1ms)) / 1000.0))
                n["hysteresis"] += int(np.sum((origin >= lo) & (origin <= hi)))
                if T == 20:
                    idx = min(int(np.floor(np.float32(np.float32(speed) / np.float32(p.max_speed)) * T)), T - 1)
                    n["first_table"] += idx == 0
                    n["last_table"] += idx == T - 1
                vals = valleys(hist, SA)
                if vals is None:
                    n["empty_front"] += 1
                else:
                    cand, kinds = candidates(vals, p, q["gdir"][k])
                    n["narrow"] += kinds.count("narrow")
                    n["wide"] += kinds.count("wide") + kinds.count("wide4")
                    n["wide4"] += kinds.count("wide4")
                    w = [np.float32(U1 * abs(delta_angle(q["gdir"][k], c)) + U2 * abs(delta_angle(last_picked, c))) for c in cand]
                    n["tie"] += len(set(w)) < len(w)
                    # ... and the least weight held by two candidates of different angles: the order decides the picked angle
                    n["tie_min"] += len(w) > 0 and min(w) < 10000000 and len({float(c) for c, x in zip(cand, w) if x == min(w)}) > 1
            # Cant_Turn_To_Goal, vfh.cpp:612-654, in float32 from the blocked circle's radius
            gx = np.float32(float(q["gdist"][k]) * np.cos(float(q["gdir"][k]) * np.pi / 180))
            gy = np.float32(float(q["gdist"][k]) * np.sin(float(q["gdir"][k]) * np.pi / 180))
            hyp = lambda x, y: np.float32(np.sqrt(float(x) * float(x) + float(y) * float(y)))   # noqa: E731
            cant = bool(np.float32(hyp(gx - blocked, gy) + q["gtol"][k]) < blocked or
                        np.float32(hyp(-gx - blocked, gy) + q["gtol"][k]) < blocked)
            n["cant_turn"] += cant
            n["speed_fell"] += 0 < o["cs"][k] < last_speed
            last_speed, last_picked, was_emergency = int(o["cs"][k]), o["picked"][k], emergency
    return n


def exists_for(name):
    """the items of ITEMS a set can reach at all.

    * first_table / last_table: only where there are twenty tables.
    * narrow, wide, wide4, tie, hysteresis need an occupied cell that is not an emergency stop, a cell of the window farther
      from the robot than robot_radius + safety distance: the windows of w2 and w3 (100 and 150 mm) have none, every return
      they see stops the robot, and their histogram is all 0 or, after an emergency, what it was.
    * a valley spans k sectors of the m = 180 / SA + 1 that can open, less the blocked one the walk starts from, and is
      (k - 1) SA wide: with H < 9 (sector angles of 50 and more) a narrow valley exists where SA < 80 and m >= 3 (50, 72), a wide
      one where (m - 2) SA >= 80 (50); the fourth candidate and equal weights are not asked of these sets.
    * speed_fell is reported, not required."""
    p = params(name)
    SA, H = p.sector_angle, hist_size(p)
    it = {"emergency", "after_emergency", "cant_turn", "empty_front"}
    far = p.window_diameter * p.cell_size / 2.0 > p.robot_radius + max(safety_dist(p, 0), safety_dist(p, p.max_speed)) + p.cell_size
    if far:
        it.add("hysteresis")
        if H >= 9:
            it |= {"narrow", "wide", "wide4", "tie", "tie_min"}
        else:
            m = 180 // SA + 1            # sectors that can open; one of them is blocked where the walk starts
            if m >= 3 and SA < 80:
                it.add("narrow")
            if (m - 2) * SA >= 80:
                it.add("wide")
    if num_tables(p) == 20:
        it |= {"first_table", "last_table"}
    return it
