"""The RRT case table (test infrastructure, CPU only: no GPU import): maps off the 0.05 m unmoved happy path on which rrt_kernel /
rrt_evaluate / wave_if_blocked (csrc/planners.hip) are held to oracle/rrt.c -- moved buffers, resolutions from 0.025 m (a disc
of 625 cells, four trips of the cell loop) to 0.5 m (a disc smaller than a cell), the three close tolerances, the 9999 m rule of
findNearNode, full trees, budgets round the speculation round size.  tests/test_gpu_rrt.py runs them on the GPU,
tests/test_rrt_cases_host.py asserts with the oracle alone that they are the hard cases they are meant to be;
check_rrt_query is the comparison every RRT test of the suite makes (tests/test_gpu_parity.py takes it from here).

A case's map is built in buffer order and then moved to each position of `moves` in turn, as GridMap::move takes them (og_move on
the oracle side, Engine.move on the engine's: engine_for);
starts are centres of cells at which og_if_blocked is false on the moved map."""
import ctypes as C
import math

import numpy as np

import _oracle as O
from ros_navigation_amd import synth
from ros_navigation_amd.capi import RRT_QUERY_DTYPE

TOLS = (0.2, 0.05, 0.5)
REPLICA_CAP = 1500          # samples of a query the Python replica of findNearNode follows


class Case:
    """name; lx, ly, res, origin; moves; master (buffer order, before the moves); g, ref (the oracle's geometry and map after
    them); q (RRT_QUERY_DTYPE)"""

    def __init__(self, name, lx, ly, res, origin=(0.0, 0.0), moves=(), nan_share=0.0):
        self.name, self.lx, self.ly, self.res, self.origin, self.moves, self.nan_share = name, lx, ly, res, origin, tuple(moves), nan_share
        self.g = O.make_geom(lx, ly, res, *origin)
        self.rows, self.cols = int(self.g.size[0]), int(self.g.size[1])
        self.master = self.ref = self.q = None

    def set_map(self, master, nan_seed=0):
        master = np.ascontiguousarray(master, np.float32).copy()
        if self.nan_share:
            master[np.random.default_rng(nan_seed).random(master.size) < self.nan_share] = np.nan
        self.master, self.ref = master, master.copy()
        for mv in self.moves:
            O.move(self.g, [self.ref], mv)
        return self

    def centre(self, i, j):
        p = O.d2(0.0, 0.0)
        O.lib().og_position_from_index(C.byref(self.g), O.i2(int(i), int(j)), p)
        return p[0], p[1]

    def map_index(self, p):
        """(i, j) of the cell of position p in MAP order (buffer index less the start index)"""
        b = O.i2(-1, -1)
        assert O.lib().og_index_from_position(C.byref(self.g), O.d2(*p), b)
        return (b[0] - self.g.start[0]) % self.rows, (b[1] - self.g.start[1]) % self.cols

    def blocked(self, p):
        return bool(O.lib().og_if_blocked(C.byref(self.g), O.fptr(self.ref), O.d2(*p)))

    def free_centres(self, n, seed, keep=lambda p: True):
        """n centres of cells (of the moved map) at which og_if_blocked is false, seeded"""
        rng = np.random.default_rng(seed)
        out = []
        while len(out) < n:
            p = self.centre(rng.integers(0, self.rows), rng.integers(0, self.cols))
            if not self.blocked(p) and keep(p):
                out.append(p)
        return out

    def queries(self, starts, targets, tols=TOLS, budget=3000, seed0=1):
        n = len(starts)
        q = np.zeros(n, RRT_QUERY_DTYPE)
        q["start"], q["target"] = np.array(starts), np.array(targets)
        q["close_tolerance"] = [tols[k % len(tols)] for k in range(n)]
        q["seed"] = np.arange(seed0, seed0 + n, dtype=np.uint32)
        q["max_samples"] = budget
        self.q = q
        return self


def _rect_case(name, lx, ly, res, density, mseed, qseed, n=16, tols=TOLS, side=(1, 3), **kw):
    c = Case(name, lx, ly, res, **kw)
    c.set_map(synth.obstacles_rect(c.rows, c.cols, density=density, seed=mseed, side=side), nan_seed=mseed)
    return c.queries(c.free_centres(n, qseed), c.free_centres(n, qseed + 1000), tols)


def case_a():
    """lattice: the stride 0.4 m is exactly two cells of 0.2 m, so hypot < 0.4 falls inside the kernel's 0.1599-0.1601 window and
    equal nearest-node distances are the rule"""
    return _rect_case("A", 4.0, 3.0, 0.2, 0.25, 5, 11)


def case_b():
    """moved once: start index (53, 4)"""
    return _rect_case("B", 6.0, 4.4, 0.1, 0.1, 7, 21, side=(2, 5), moves=[(0.73, -0.41)])


def case_c():
    """moved twice, 5 % NaN cells scattered before the moves, origin off zero"""
    return _rect_case("C", 6.0, 4.0, 0.05, 0.15, 9, 31, side=(3, 10), origin=(1.0, -2.0), moves=[(0.33, 0.21), (-0.52, 0.4)], nan_share=0.05)


def case_d():
    """a disc smaller than a cell: ni, nj of wave_if_blocked are 1 or 2"""
    return _rect_case("D", 12.0, 8.0, 0.5, 0.1, 13, 41, tols=(0.2, 0.5), side=(1, 2), moves=[(1.6, -1.1)])


def case_e():
    """the disc's bounding box is 25 x 25 cells (four trips of the k0 += 192 loop, k / ni by float reciprocal up to k = 624) at
    coordinates of 1500 m.  Two walls with a door each: starts beyond the second wall, targets before the first, and two targets
    in a closed room.  (The strip that enters with the move is 12 cells of NaN: narrower than the disc, so the walls stay shut.)"""
    c = Case("E", 7.5, 5.0, 0.025, origin=(1500.0, -800.0), moves=[(1500.3, -799.7)])
    m = np.zeros((c.cols, c.rows), np.float32)          # m[j, i], before the move
    m[:, 100:104] = 180.0
    m[130:170, 100:104] = 0.0                           # a door of 1.0 m in the first wall
    m[:, 196:200] = 180.0
    m[20:60, 196:200] = 0.0                             # and one at the other end of the second
    m[0:60, 40:44] = 180.0                              # a closed room in the corner
    m[56:60, 0:44] = 180.0
    m[0, :] = m[-1, :] = 180.0
    m[:, 0] = m[:, -1] = 180.0
    c.set_map(m.reshape(-1))
    i_of = lambda p: c.map_index(p)[0]                  # noqa: E731  (the move shifts map indices by 12)
    starts = c.free_centres(12, 51, lambda p: i_of(p) > 225)
    targets = c.free_centres(10, 52, lambda p: 60 < i_of(p) < 105) + c.free_centres(2, 53, lambda p: i_of(p) < 50 and c.map_index(p)[1] < 66)
    return c.queries(starts, targets)


def case_f():
    """full tree: hypot < 0.0 never holds, so the tree fills its 2000 nodes (status 0)"""
    c = Case("F", 6.0, 6.0, 0.1)
    c.set_map(np.zeros(c.rows * c.cols, np.float32))
    return c.queries(c.free_centres(4, 61), c.free_centres(4, 62), tols=(0.0,), budget=100000)


def case_g():
    """the 9999 rule of findNearNode (`shortest` starts at 9999.0: a sample farther than that from every node extends node 0) and
    targets just outside the border"""
    c = Case("G", 6.0, 4.0, 0.1)
    c.set_map(synth.obstacles_rect(c.rows, c.cols, density=0.05, seed=17, side=(2, 5)))
    starts = c.free_centres(6, 71)
    cx, cy = c.g.pos[0], c.g.pos[1]
    targets = [(cx + 20000.0, cy + 3.0), (starts[1][0] + 9999.0, starts[1][1]), (cx - c.lx / 2 - 1.0, cy)] + c.free_centres(3, 72)
    return c.queries(starts, targets, tols=(0.2,))


H_BUDGETS = (-5, 0, 1, 2, 3, 7, 8, 9, 10, 30, 31, 32, 61, 62, 63, 64)
H_SEEDS = (0, 1, 2**31 - 1, 2**31, 2**32 - 1)


def case_h():
    """budgets round the speculation round size RRT_SPEC and the 31- / 62-draw window edges of rng_refill and startmask, seeds
    that are 0 or negative as int32_t, on case B's moved map"""
    c = _rect_case("H", 6.0, 4.4, 0.1, 0.1, 7, 81, side=(2, 5), moves=[(0.73, -0.41)])
    c.q["max_samples"] = H_BUDGETS
    c.q["seed"][:len(H_SEEDS)] = H_SEEDS
    c.q["seed"][8:8 + len(H_SEEDS)] = H_SEEDS       # ... and again with the budgets that make a second round
    return c


BUILDERS = dict(A=case_a, B=case_b, C=case_c, D=case_d, E=case_e, F=case_f, G=case_g, H=case_h)
_cases = {}


def case(name):
    """the case, built once per process and not to be modified"""
    if name not in _cases:
        _cases[name] = BUILDERS[name]()
    return _cases[name]


def engine_for(R, c):
    """an engine with the case's map in all three layers, moved as the oracle's was: start index and master layer equal"""
    e = R.Engine(c.lx, c.ly, c.res, *c.origin)
    assert (e.rows, e.cols) == (c.rows, c.cols)
    for l in range(3):
        e.upload(l, c.master)
    for mv in c.moves:
        e.move(*mv)
    gg = e.geometry()
    assert tuple(gg.start_index) == tuple(c.g.start) and tuple(gg.position) == tuple(c.g.pos)
    dev = e.download(R.capi.LAYER_MASTER)
    assert np.array_equal(np.isnan(dev), np.isnan(c.ref)) and np.array_equal(dev[~np.isnan(dev)], c.ref[~np.isnan(c.ref)])
    return e


# ---- the oracle's answers ----
def oracle_plan(g, ref, q, k, steer=1, cap=2048):
    return O.rrt_plan(g, ref, tuple(q["start"][k]), tuple(q["target"][k]), tol=float(q["close_tolerance"][k]), steer=steer,
                      seed=int(q["seed"][k]), max_samples=int(q["max_samples"][k]), cap=cap)


_answers = {}


def answers(name):
    """oracle/rrt.c (steer = 1) for every query of the case, computed once per process: (results as RRT_RESULT_DTYPE-shaped
    int32 [n, 4] = status, path_len, tree_size, samples; list of way point arrays)"""
    if name not in _answers:
        c = case(name)
        res, paths = [], []
        for k in range(len(c.q)):
            r, p = oracle_plan(c.g, c.ref, c.q, k)
            res.append((r.status, r.path_len, r.tree_size, r.samples))
            paths.append(p)
        _answers[name] = (np.array(res, np.int32), paths)
    return _answers[name]


def check_rrt_query(res, paths, q, k, g, master, tol=0.2):
    """One RRT query of a batch against oracle/rrt.c, BOTH formulations of extendTree's steering step
    (the reference's move_control/src/rrt_planner.cpp:43-51):
      steer = 1  the kernel's own (near + 0.4 (dx, dy) / sqrt(dx^2 + dy^2), IEEE operations only): status, tree size, samples,
                 path length and every way point bit for bit;
      steer = 0  the REFERENCE's (a = atan2(dy, dx); near + 0.4 (cos a, sin a), this libc's libm): the same counts exactly and
                 every way point within 1e-9 m -- the device-side check against the reference's formulation (the one round 5
                 dropped).  A last-bit tie can in principle part the two trees (scripts/fuzz_rrt.py: 4 in 1.9e5 queries, none
                 on any map the tests use), so a test that meets one names it instead of loosening this."""
    args = dict(tol=tol, seed=int(q["seed"][k]), max_samples=int(q["max_samples"][k]))
    ores, opath = O.rrt_plan(g, master, tuple(q["start"][k]), tuple(q["target"][k]), steer=1, **args)
    got = (res["status"][k], res["tree_size"][k], res["samples"][k], res["path_len"][k])
    assert got == (ores.status, ores.tree_size, ores.samples, ores.path_len), (k, "steer=1")
    assert np.array_equal(paths[k, :ores.path_len], opath), (k, "steer=1")
    rres, rpath = O.rrt_plan(g, master, tuple(q["start"][k]), tuple(q["target"][k]), steer=0, **args)
    assert got == (rres.status, rres.tree_size, rres.samples, rres.path_len), (k, "steer=0: the reference's atan2 / cos / sin")
    if rres.path_len:
        assert np.abs(paths[k, :rres.path_len] - rpath).max() < 1e-9, (k, "steer=0 way points")
    return ores.status


# ---- conditions: what makes a case a hard one, from the oracle's results alone ----
_libm = None


def glibc_hypot(x, y):
    """the oracle's hypot (CPython's math.hypot is another algorithm)"""
    global _libm
    if _libm is None:
        _libm = C.CDLL("libm.so.6")
        _libm.hypot.restype = C.c_double
        _libm.hypot.argtypes = [C.c_double, C.c_double]
    return _libm.hypot(x, y)


def replica(c, k, cap=REPLICA_CAP):
    """og_rrt_plan_steer(steer = 1) restated in Python over the oracle's og_rand stream for the first `cap` samples of query k,
    counting what the results do not show: samples whose NEAREST SQUARED distance is >= 9e7 (the kernel then asks hypot < 9999),
    samples whose snap test hypot < 0.4 falls inside the kernel's window 0.1599 <= d^2 <= 0.1601, and samples with a second node
    within the kernel's 2^-46 band of the nearest (the band rescan).  Returns a dict; "complete" says the query ended within the
    cap, and then status / tree_size / samples are the replica's own, to be held against the oracle's."""
    L, g, q = O.lib(), c.g, c.q[k]
    rs = O.RandState()
    L.og_srand(C.byref(rs), int(q["seed"]))
    target, tol = (float(q["target"][0]), float(q["target"][1])), float(q["close_tolerance"])
    inside = bool(L.og_position_within_map(O.d2(*target), g.len, g.pos))
    tree = np.zeros((2000, 2))
    n_tree = samples = far = window = band = 0
    node = (float(q["start"][0]), float(q["start"][1]))
    budget = min(int(q["max_samples"]), cap)
    status = None
    for _ in range(2000):
        tree[n_tree] = node
        n_tree += 1
        if inside:
            fin = glibc_hypot(node[0] - target[0], node[1] - target[1]) < tol
        else:
            fin = ((g.pos[0] + g.len[0] / 2 - node[0]) < tol or (g.pos[1] + g.len[1] / 2 - node[1]) < tol or
                   (node[0] - (g.pos[0] - g.len[0] / 2)) < tol or (node[1] - (g.pos[1] - g.len[1] / 2)) < tol)
        if fin:
            status = 1
            break
        while True:
            if samples >= budget:
                status = -1
                break
            samples += 1
            if L.og_rand(C.byref(rs)) % 10 > 3:
                rnd = c.centre(L.og_rand(C.byref(rs)) % c.rows, L.og_rand(C.byref(rs)) % c.cols)
            else:
                rnd = target
            d = tree[:n_tree] - rnd
            sq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
            m2 = float(sq.min())
            cand = np.nonzero(sq <= m2 + m2 * 2.0 ** -46 + 1.0e-300)[0]
            far += m2 >= 9.0e7
            band += len(cand) > 1
            near, shortest = 0, 9999.0
            for i in cand:          # findNearNode: strict <, so the lowest index among equals; nodes outside the band are farther
                h = glibc_hypot(rnd[0] - tree[i, 0], rnd[1] - tree[i, 1])
                if h < shortest:
                    near, shortest = int(i), h
            npx, npy = float(tree[near, 0]), float(tree[near, 1])
            dd2 = (npx - rnd[0]) ** 2 + (npy - rnd[1]) ** 2
            window += 0.1599 <= dd2 <= 0.1601
            if glibc_hypot(npx - rnd[0], npy - rnd[1]) < 0.4:
                nw = rnd
            else:
                sdx, sdy = rnd[0] - npx, rnd[1] - npy
                sh = math.sqrt(sdx * sdx + sdy * sdy)
                nw = (npx + 0.4 * (sdx / sh), npy + 0.4 * (sdy / sh))
            if not c.blocked(nw):
                node = nw
                break
        if status == -1:
            break
    if status is None:
        status = 0
    complete = not (status == -1 and budget < int(q["max_samples"]))
    return dict(complete=complete, status=status, tree_size=n_tree, samples=samples, far=int(far), window=int(window), band=int(band))


def conditions(name):
    """the figures the conditions of a case are asserted on, from oracle/rrt.c alone (and, for A and G, the replica)"""
    c = case(name)
    res, paths = answers(name)
    out = dict(reached=int((res[:, 0] == 1).sum()), full=int((res[:, 0] == 0).sum()),
               aborted_1000=int(((res[:, 0] == -1) & (c.q["max_samples"] >= 1000)).sum()), samples=int(res[:, 3].sum()),
               longest_path=int(res[:, 1].max()), tree_sizes=res[:, 2].tolist())
    if name in ("A", "G"):
        rep = [replica(c, k) for k in range(len(c.q))]
        for k, r in enumerate(rep):     # the replica is the oracle where it ran to the end
            if r["complete"]:
                assert (r["status"], r["tree_size"], r["samples"]) == (res[k, 0], res[k, 2], res[k, 3]), (name, k, r, res[k])
        out.update(far=sum(r["far"] for r in rep), window=sum(r["window"] for r in rep), band=sum(r["band"] for r in rep),
                   replica_samples=sum(r["samples"] for r in rep))
    return out
