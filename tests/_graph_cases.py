"""Waypoint graphs and queries for the graph A* (graph_astar_kernel, og_graph_astar), shared by tests/test_graph_astar_host.py
(the oracle against a plain Dijkstra and numpy), tests/test_gpu_graph_astar.py (the kernel against the oracle and against
Dijkstra) and scripts/fuzz_graph.py.  Test infrastructure, not a conftest.

A case is a dict of name, family, exact, V (float64, nv x 2), E (int32, ne x 2), W (float32 per edge, or None) and st (float64,
n x 4: start x, y, target x, y); the arrays are read-only.  random_cases(family) draws them from a fixed seed:

  vertices on the 0.5 m lattice in [0, 12)^2 (duplicate vertices, routes of equal cost, ties of the closest-vertex search), query
  coordinates on the same lattice in [-1, 13]; nv from NV, ne uniform in [0, 3 nv] with end points drawn freely (self loops,
  parallel edges, several components); query counts from NQ, so that a batch ends before, at and after a workgroup of 64.

  euclid  W = ceil(8 len) / 8 + k / 8, k uniform in 0..23: a multiple of 1/8 that is >= the edge's Euclidean length.  The
          heuristic is admissible (in float32 as well: len = sqrt(m) / 2 with m an integer <= 1152 is either a multiple of 1/8,
          and then sqrtf is exact, or at least 1 / 272 below the next one, far more than half an ulp), and every sum of weights is
          exact in float32 and in float64 (multiples of 1/8 below 2^21).  A* must return a route of Dijkstra's cost: exact = True.
  free    W from FREE_WEIGHTS, unrelated to the geometry: the heuristic is inconsistent, d[] is lowered through the undirected
          branch of relax() and black vertices come back onto the heap.
  zero    W = None, add_edge without a property: every weight 0, f == h.

hand_cases() adds the hand-written ones (see there).  `exact` marks every case whose weights are >= the Euclidean length and
sum exactly, whatever its family: those are the cases the Dijkstra checks run on.

dijkstra() is the independent reference: float64, heapq, written from the textbook and sharing nothing with oracle/astar.c or the
kernel.  closest_vertex() is the float64 numpy statement of AStarPlanner::findClosedVertex."""
import ctypes as C
import functools
import heapq

import numpy as np

import _oracle as O

NV = (1, 2, 9, 64, 65, 200, 256)
NQ = (1, 63, 64, 65, 200)
FAMILIES = ("euclid", "free", "zero")
FREE_WEIGHTS = np.array([1, 2, 0.5, 3.25, 0, 0.125, 7], np.float32)
FLT_MAX = np.float32(3.4028234663852886e+38)
PER_NV = 2                              # random cases per vertex count and family


def euclid_weights(rng, V, E):
    ln = np.hypot(V[E[:, 0], 0] - V[E[:, 1], 0], V[E[:, 0], 1] - V[E[:, 1], 1])
    return (np.ceil(ln * 8) / 8 + rng.integers(0, 24, len(E)) / 8).astype(np.float32)


def lattice_queries(rng, n):
    return np.round(rng.uniform(-1, 13, (n, 4)) * 2) / 2


def random_graph(rng, nv, family):
    """V, E, W of one random graph of the family (scripts/fuzz_graph.py draws from this as well)"""
    V = rng.integers(0, 24, (nv, 2)).astype(np.float64) * 0.5
    ne = int(rng.integers(0, 3 * nv + 1))
    E = rng.integers(0, nv, (ne, 2)).astype(np.int32)
    if family == "euclid":
        W = euclid_weights(rng, V, E)
    elif family == "free":
        W = rng.choice(FREE_WEIGHTS, ne).astype(np.float32)
    else:
        W = None
    return V, E, W


def _case(name, family, exact, V, E, W, st):
    c = dict(name=name, family=family, exact=bool(exact), V=np.ascontiguousarray(V, np.float64).reshape(-1, 2),
             E=np.ascontiguousarray(E, np.int32).reshape(-1, 2), W=None if W is None else np.ascontiguousarray(W, np.float32).reshape(-1),
             st=np.ascontiguousarray(st, np.float64).reshape(-1, 4))
    assert c["W"] is None or len(c["W"]) == len(c["E"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def random_cases(family):
    rng = np.random.default_rng([2031, FAMILIES.index(family)])
    out = []
    for k in range(PER_NV * len(NV)):
        nv = NV[k % len(NV)]
        nq = NQ[k % len(NQ)]            # 7 and 5 are coprime: over fourteen cases every count comes up with several sizes
        V, E, W = random_graph(rng, nv, family)
        out.append(_case("%s-%d-nv%d-nq%d" % (family, k, nv, nq), family, family == "euclid", V, E, W, lattice_queries(rng, nq)))
    return tuple(out)


def reference_graph():
    loc = (C.c_double * 18)()
    euv = (C.c_int * 20)()
    O.lib().og_reference_graph(loc, euv)
    return np.array(loc).reshape(9, 2), np.array(euv, np.int32).reshape(10, 2)


LINE_NV = 256


@functools.lru_cache(maxsize=None)
def hand_cases():
    rng = np.random.default_rng(2032)
    out = []
    # the reference's own nine vertices (8 m x 5 m cells), its ten edges weighted with their lengths plus k / 8
    V, E = reference_graph()
    st = np.round(rng.uniform(-2, 24, (48, 4)) * 2) / 2
    st[:, 1::2] = np.round(rng.uniform(-2, 12, (48, 2)) * 2) / 2
    out.append(_case("reference-weighted", "hand", True, V, E, euclid_weights(rng, V, E), st))
    # two components: a square 0-1-2-3 and a triangle 4-5-6, no edge between them
    V = np.array([[0, 0], [2, 0], [2, 2], [0, 2], [8, 8], [10, 8], [9, 10]], np.float64)
    E = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [4, 5], [5, 6], [6, 4]], np.int32)
    out.append(_case("two-components", "hand", True, V, E, euclid_weights(rng, V, E), lattice_queries(rng, 40)))
    # parallel edges of different weight, the dearer one first in one pair and last in the other; the detour 0-2-1 costs 4
    V = np.array([[0, 0], [2, 0], [1, 1], [4, 0]], np.float64)
    E = np.array([[0, 1], [0, 1], [0, 2], [2, 1], [1, 3], [1, 3], [3, 1]], np.int32)
    W = np.array([5, 2.5, 2, 2, 2, 6, 2.125], np.float32)
    out.append(_case("parallel-edges", "hand", True, V, E, W, np.round(rng.uniform(-1, 5, (24, 4)) * 2) / 2))
    # one edge of weight FLT_MAX: closed_plus keeps d at "infinity" across it.  0-1 is that edge and 0-2-1 a way round it;
    # 3 hangs on 1 by a second FLT_MAX edge alone: a white vertex is queued whether or not its distance fell, so 3 comes off the
    # heap with d = FLT_MAX and the route is the goal by itself (not exact: in float64 FLT_MAX is a length like any other)
    V = np.array([[0, 0], [4, 0], [2, 2], [8, 0]], np.float64)
    E = np.array([[0, 1], [0, 2], [2, 1], [1, 3]], np.int32)
    W = np.array([FLT_MAX, 3, 3, FLT_MAX], np.float32)
    out.append(_case("flt-max-edge", "hand", False, V, E, W, np.round(rng.uniform(-1, 9, (24, 4)) * 2) / 2))
    # every vertex farther than 999 m from some queries: closedDistance = 999 is never beaten and vertex 0 is the answer,
    # although vertex 2 is the nearest; other queries lie within 999 m of some vertices only
    V = np.array([[1500, 40], [1500.5, 40], [1400, 0], [1450, 0.5], [1500, 40]], np.float64)
    E = np.array([[0, 1], [1, 2], [2, 3], [3, 4], [0, 3]], np.int32)
    st = np.array([[0, 0, 1, 1], [0, 0, 1450, 0], [1400, 0, -3, 2.5], [401.5, 0, 0, 0], [401, 0, 0, 0], [460, 0, 502, 40],
                   [400, 0, 1500, 40], [2600, 40, 0, 0], [2450, 0.5, 1500.5, 41], [0, -950, 1400, 2000]], np.float64)
    W = np.array([0.5, 109, 50.5, 64, 66], np.float32)      # lengths 0.5, 108.2, 50.0, 63.7, 63.7
    out.append(_case("beyond-999m", "hand", True, V, E, W, st))
    # no edge at all: a route only from a vertex to itself
    V = np.array([[1, 1], [3, 1], [1, 1], [5, 5], [0, 4]], np.float64)
    out.append(_case("no-edges", "hand", True, V, np.zeros((0, 2), np.int32), None, lattice_queries(rng, 24)))
    # 256 vertices in a line, half a metre apart: the longest route there is, 256 vertices and 258 positions
    V = np.stack([np.arange(LINE_NV) * 0.5, np.zeros(LINE_NV)], axis=1)
    E = np.stack([np.arange(LINE_NV - 1), np.arange(1, LINE_NV)], axis=1).astype(np.int32)
    st = np.array([[-1, 0, 200, 0.5], [200, 0, -1, 0], [0, 0, 127.5, 0], [127.5, 1, 0, 1], [60.25, 0, 60.25, 0], [3, 0, 100, -2]], np.float64)
    out.append(_case("line-256", "hand", True, V, E, np.full(LINE_NV - 1, 0.5, np.float32), st))
    # a 4-connected 12 x 12 grid, one metre apart, its edges in random order: many vertices at one distance from the goal and
    # many routes of one cost, so the order in which the heap hands out equal keys decides the route.  Once without weights
    # (f == h) and once with every weight the edge's length (f == the route's length on every shortest route)
    ij = np.array([(i, j) for j in range(12) for i in range(12)])
    E = np.array([(a, a + 1) for a in range(144) if a % 12 != 11] + [(a, a + 12) for a in range(132)], np.int32)
    E = E[rng.permutation(len(E))]
    out.append(_case("grid-zero", "hand", False, ij.astype(np.float64), E, None, lattice_queries(rng, 64)))
    out.append(_case("grid-unit", "hand", True, ij.astype(np.float64), E, np.ones(len(E), np.float32), lattice_queries(rng, 64)))
    return tuple(out)


def all_cases():
    return sum((random_cases(f) for f in FAMILIES), ()) + hand_cases()


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


def names(kind=None):
    """case names for pytest.mark.parametrize: of one family, 'hand', or all"""
    if kind == "hand":
        return ["reference-weighted", "two-components", "parallel-edges", "flt-max-edge", "beyond-999m", "no-edges", "line-256",
                "grid-zero", "grid-unit"]
    fams = FAMILIES if kind is None else (kind,)
    out = ["%s-%d-nv%d-nq%d" % (f, k, NV[k % len(NV)], NQ[k % len(NQ)]) for f in fams for k in range(PER_NV * len(NV))]
    return out + (names("hand") if kind is None else [])


# ------------------------------------------------------------------------------------------------
# the oracle's answers, assembled as AStarPlanner::makePlan does: start, vertex locations, target
# ------------------------------------------------------------------------------------------------
def oracle_route(L, V, E, W, s, t):
    """og_graph_astar from vertex s to vertex t -> list of vertex indices (empty: no route)"""
    nv, ne = len(V), len(E)
    verts = (C.c_int * (nv + 2))()
    n = L.og_graph_astar(nv, V.ctypes.data_as(C.POINTER(C.c_double)), ne, E.ctypes.data_as(C.POINTER(C.c_int)) if ne else None,
                         W.ctypes.data_as(C.POINTER(C.c_float)) if W is not None else None, s, t, verts, nv + 2)
    return [verts[i] for i in range(n)]


def oracle_closest(L, V, x, y):
    return L.og_graph_closest_vertex(len(V), V.ctypes.data_as(C.POINTER(C.c_double)), O.d2(x, y))


def oracle_plan(V, E, W, st):
    """per query (start vertex, goal vertex, route as vertex indices, path as an array of positions [len, 2])"""
    L = O.lib()
    out = []
    for q in st:
        s, t = oracle_closest(L, V, q[0], q[1]), oracle_closest(L, V, q[2], q[3])
        r = oracle_route(L, V, E, W, s, t)
        path = np.vstack([q[:2]] + [V[v] for v in r] + [q[2:]]) if r else np.zeros((0, 2))
        out.append((s, t, tuple(r), path))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_answers(name):
    """oracle_plan of a case, computed once and shared (read-only)"""
    c = by_name(name)
    res = oracle_plan(c["V"], c["E"], c["W"], c["st"])
    for r in res:
        r[3].setflags(write=False)
    return res


# ------------------------------------------------------------------------------------------------
# the independent references
# ------------------------------------------------------------------------------------------------
def edge_costs(E, W):
    """{(u, v): cheapest weight of an edge between u and v}, both directions, float64"""
    best = {}
    for k, (u, v) in enumerate(E.tolist()):
        w = float(W[k]) if W is not None else 0.0
        for a, b in ((u, v), (v, u)):
            if w < best.get((a, b), np.inf):
                best[(a, b)] = w
    return best


def dijkstra(nv, E, W, s):
    """distance from s to every vertex (float64, inf = not connected), undirected, non-negative weights"""
    adj = [[] for _ in range(nv)]
    for k, (u, v) in enumerate(E.tolist()):
        w = float(W[k]) if W is not None else 0.0
        adj[u].append((v, w))
        adj[v].append((u, w))
    dist = [np.inf] * nv
    dist[s] = 0.0
    heap = [(0.0, s)]
    while heap:
        d, u = heapq.heappop(heap)
        if d > dist[u]:
            continue
        for v, w in adj[u]:
            if d + w < dist[v]:
                dist[v] = d + w
                heapq.heappush(heap, (d + w, v))
    return dist


def closest_vertex(V, x, y):
    """AStarPlanner::findClosedVertex in float64 numpy: the nearest vertex closer than 999 m, the lowest index among equals;
    vertex 0 when there is none (the value oracle and kernel give the reference's uninitialised result)"""
    d = np.hypot(x - V[:, 0], y - V[:, 1])
    return int(np.argmin(d)) if d.min() < 999.0 else 0


def route_cost(cost, route):
    """cost of a route of vertex indices by the cheapest parallel edge per step; None when a step has no edge"""
    total = 0.0
    for u, v in zip(route[:-1], route[1:]):
        if (u, v) not in cost:
            return None
        total += cost[(u, v)]
    return total


def positions_cost(V, cost, path, s, t):
    """Least cost of a walk from vertex s to vertex t whose vertices lie at the positions path[1:-1], one after the other --
    None when there is no such walk.  Vertices are matched by exact coordinates; where several share a position the walk may
    use any of them (a dynamic programme over the sets), so the result is the cost of a real walk from s to t: never below
    Dijkstra's distance, and equal to it exactly when the positions can be a shortest route."""
    sets = [np.flatnonzero((V[:, 0] == p[0]) & (V[:, 1] == p[1])).tolist() for p in path[1:-1]]
    if not sets or s not in sets[0] or t not in sets[-1]:
        return None
    best = {s: 0.0}
    for nxt in sets[1:]:
        step = {}
        for u, du in best.items():
            for v in nxt:
                if (u, v) in cost and du + cost[(u, v)] < step.get(v, np.inf):
                    step[v] = du + cost[(u, v)]
        best = step
    return best.get(t)
