"""The waypoint-graph A* ORACLE (og_graph_astar, og_graph_closest_vertex; oracle/astar.c) against references that share nothing
with it -- no GPU.  oracle/astar.c restates boost::astar_search statement for statement, and graph_astar_kernel restates the same
statements again: tests/test_gpu_graph_astar.py holds the kernel to the oracle bit for bit, this file holds the oracle to
  * a plain Dijkstra (tests/_graph_cases.py: float64, heapq) on every case whose weights are admissible and sum exactly: the
    route starts at the closest start vertex, ends at the closest goal vertex, walks along edges and costs exactly Dijkstra's
    distance; and on every case of every family there is a route iff Dijkstra reaches the goal;
  * a float64 numpy argmin for the closest vertex, lowest index among equals, vertex 0 beyond 999 m;
and asserts, from counters inside the oracle, that the committed cases reach the branches a wrong kernel would differ in
(premises: if one fails the CASES are wrong -- change tests/_graph_cases.py until it holds)."""
import ctypes as C

import numpy as np
import pytest

import _graph_cases as G
import _oracle as O
from _build import capi  # noqa: F401  (the fixture)

RNA_EINVAL = -1


def checked(case):
    """per query of a case: (has a route, route length in vertices) after the Dijkstra checks that apply to the case"""
    V, E, W = case["V"], case["E"], case["W"]
    cost = G.edge_costs(E, W)
    dist = {}
    out = []
    for k, (s, t, route, path) in enumerate(G.oracle_answers(case["name"])):
        q = case["st"][k]
        assert s == G.closest_vertex(V, q[0], q[1]) and t == G.closest_vertex(V, q[2], q[3]), (case["name"], k)
        if s not in dist:
            dist[s] = G.dijkstra(len(V), E, W, s)
        assert bool(route) == bool(dist[s][t] < np.inf), (case["name"], k, s, t, route)
        if route and case["exact"]:
            assert route[0] == s and route[-1] == t, (case["name"], k, route)
            assert len(set(route)) == len(route), (case["name"], k, route)
            c = G.route_cost(cost, route)
            assert c is not None, (case["name"], k, "a step of the route is no edge", route)
            assert c == dist[s][t], (case["name"], k, route, c, dist[s][t])
        if route:
            assert np.array_equal(path[0], q[:2]) and np.array_equal(path[-1], q[2:]) and np.array_equal(path[1:-1], V[list(route)])
        out.append((bool(route), len(route)))
    return out


@pytest.mark.parametrize("name", G.names())
def test_oracle_routes_are_dijkstra_routes(name):
    checked(G.by_name(name))


def test_euclid_cases_have_routes_and_dead_ends():
    """what the Dijkstra check asserts about its own inputs: at least half of the euclid queries have a route, at least a
    tenth have none, and some routes are long enough to have a choice"""
    res = [r for c in G.random_cases("euclid") for r in checked(c)]
    n, with_route = len(res), sum(r[0] for r in res)
    print("euclid: %d queries, %d with a route, longest %d vertices" % (n, with_route, max(r[1] for r in res)))
    assert with_route >= n / 2 and n - with_route >= n / 10, (n, with_route)
    assert max(r[1] for r in res) >= 8


def counters_of(cases):
    O.graph_astar_counters()            # zero them
    L = O.lib()
    for c in cases:
        for q in c["st"]:
            s, t = G.oracle_closest(L, c["V"], q[0], q[1]), G.oracle_closest(L, c["V"], q[2], q[3])
            G.oracle_route(L, c["V"], c["E"], c["W"], s, t)
    return O.graph_astar_counters()


def test_premises_hold_without_a_gpu():
    n = {f: counters_of(G.random_cases(f)) for f in G.FAMILIES}
    print(n)
    # the free family is the one that drives relax()'s undirected branch, the re-opening of black vertices and decrease-key
    assert n["free"]["undirected"] > 0 and n["free"]["black_reopened"] > 0 and n["free"]["gray_decreased"] > 0, n["free"]
    for f in G.FAMILIES:
        assert n[f]["max_heap"] > 5, (f, n[f])          # a 4-ary heap of six entries has a second level
    # batches end before, at and after the end of a workgroup, and go on into a fourth one
    assert {len(c["st"]) for f in G.FAMILIES for c in G.random_cases(f)} == set(G.NQ)
    for f in G.FAMILIES:
        assert {len(c["V"]) for c in G.random_cases(f)} == set(G.NV)
    # closest-vertex ties: queries whose nearest distance is shared by two vertices at different indices
    ties = 0
    for c in G.random_cases("euclid"):
        for q in c["st"]:
            d = np.hypot(q[0] - c["V"][:, 0], q[1] - c["V"][:, 1])
            ties += int((d == d.min()).sum() > 1)
    assert ties >= 50, ties


def test_hand_cases_are_what_they_say():
    ans = {n: G.oracle_answers(n) for n in G.names("hand")}
    assert [c["name"] for c in G.hand_cases()] == G.names("hand") and [c["name"] for c in G.all_cases()] == G.names()
    # two components: routes inside each, none across
    r = ans["two-components"]
    assert any(a[2] and a[0] < 4 for a in r) and any(a[2] and a[0] >= 4 for a in r) and any(not a[2] and (a[0] < 4) != (a[1] < 4) for a in r)
    assert all(bool(a[2]) == ((a[0] < 4) == (a[1] < 4)) for a in r)
    # parallel edges: 0 -> 1 directly by the cheaper edge (2.5 < the detour's 4 < 5), 1 -> 3 by the cheapest of three
    c = G.by_name("parallel-edges")
    assert G.oracle_route(O.lib(), c["V"], c["E"], c["W"], 0, 1) == [0, 1] and G.oracle_route(O.lib(), c["V"], c["E"], c["W"], 0, 3) == [0, 1, 3]
    assert G.edge_costs(c["E"], c["W"])[(0, 1)] == 2.5 and G.edge_costs(c["E"], c["W"])[(3, 1)] == 2.0
    # FLT_MAX: round it, never across it; the vertex behind it alone comes back as a route of itself
    c = G.by_name("flt-max-edge")
    L = O.lib()
    assert G.oracle_route(L, c["V"], c["E"], c["W"], 0, 1) == [0, 2, 1] and G.oracle_route(L, c["V"], c["E"], c["W"], 1, 0) == [1, 2, 0]
    assert G.oracle_route(L, c["V"], c["E"], c["W"], 0, 3) == [3]
    assert any(a[2] == (3,) and a[0] != 3 for a in ans["flt-max-edge"]) and any(len(a[2]) == 3 for a in ans["flt-max-edge"])
    # beyond 999 m: vertex 0 although vertex 2 is the nearest; 998.5 m is inside, 999 m is not
    c = G.by_name("beyond-999m")
    r = ans["beyond-999m"]
    assert (r[0][0], r[0][1]) == (0, 0) and r[0][2] == (0,) and len(r[0][3]) == 3
    assert int(np.argmin(np.hypot(c["V"][:, 0], c["V"][:, 1]))) == 2
    assert r[3][0] == 2 and r[4][0] == 0 and r[1][1] == 3
    # no edges: a route iff start and goal snap to the same vertex, and then it is that vertex
    r = ans["no-edges"]
    assert any(a[2] for a in r) and any(not a[2] for a in r) and all((a[0] == a[1]) == bool(a[2]) and len(a[2]) <= 1 for a in r)
    assert all(a[0] != 2 and a[1] != 2 for a in r)       # vertex 2 duplicates vertex 0: never the closest
    # the line: 256 vertices, 258 positions, both ways
    r = ans["line-256"]
    assert r[0][2] == tuple(range(256)) and len(r[0][3]) == 258 and r[1][2] == tuple(range(255, -1, -1))
    assert r[4][2] == (r[4][0],) and r[4][0] in (120, 121)


@pytest.mark.parametrize("name", G.names("euclid") + ["beyond-999m", "no-edges", "reference-weighted"])
def test_closest_vertex_matches_numpy(name):
    c = G.by_name(name)
    L = O.lib()
    rng = np.random.default_rng(7)
    pts = np.concatenate([c["st"].reshape(-1, 2), c["V"][rng.integers(0, len(c["V"]), 16)]])   # lattice queries; vertices themselves
    for x, y in pts:
        assert G.oracle_closest(L, c["V"], x, y) == G.closest_vertex(c["V"], x, y), (name, x, y)


def test_refusals_come_before_the_engine_is_touched(capi):
    """rna_graph_astar_batch's argument checks with an engine pointer that must never be dereferenced: a bad graph, a negative
    weight among them, is refused before anything is staged or launched"""
    L = capi.lib()
    fake = C.c_void_p(1)
    V = np.array([[0, 0], [1, 0], [5, 5]], np.float64)
    E = np.array([[0, 1], [1, 2]], np.int32)
    st = np.zeros((2, 4))
    paths, plen = np.full((2, 8, 2), 7.0), np.full(2, 7, np.int32)
    p = capi._ptr

    def call(nv=3, E=E, W=None, n=2, max_len=8, engine=fake):
        W = None if W is None else np.asarray(W, np.float32)
        return L.rna_graph_astar_batch(engine, nv, p(V), len(E), p(E), p(W) if W is not None else None, p(st), n, p(paths), max_len, p(plen))

    assert call(engine=None) == RNA_EINVAL
    assert call(nv=0) == RNA_EINVAL and call(nv=257) == RNA_EINVAL and call(max_len=2) == RNA_EINVAL and call(n=-1) == RNA_EINVAL
    assert call(E=np.array([[0, 1], [1, 3]], np.int32)) == RNA_EINVAL and call(E=np.array([[-1, 1], [1, 2]], np.int32)) == RNA_EINVAL
    for W in ([-1, 1], [1, -1], [0.5, -1e-30], [-np.inf, 2], [np.nan, -0.125]):
        assert call(W=W) == RNA_EINVAL, W
    assert call(n=0) == 0 and call(n=0, W=[1, 2]) == 0       # an empty batch is RNA_OK
    assert np.all(paths == 7.0) and np.all(plen == 7)
    # a weight array that is not one per edge never reaches the library
    with pytest.raises(ValueError):
        capi.Engine.graph_astar(None, V, E, st, edge_weight=[1.0])


def test_negative_edge_runs_until_float_absorption():
    """Why rna_graph_astar_batch refuses a negative weight (include/rna.h): two vertices joined by an edge of weight -1 and a
    goal that is not connected.  relax() lowers either end in turn and re-opens it, until d - 1 == d in float32: 2^24 pops.
    This runs the CPU oracle alone; the kernel is never given such a graph."""
    V = np.array([[0, 0], [1, 0], [5, 5]], np.float64)
    E = np.array([[0, 1]], np.int32)
    O.graph_astar_counters()
    assert G.oracle_route(O.lib(), V, E, np.array([-1], np.float32), 0, 2) == []
    n = O.graph_astar_counters()
    print(n)
    assert n["pops"] >= 2 ** 24 and n["black_reopened"] + n["gray_decreased"] >= 2 ** 24 - 2, n
    O.graph_astar_counters()
    assert G.oracle_route(O.lib(), V, E, np.array([1], np.float32), 0, 2) == []
    assert O.graph_astar_counters()["pops"] == 2
