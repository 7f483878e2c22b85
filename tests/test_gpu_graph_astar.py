"""graph_astar_kernel (ros_navigation_amd/csrc/planners.hip) on weighted graphs of up to 256 vertices: the cases of
tests/_graph_cases.py (three weight families on the 0.5 m lattice, the hand-written graphs), batches that cross a workgroup,
the output contract of rna_graph_astar_batch and its refusals.

Two references.  The oracle (og_graph_closest_vertex + og_graph_astar + start / target, assembled as AStarPlanner::makePlan does)
must be met bit for bit: both sides restate boost::astar_search statement for statement and both are built without FMA
contraction.  Because the oracle is the kernel's twin, the kernel's answers are ALSO held, without going through the oracle, to a
plain float64 Dijkstra wherever the heuristic is admissible: the positions that come back are matched to vertices by their
coordinates and must be a walk along edges, from the closest start vertex to the closest goal vertex, of Dijkstra's cost exactly.
tests/test_graph_astar_host.py (no GPU) asserts what these inputs reach."""
import numpy as np
import pytest

import _graph_cases as G
import _oracle as O  # noqa: F401  (the oracle library is built by the session fixture)
from _gpu import R  # noqa: F401  (R: the fixture)

pytestmark = pytest.mark.gpu
SENT = -12345.678               # what a caller left in the output rows
SENT_LEN = -77


def engine(R):
    return R.Engine(2.0, 2.0, 0.05)     # nothing here needs the map


def raw(R, e, V, E, W, st, max_len, nv=None, ne=None, n=None):
    """rna_graph_astar_batch itself, into rows the caller filled with SENT -> (status, path_len, paths)"""
    V, st = np.ascontiguousarray(V, np.float64), np.ascontiguousarray(st, np.float64)
    E = np.ascontiguousarray(E, np.int32)
    W = None if W is None else np.ascontiguousarray(W, np.float32)
    rows = max(len(st), 1)
    paths = np.full((rows, max(max_len, 1), 2), SENT, np.float64)
    plen = np.full(rows, SENT_LEN, np.int32)
    p = R.capi._ptr
    rc = e._L.rna_graph_astar_batch(e.h, len(V) if nv is None else nv, p(V), len(E) if ne is None else ne, p(E),
                                    p(W) if W is not None else None, p(st), len(st) if n is None else n, p(paths), max_len, p(plen))
    return rc, plen, paths


def assert_matches_oracle(plen, paths, want, tag):
    for k, (s, t, route, path) in enumerate(want):
        assert plen[k] == len(path), (tag, k, int(plen[k]), len(path), s, t)
        assert np.array_equal(paths[k, :len(path)], path), (tag, k, s, t, paths[k, :plen[k]].tolist(), path.tolist())


def case_against_oracle(R, name):
    c = G.by_name(name)
    e = engine(R)
    plen, paths = e.graph_astar(c["V"], c["E"], c["st"], edge_weight=c["W"])
    e.close()
    assert_matches_oracle(plen, paths, G.oracle_answers(name), name)


@pytest.mark.parametrize("name", [n for f in G.FAMILIES for n in G.names(f)])
def test_kernel_matches_oracle(R, name):
    case_against_oracle(R, name)


@pytest.mark.parametrize("name", G.names("hand"))
def test_hand_written_cases_match_oracle(R, name):
    case_against_oracle(R, name)


@pytest.mark.parametrize("name", [c["name"] for c in G.all_cases() if c["exact"]])
def test_kernel_routes_cost_what_dijkstra_says(R, name):
    """no oracle on this path: numpy's closest vertex, Dijkstra's distance, the kernel's positions"""
    c = G.by_name(name)
    V, E, W, st = c["V"], c["E"], c["W"], c["st"]
    e = engine(R)
    plen, paths = e.graph_astar(V, E, st, edge_weight=W)
    e.close()
    cost = G.edge_costs(E, W)
    dist = {}
    for k, q in enumerate(st):
        s, t = G.closest_vertex(V, q[0], q[1]), G.closest_vertex(V, q[2], q[3])
        if s not in dist:
            dist[s] = G.dijkstra(len(V), E, W, s)
        if dist[s][t] == np.inf:
            assert plen[k] == 0, (name, k, s, t, int(plen[k]))
            continue
        assert 3 <= plen[k] <= len(V) + 2, (name, k, int(plen[k]))
        path = paths[k, :plen[k]]
        assert np.array_equal(path[0], q[:2]) and np.array_equal(path[-1], q[2:]), (name, k)
        got = G.positions_cost(V, cost, path, s, t)
        assert got is not None, (name, k, s, t, "not a walk along edges from the start vertex to the goal vertex", path.tolist())
        assert got == dist[s][t], (name, k, s, t, got, dist[s][t], path.tolist())


def test_batches_across_workgroups(R):
    """the scratch of query q lies at q * 2 nv floats and q * 4 nv ints and lane q >= n leaves: one query gives one row wherever
    it stands in a batch of 200 on 256 vertices, and the row it gets alone"""
    c = next(c for c in G.random_cases("free") if len(c["V"]) == 256 and len(c["E"]) > 256)
    V, E, W = c["V"], c["E"], c["W"]
    rng = np.random.default_rng(11)
    st = G.lattice_queries(rng, 200)
    probe = next(q for q, a in zip(c["st"], G.oracle_answers(c["name"])) if len(a[2]) >= 4)     # a query with a route of some length
    at = (0, 63, 64, 65, 199)
    st[list(at)] = probe
    want = G.oracle_plan(V, E, W, st)
    assert sum(1 for a in want if a[2]) >= 50
    e = engine(R)
    plen, paths = e.graph_astar(V, E, st, edge_weight=W)
    assert_matches_oracle(plen, paths, want, "200")
    alone_len, alone = e.graph_astar(V, E, st[:1], edge_weight=W)
    assert alone_len[0] == len(want[0][3]) >= 6
    for k in at:
        assert plen[k] == alone_len[0] and np.array_equal(paths[k], alone[0]), k
    # a batch of 65: the one query of the second workgroup is answered, the 63 idle lanes beside it write nothing
    rc, plen65, paths65 = raw(R, e, V, E, W, st[:65], 258)
    assert rc == R.capi.RNA_OK
    assert plen65[64] == plen[64] > 0 and np.array_equal(paths65[64, :plen[64]], paths[64, :plen[64]])
    assert np.array_equal(plen65, plen[:65])
    for k in range(65):
        assert np.array_equal(paths65[k, :plen[k]], paths[k, :plen[k]]) and np.all(paths65[k, plen[k]:] == SENT), k
    e.close()


def test_output_contract(R):
    e = engine(R)
    # a mixed batch at a max_len equal to one route's length: that row and every shorter one are written whole and no further,
    # a longer one reports its length and is left alone, a query without a route reports 0 and is left alone
    c = next(c for c in G.random_cases("euclid") if len(c["V"]) == 200 and len(c["st"]) >= 63)
    want = G.oracle_answers(c["name"])
    lens = sorted({len(a[3]) for a in want})
    assert lens[0] == 0 and len(lens) >= 5
    exact = lens[len(lens) // 2]
    for max_len in (exact, exact - 1):
        rc, plen, paths = raw(R, e, c["V"], c["E"], c["W"], c["st"], max_len)
        assert rc == R.capi.RNA_OK
        seen = set()
        for k, a in enumerate(want):
            n = len(a[3])
            assert plen[k] == n, (max_len, k)
            if 0 < n <= max_len:
                assert np.array_equal(paths[k, :n], a[3]) and np.all(paths[k, n:] == SENT), (max_len, k)
            else:
                assert np.all(paths[k] == SENT), (max_len, k, n)
            seen.add("none" if n == 0 else "fits" if n < max_len else "whole" if n == max_len else "one short" if n == max_len + 1 else "short")
        assert seen >= ({"none", "fits", "whole", "short"} if max_len == exact else {"none", "fits", "one short"}), (max_len, seen)
    # the longest route there is: 256 vertices in a line, 258 positions
    c = G.by_name("line-256")
    want = G.oracle_answers("line-256")
    rc, plen, paths = raw(R, e, c["V"], c["E"], c["W"], c["st"], 258)
    assert rc == R.capi.RNA_OK and plen[0] == 258 and plen[1] == 258
    assert_matches_oracle(plen, paths, want, "line-256 at 258")
    assert all(np.all(paths[k, plen[k]:] == SENT) for k in range(len(want)))
    rc, plen, paths = raw(R, e, c["V"], c["E"], c["W"], c["st"], 257)
    assert rc == R.capi.RNA_OK and plen[0] == 258 and plen[1] == 258 and np.all(paths[0] == SENT) and np.all(paths[1] == SENT)
    assert plen[5] == 197 and np.array_equal(paths[5, :197], want[5][3]) and np.all(paths[5, 197:] == SENT)
    e.close()


def test_refusals(R):
    e = engine(R)
    c = G.by_name("parallel-edges")
    V, E, W, st = c["V"], c["E"], c["W"], c["st"]
    nv = len(V)
    EINVAL, OK = -1, R.capi.RNA_OK       # RNA_EINVAL, include/rna.h
    bad_end, minus_one, neg_w, neg_w_last = E.copy(), E.copy(), W.copy(), W.copy()
    bad_end[3, 1] = nv
    minus_one[2, 0] = -1
    neg_w[1] = -0.125
    neg_w_last[-1] = -np.float32(1e-30)
    big = np.zeros((257, 2))
    for what, args in (("nv = 0", dict(V=V, E=E[:0], W=None, max_len=8, nv=0)),
                       ("nv = 257", dict(V=big, E=E, W=W, max_len=300)),
                       ("max_len = 2", dict(V=V, E=E, W=W, max_len=2)),
                       ("an edge end equal to nv", dict(V=V, E=bad_end, W=W, max_len=8)),
                       ("an edge end of -1", dict(V=V, E=minus_one, W=W, max_len=8)),
                       ("a negative weight", dict(V=V, E=E, W=neg_w, max_len=8)),
                       ("a tiny negative weight on the last edge", dict(V=V, E=E, W=neg_w_last, max_len=8)),
                       ("a negative weight of minus infinity", dict(V=V, E=E, W=np.where(np.arange(len(W)) == 0, -np.inf, W), max_len=8))):
        rc, plen, paths = raw(R, e, st=st, **args)
        assert rc == EINVAL, (what, rc)
        assert np.all(plen == SENT_LEN) and np.all(paths == SENT), what      # nothing ran
    # Engine.graph_astar raises for them, and for a weight array that is not one per edge (the library would read past it)
    with pytest.raises(R.capi.RnaError, match="RNA_EINVAL"):
        e.graph_astar(V, E, st, edge_weight=neg_w)
    with pytest.raises(ValueError):
        e.graph_astar(V, E, st, edge_weight=W[:-1])
    # an empty batch is no error
    rc, plen, paths = raw(R, e, V, E, W, st[:0], 8)
    assert rc == OK and np.all(plen == SENT_LEN) and np.all(paths == SENT)
    # -0.0 and NaN are not negative: they pass, and NaN never relaxes (on either side)
    odd = W.copy()
    odd[0], odd[4] = -0.0, np.nan
    rc, plen, paths = raw(R, e, V, E, odd, st, nv + 2)
    assert rc == OK
    assert_matches_oracle(plen, paths, G.oracle_plan(V, E, odd, st), "-0.0 and NaN")
    # and the engine answers a good batch after all of it
    plen, paths = e.graph_astar(V, E, st, edge_weight=W)
    assert_matches_oracle(plen, paths, G.oracle_answers("parallel-edges"), "after the refusals")
    assert plen.max() >= 4
    e.close()
