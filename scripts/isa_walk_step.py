"""Developer tool: static instruction count of ONE STEP of the grid-A* path walk (tsa_backtrace_wave, astar_tile.hip) on its laid-out
path, and of the parent-map loop in front of it, in the assembly of a kernel that holds the walk.
  hipcc <the Makefile's flags for astar_tile.hip> -S --cuda-device-only astar_tile.hip -o /tmp/astar_tile.s
  python scripts/isa_walk_step.py /tmp/astar_tile.s [kernel symbol]
The step: the shortest way, counted in instructions, round the walk's inner loop -- from the `; TSA_STEP begin` comment through
`; TSA_STEP end` back to `; TSA_STEP begin`, following branches as the assembly lays them out and never through a store to global
memory (the 64 parked cells leave once in 64 steps).  A build without those comments (the walk that probed its eight neighbours at
every cell) is measured round the first loop of depth 2 behind `; TSA_WALK begin`, the same way, through the bit search that picks
the move from the ballot; that walk's step depends on the move it finds, so the shortest way is its cheapest move.
tests/test_astar_trace_parents_host.py bounds the step with step_counts()."""
import collections
import heapq
import re
import sys

TRACE = "_ZN3rna16tsa_trace_kernelENS_9TsaLaunchE"


def kernel_body(asm, symbol):
    lines = asm.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(symbol + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return [l.strip() for l in lines[start:end]]


def is_instruction(l):
    return bool(l) and l[0] not in ";." and not l.endswith(":")


def kind(l):
    op = l.split()[0]
    return "valu" if op.startswith("v_") else "salu" if op.startswith("s_") else "lds" if op.startswith("ds_") else "vmem"


def shortest(body, src, dst):
    """the cheapest way from line src to line dst in instructions (comments and labels cost nothing; src is counted, dst is not),
    over at least one edge, as a list of line numbers; None if there is none"""
    labels = {m.group(1): i for i, m in ((i, re.match(r"(\.LBB\w+):", l)) for i, l in enumerate(body)) if m}

    def after(i):
        l = body[i]
        if not is_instruction(l):
            return [i + 1]
        if l.startswith("global_store") or l.startswith("s_endpgm"):
            return []
        if l.startswith("s_branch"):
            return [labels[l.split()[1]]]
        return [i + 1] + ([labels[l.split()[1]]] if l.startswith("s_cbranch") else [])

    cost = lambda i: 1 if is_instruction(body[i]) else 0
    dist, prev, heap = {}, {}, []
    for j in after(src):
        if j < len(body) and cost(src) < dist.get(j, 1 << 30):
            dist[j], prev[j] = cost(src), src
            heapq.heappush(heap, (cost(src), j))
    while heap:
        d, i = heapq.heappop(heap)
        if i == dst:
            path = [prev[i]]
            while path[-1] != src:
                path.append(prev[path[-1]])
            return path[::-1]
        if d > dist[i]:
            continue
        for j in after(i):
            if j < len(body) and d + cost(i) < dist.get(j, 1 << 30):
                dist[j], prev[j] = d + cost(i), i
                heapq.heappush(heap, (d + cost(i), j))
    return None


def step_counts(asm, symbol=TRACE):
    """{"step": {kind: n, "all": n}, "parents": {...} or None} of the kernel `symbol`"""
    body = kernel_body(asm, symbol)
    walk = next(i for i, l in enumerate(body) if "TSA_WALK begin" in l)
    begin = [i for i, l in enumerate(body) if "TSA_STEP begin" in l]
    end = [i for i, l in enumerate(body) if "TSA_STEP end" in l]
    if begin:
        assert len(begin) == 1 and len(end) == 1, (begin, end)
        there, back = shortest(body, begin[0], end[0]), shortest(body, end[0], begin[0])
        assert there and back, "no way round the step's loop"
        path = there + back
    else:
        head = next(i for i in range(walk, len(body)) if "Inner Loop Header: Depth=2" in body[i])
        probe = next(i for i in range(head, len(body)) if body[i].startswith("s_ff1_i32_b32"))   # the move is picked from the ballot
        there, back = shortest(body, head, probe), shortest(body, probe, head)
        assert there and back, "no way round the walk's loop"
        path = there + back
    out = {"step": collections.Counter(kind(body[i]) for i in path if is_instruction(body[i])), "parents": None}
    a = [i for i, l in enumerate(body) if "TSA_PARENTS begin" in l]
    b = [i for i, l in enumerate(body) if "TSA_PARENTS end" in l]
    if a:
        assert len(a) == 1 and len(b) == 1 and a[0] < b[0]
        out["parents"] = collections.Counter(kind(l) for l in body[a[0]:b[0]] if is_instruction(l))
    for c in (out["step"], out["parents"]):
        if c is not None:
            c["all"] = sum(c.values())
    return out


if __name__ == "__main__":
    res = step_counts(open(sys.argv[1]).read(), sys.argv[2] if len(sys.argv) > 2 else TRACE)
    for name in ("step", "parents"):
        c = res[name]
        if c is None:
            print("%-8s (no such region in this build)" % name)
        else:
            print("%-8s all %4d | valu %4d salu %4d lds %3d vmem %3d" % (name, c["all"], c["valu"], c["salu"], c["lds"], c["vmem"]))
