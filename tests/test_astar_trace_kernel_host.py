"""CPU-only (hipcc cross-compiles): the resources of the grid-A* trace kernel.  Its workgroup -- eight wavefronts, one path each --
is there to take the place one search workgroup leaves on a CU that three others still hold: two wavefronts per SIMD next to the
searches' six, so at most 64 VGPRs like them, nothing in scratch (the walk is one chain of dependent instructions; a reload in it
is a memory round trip per step), and its eight LDS images beside three search workgroups' LDS at the bench's map size.  The
pipelined search kernel in turn no longer holds the walk's code."""
import os
import re

from _build import CSRC, device_asm, needs_hipcc, resources

LDS_PER_CU = 160 * 1024
TI, TJ = 64, 16
PATHS = 8                                                  # TSA_TRACE_PATHS
IMAGE_BYTES = (TI + 2) * (TJ + 2) * 4 + TI * TJ            # a tile with its halo ring in words, the tile's masks in bytes


@needs_hipcc
def test_a_trace_workgroup_fits_where_a_search_workgroup_was():
    tile = resources("astar_tile.hip")
    trace = next(v for k, v in tile.items() if "tsa_trace_kernel" in k)
    search = next(v for k, v in tile.items() if "tsa_search_kernelILi8ELb0E" in k)
    assert trace["VGPRs"] <= 64 and trace["AGPRs"] == 0, trace
    assert trace["ScratchSize"] == 0, trace
    bench_search_lds = search["LDS"] + 4 * 4 * ((64 * 256 + 31) // 32)      # + the four tile bit sets of a 4096 x 4096 map
    assert trace["LDS"] + PATHS * IMAGE_BYTES + 3 * bench_search_lds <= LDS_PER_CU, (trace["LDS"], PATHS * IMAGE_BYTES, bench_search_lds)
    # the launch sizes the dynamic LDS by the same two constants
    src = open(os.path.join(CSRC, "astar_tile.hip")).read()
    assert re.search(r"constexpr int TSA_TRACE_PATHS = %d;" % PATHS, src)
    assert re.search(r"constexpr int TSA_TRACE_IMAGE_WORDS = BW \* \(TJ \+ 2\) \+ TILE_WORDS / 4;", src) and "constexpr int BW = TI + 2;" in src


@needs_hipcc
def test_only_the_kernels_that_trace_inside_hold_the_walk():
    """the walk marks its beginning with a comment in the assembly: it is in the trace kernel, in the latency instantiation and in
    both retry instantiations of the search kernel, and not in the pipelined first pass; the trace wavefronts raise their issue
    priority as the walking wavefront of a search workgroup does"""
    lines = device_asm("astar_tile.hip").split("\n")

    def body(symbol):
        start = next(i for i, l in enumerate(lines) if l.startswith(symbol + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))     # (a kernel may end in several places)
        return [l.strip() for l in lines[start:end]]

    def walks(symbol):
        return sum(1 for l in body(symbol) if "TSA_WALK begin" in l)

    search = "_ZN3rna17tsa_search_kernelILi%dELb%dEEEvNS_9TsaLaunchE"
    trace = "_ZN3rna16tsa_trace_kernelENS_9TsaLaunchE"
    assert walks(trace) == 1 and any(re.match(r"s_setprio 3\b", l) for l in body(trace))
    assert walks(search % (16, 0)) == 1 and walks(search % (8, 1)) == 1 and walks(search % (16, 1)) == 1
    assert walks(search % (8, 0)) == 0
