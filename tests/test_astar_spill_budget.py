"""CPU-only (hipcc cross-compiles): the spill budget of the pipelined grid-A* search kernel.  The tile job is bound by instruction
issue, and a spilled SGPR costs the vector port twice -- a v_writelane where it is put away, a v_readlane (mostly with a wait state
behind it) wherever it is needed again.  The kernel compiled with the Makefile's own flags must keep 64 VGPRs, must not grow its
scratch, must not spill more than the counts committed here -- which lie below the 110 SGPRs / 5 VGPRs of the kernel before the
halo step formed its pass-on thresholds in one block of assembly per row and the loop that takes the jobs stopped carrying lane masks
and a 64-bit LDS address across them (profiles/astar_spill_sites_*.txt, profiles/astar_spill_steps.txt) -- and must keep the sweeps,
where most of a job's instructions are issued, free of spill traffic."""
import re

from _build import device_asm, needs_hipcc, resources

# <WAVES, RETRY> -> (sgpr_spill_count, vgpr_spill_count) of the committed kernel
COMMITTED = {"ILi8ELb0E": (67, 4), "ILi8ELb1E": (71, 3)}
BEFORE = (110, 5)          # tsa_search_kernel<8, false> before; the other instantiations had 109-113 / 5
SCRATCH_BYTES = 24


def metadata(asm, sym):
    """the .amdhsa metadata entry of the kernel whose symbol contains `sym`, as {key: int}"""
    m = re.search(r"\.name:\s+\S*tsa_search_kernel%s\S*\n(.*?)\.wavefront_size" % sym, asm, re.S)
    assert m, sym
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", m.group(1))}


def kernel_lines(asm, sym):
    lines = asm.split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"_ZN3rna17tsa_search_kernel%s\w*:" % sym, l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    return [l.strip() for l in lines[start:end]]


def spill_registers(lines):
    """VGPRs whose lanes hold spilled SGPRs: written lane by lane from scalar registers OUTSIDE inline assembly (the job's own
    v_writelane -- a column candidate into lane 0 / 63 of a row -- are inline assembly)"""
    count, in_asm = {}, False
    for l in lines:
        if l.startswith(";;#ASMSTART"):
            in_asm = True
        elif l.startswith(";;#ASMEND"):
            in_asm = False
        elif not in_asm:
            m = re.match(r"v_writelane_b32 (v\d+), s\d+, \d+$", l)
            if m:
                count[m.group(1)] = count.get(m.group(1), 0) + 1
    return {r for r, n in count.items() if n >= 8}


@needs_hipcc
def test_the_search_kernel_spills_less_than_before():
    asm = device_asm("astar_tile.hip")
    res = resources("astar_tile.hip")
    for sym, (sgpr, vgpr) in COMMITTED.items():
        md = metadata(asm, sym)
        r = next(v for k, v in res.items() if "tsa_search_kernel" + sym in k)
        print(sym, md["sgpr_spill_count"], md["vgpr_spill_count"], md["vgpr_count"], md["private_segment_fixed_size"], r)
        assert md["vgpr_count"] == 64 and r["VGPRs"] == 64, (sym, md, r)          # eight wavefronts per SIMD
        assert md["private_segment_fixed_size"] <= SCRATCH_BYTES and r["ScratchSize"] <= SCRATCH_BYTES, (sym, md, r)
        assert md["sgpr_spill_count"] <= sgpr and md["vgpr_spill_count"] <= vgpr, (sym, md)
        assert sgpr < BEFORE[0] and vgpr <= BEFORE[1]


@needs_hipcc
def test_no_spill_traffic_inside_the_sweeps():
    """between the marks halo_end and results_begin -- the row evaluations of both sweeps as the block placement laid them out -- no
    lane of a spill register is read or written (a row's scan and other rare blocks are placed elsewhere)"""
    lines = kernel_lines(device_asm("astar_tile.hip"), "ILi8ELb0E")
    regs = spill_registers(lines)
    assert regs, "no spill register found: the kernel does spill SGPRs"
    a = next(i for i, l in enumerate(lines) if "TSA_MARK halo_end" in l)
    b = next(i for i, l in enumerate(lines) if "TSA_MARK results_begin" in l)
    assert 0 < a < b and b - a > 2000, (a, b)      # the sweeps are the bulk of the job
    inside = [l for l in lines[a:b]
              if (re.match(r"v_readlane_b32 s\d+, (v\d+), \d+$", l) or re.match(r"v_writelane_b32 (v\d+), s\d+, \d+$", l))
              and re.search(r"\b(v\d+)\b", l).group(1) in regs]
    assert not inside, inside
