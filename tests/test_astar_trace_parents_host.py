"""CPU-only: the parent map of the grid-A* path walk (tsa_backtrace_wave, astar_tile.hip).  Per tile the walking wavefront decides
for all 1 024 cells at once which neighbour each steps to, and a step then reads that code.
  - the rule, one cell: tests/cpp/astar_trace_parent_test.cpp compiles csrc/astar_trace_parent.hpp -- the text the kernel compiles --
    with the host compiler and checks tsa_parent_code on two million random 3 x 3 neighbourhoods (unreached words, several
    neighbours that tie, mask bytes that forbid the first of them) against a restatement of the oracle's backtrace;
  - the resources (hipcc cross-compiles, the Makefile's own flags): the parent-map loop and the step are marked with comments in
    the assembly of every kernel that holds the walk; the step's instructions on its laid-out path (scripts/isa_walk_step.py) are
    bounded by what this change reached plus two: 25 in the trace kernel, where the walk that probed eight neighbours at every cell
    had 91 on its cheapest move (profiles/astar_trace_parents.txt)."""
import importlib.util
import os
import subprocess

from _build import BIN_DIR, ROOT, device_asm, needs_hipcc

STEP_REACHED = 25          # tsa_trace_kernel, this change; profiles/astar_trace_parents.txt
STEP_BOUND = STEP_REACHED + 2
SEARCH = "_ZN3rna17tsa_search_kernelILi%dELb%dEEEvNS_9TsaLaunchE"


def test_the_rule_of_one_cell_against_the_oracles_backtrace():
    os.makedirs(BIN_DIR, exist_ok=True)
    exe = os.path.join(BIN_DIR, "astar_trace_parent_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "astar_trace_parent_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "checked 2000000" in out.stdout


def _tool():
    spec = importlib.util.spec_from_file_location("isa_walk_step", os.path.join(ROOT, "scripts", "isa_walk_step.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@needs_hipcc
def test_a_step_reads_its_parent_and_stays_within_its_instruction_budget():
    tool = _tool()
    asm = device_asm("astar_tile.hip")
    for symbol in (tool.TRACE, SEARCH % (16, 0), SEARCH % (8, 1), SEARCH % (16, 1)):
        body = tool.kernel_body(asm, symbol)
        for mark in ("TSA_PARENTS begin", "TSA_PARENTS end", "TSA_STEP begin", "TSA_STEP end"):
            assert sum(1 for l in body if mark in l) == 1, (symbol, mark)
        c = tool.step_counts(asm, symbol)
        print(symbol, dict(c["step"]), dict(c["parents"]))
        assert c["step"]["all"] <= STEP_BOUND, (symbol, c["step"])
        # a step: one byte of the parent map and nothing else from memory; no probe, no ballot, no store on its path
        assert c["step"]["lds"] == 1 and c["step"]["vmem"] == 0, (symbol, c["step"])
        # the parent map is made in LDS alone; its loop takes four rows a turn, and a neighbour's test (reached, equal, allowed, join)
        # is no more than eight instructions: 4 rows x 8 neighbours x 8
        assert c["parents"]["vmem"] == 0 and 0 < c["parents"]["all"] <= 4 * 8 * 8, (symbol, c["parents"])
    # the pipelined first pass hands its paths over: neither region is in its code
    first = tool.kernel_body(asm, SEARCH % (8, 0))
    assert not any("TSA_STEP" in l or "TSA_PARENTS" in l for l in first)
