#!/usr/bin/env python3
"""sha256 of the gfx950 device assembly of every unit of csrc/Makefile's SRCS, for one csrc/ directory or several side by side.

A refactor that claims "the device code is unchanged" is checked with it on the CPU: extract the parent's tree next to the
working tree (`git archive <parent> ros_navigation_amd/csrc include | tar -x -C /tmp/parent`) and run

    python3 scripts/device_asm_sha.py /tmp/parent/ros_navigation_amd/csrc ros_navigation_amd/csrc

Every unit is compiled with the command line its Makefile prints for the object file (per-file flags included, as
tests/_build.py derives it), `-c ... -o unit.o` replaced by `-S --cuda-device-only -o -`.  Needs hipcc, no GPU."""
import concurrent.futures
import hashlib
import os
import re
import shlex
import subprocess
import sys


def units(csrc):
    return re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()


def asm_sha(csrc, src):
    obj = src[:-len(".hip")] + ".o"
    dry = subprocess.run(["make", "-n", "-B", "-C", csrc, obj], capture_output=True, text=True, check=True)
    lines = [shlex.split(l) for l in dry.stdout.splitlines() if l.rstrip().endswith(" -c %s -o %s" % (src, obj))]
    assert len(lines) == 1, dry.stdout
    out = subprocess.run(lines[0][:-2] + ["-S", "--cuda-device-only", "-o", "-"], cwd=csrc, capture_output=True, check=True)
    return hashlib.sha256(out.stdout).hexdigest()


def source_lines(csrc):
    return sum(len(open(os.path.join(csrc, f), "rb").read().splitlines()) for f in sorted(os.listdir(csrc))
               if re.search(r"\.(hip|hpp|h|cpp)$|^Makefile$", f))


def main(dirs):
    names = units(dirs[-1])
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        shas = {(d, s): pool.submit(asm_sha, d, s) for d in dirs for s in names if os.path.exists(os.path.join(d, s))}
    differ = 0
    for s in names:
        row = [shas[(d, s)].result() if (d, s) in shas else "-" * 64 for d in dirs]
        same = len(set(row)) == 1
        differ += not same
        print("%-16s %s%s" % (s, "  ".join(row), "" if len(dirs) == 1 else ("  identical" if same else "  DIFFERS")))
    for d in dirs:
        print("%s: %d source lines (*.hip *.hpp *.h *.cpp Makefile)" % (d, source_lines(d)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:] or [os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ros_navigation_amd", "csrc")]))
