"""Native build products of a test session, each built ONCE per pytest process (test infrastructure).

Round 3's suite ran `make -C csrc` + `make -C oracle` + a g++ / hipcc link inside every C++ test: on a cold box (fresh
snapshot, compilers and ROCm libraries not yet paged in) that was minutes of the driver's 20.  Here: `native()` runs the
two makes once, `cpp(name)` builds a test binary the first time a test asks for it and hands the same file to every
later test.

The kernel budgets too: `resources(src)` and `device_asm(src)` compile a source of csrc/ with the command line csrc/Makefile
itself prints for its object file -- per-file flags included, so a budget is checked on the build that is the product -- once
per session, and `c_values()` / `sources_in_build_files()` are what the *_host.py test of every feature asks of the header and
of the two build files."""
import os
import re
import shlex
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ros_navigation_amd", "csrc")
LIB_DIR = os.path.join(ROOT, "ros_navigation_amd")
ORACLE_DIR = os.path.join(ROOT, "oracle")
INCLUDE = os.path.join(ROOT, "include")
HOST = os.path.join(LIB_DIR, "host")
HPP = os.path.join(HOST, "move_control_amd.hpp")
HIPCC = "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
BIN_DIR = os.path.join(tempfile.gettempdir(), "rna_test_bin_%d" % os.getuid())

_done = {}


def native():
    """librna.so, librna_rccl.so (HIP, gfx950) and the oracle, once per session"""
    if "native" not in _done:
        subprocess.check_call(["make", "-C", CSRC, "-j8", "-s"])
        subprocess.check_call(["make", "-C", ORACLE_DIR, "-s"], stdout=subprocess.DEVNULL)
        _done["native"] = True


@pytest.fixture(scope="module")
def capi():
    """the ctypes binding, librna.so built first; a test module takes it with `from _build import capi  # noqa: F401`"""
    native()
    from ros_navigation_amd import capi
    return capi


# name -> (source relative to the repo root, kind): "host" = g++ against librna + the oracle (the C++ host mirrors check
# themselves against it), "plain" = g++ alone, "rccl" = hipcc against librna_rccl + librccl
SOURCES = {
    "host_mirror_test": ("tests/cpp/host_mirror_test.cpp", "host"),
    "nav_graph_node_shaped": ("tests/cpp/nav_graph_node_shaped.cpp", "host"),
    "nav_node_shaped": ("tests/cpp/nav_node_shaped.cpp", "host"),
    "rate_loop_test": ("tests/cpp/rate_loop_test.cpp", "plain"),
    "id_bootstrap_test": ("tests/cpp/id_bootstrap_test.cpp", "plain"),
    "gridmath_index_test": ("tests/cpp/gridmath_index_test.cpp", "plain"),
    "map_state_test": ("tests/cpp/map_state_test.cpp", "plain"),
    "vfh_tables_dump": ("tests/cpp/vfh_tables_dump.cpp", "plain"),
    "tiled_host": ("examples/tiled_host.cpp", "rccl"),
}


def cpp(name):
    """path of the test binary `name`, built on first use"""
    if name in _done:
        return _done[name]
    src, kind = SOURCES[name]
    src = os.path.join(ROOT, src)
    os.makedirs(BIN_DIR, exist_ok=True)
    exe = os.path.join(BIN_DIR, name)
    if kind == "plain":
        # (-ffp-contract=off as csrc/Makefile: the tables of vfh_tables_dump are compared bit for bit)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-pthread", src, "-o", exe])
    elif kind == "host":
        native()
        subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wno-reorder", src, "-o", exe, "-L" + LIB_DIR, "-lrna", "-L" + ORACLE_DIR,
                               "-lrna_oracle", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath," + ORACLE_DIR, "-lm", "-lpthread"])
    elif kind == "rccl":
        native()
        subprocess.check_call([HIPCC, "-O1", "-std=c++17", src, "-o", exe, "-L" + LIB_DIR, "-lrna_rccl", "-lrna", "-L/opt/rocm/lib", "-lrccl",
                               "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])
    else:
        raise ValueError(kind)
    _done[name] = exe
    return exe


# ---- kernel resources ----
commands = {}     # source -> the last compile command run for it


def _compile(src, *extra):
    """runs the Makefile's own compile line for `src` (csrc/<name>.hip), its `-o <name>.o` replaced by `extra`"""
    obj = src[:-len(".hip")] + ".o"
    dry = subprocess.run(["make", "-n", "-B", "-C", CSRC, obj], capture_output=True, text=True)
    assert dry.returncode == 0, dry.stderr[-2000:]
    lines = [shlex.split(l) for l in dry.stdout.splitlines() if l.rstrip().endswith(" -c %s -o %s" % (src, obj))]
    assert len(lines) == 1, dry.stdout
    commands[src] = lines[0][:-2] + list(extra)
    out = subprocess.run(commands[src], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return out


def resources(src):
    """{kernel: {"VGPRs", "AGPRs", "LDS", "ScratchSize"}} of csrc/`src` for gfx950, compiled once per session"""
    key = ("resources", src)
    if key not in _done:
        out = _compile(src, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage")
        res, name = {}, None
        for line in out.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                res[name] = {}
            for key_re in ("VGPRs", "AGPRs", r"LDS Size \[bytes/block\]", r"ScratchSize \[bytes/lane\]"):
                m = re.search(r"remark:\s+" + key_re + r": (\d+)", line)
                if m and name:
                    res[name][key_re.split(" ")[0]] = int(m.group(1))
        _done[key] = res
    return _done[key]


def device_asm(src):
    """the gfx950 assembly of csrc/`src` as text, compiled once per session"""
    key = ("asm", src)
    if key not in _done:
        _done[key] = _compile(src, "-S", "--cuda-device-only", "-o", "-").stdout
    return _done[key]


# ---- the header and the build files ----
def c_values(tmp_path, body):
    """the integers a C99 program prints whose main() is `body`, compiled against include/rna.h"""
    src, exe = tmp_path / "values.c", tmp_path / "values"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rna.h"\nint main(void) {\n%s\n  return 0;\n}\n' % body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + INCLUDE, str(src), "-o", str(exe)])
    return [int(v) for v in subprocess.check_output([str(exe)]).split()]


def sources_in_build_files(name):
    """csrc/`name`.hip is compiled by the Makefile and by CMakeLists.txt"""
    assert re.search(r"^SRCS\s*:=.*\b%s\.hip\b" % name, open(os.path.join(CSRC, "Makefile")).read(), re.M)
    assert re.search(r"set\(RNA_SRCS[^)]*\b%s\b" % name, open(os.path.join(ROOT, "CMakeLists.txt")).read())
