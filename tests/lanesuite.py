"""What the CPU suites of the lane and wave routines share (test_walk_cpu, test_index_cpu, test_seek_cpu, test_seektab_cpu, test_seeksums_cpu,
test_seekmany_cpu, test_seekidx_cpu, test_scatter_cpu, test_dictfill_cpu, test_xxh64_cpu, test_xxh64_quad_cpu, test_entry_verdict_cpu): the build of a harness under
tests/emu/ (every one runs a routine of zstd-rs_amd/csrc over the accessors of tests/emu/zg_lane_mem.h) as a shared library and, where it has
a main, as a stand-alone AddressSanitizer program; the run of such a program; the fixture each suite's `built` is made of; two ctypes helpers.
The sanitizer's runtime is linked statically into a program with its own main: nothing is loaded into the interpreter."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstd-rs_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
FLAGS = ["-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-I", CSRC]
ASAN = ["-O1", "-g", "-fsanitize=address", "-static-libasan", "-fno-omit-frame-pointer"]
HOST_PARSE = ("zg_host_parse.cpp",)   # extra_sources of the harnesses that compare with the host's parse


def build(tmp, source, name, main_define=None, extra_sources=()):
    """tests/emu/<source> as <tmp>/lib<name>.so and, with main_define, as the program <tmp>/<name>_asan; (CDLL, program path or None)"""
    srcs = [os.path.join(EMU, source)] + [os.path.join(CSRC, s) for s in extra_sources]
    so, exe = os.path.join(str(tmp), "lib%s.so" % name), None
    subprocess.check_call(["g++", "-O2", *FLAGS, "-shared", "-fPIC", "-o", so, *srcs])
    if main_define:
        exe = os.path.join(str(tmp), name + "_asan")
        subprocess.check_call(["g++", *ASAN, "-D" + main_define, *FLAGS, "-o", exe, *srcs])
    return C.CDLL(so), exe


def run_stand_alone(exe, args, marker, timeout):
    """the program as a child process: it ends with 0, says `marker` and AddressSanitizer says nothing; its stdout"""
    p = subprocess.run([exe, *[str(a) for a in args]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    assert marker in p.stdout and b"AddressSanitizer" not in p.stderr, p.stderr.decode()[-4000:]
    return p.stdout


def built_fixture(source, name, main_define=None, extra_sources=(), declare=None):
    """a module-scoped fixture: build() into a temporary directory of its own, then declare(L) for the suite's argtypes. Its value is the
    library where the harness has no program, else (library, program path, directory). A suite that borrows another suite's fixture gets
    what that suite built: one build per harness and session."""
    @pytest.fixture(scope="module")
    def built(tmp_path_factory):
        if name not in _BUILT:
            d = tmp_path_factory.mktemp(name)
            L, exe = build(d, source, name, main_define, extra_sources)
            if declare:
                declare(L)
            _BUILT[name] = (L, exe, d) if main_define else L
        return _BUILT[name]
    return built


_BUILT = {}


def exact_buffer(data):
    """a ctypes buffer of exactly len(data) bytes (create_string_buffer alone appends a NUL)"""
    return C.create_string_buffer(data, len(data))


def aligned_copy(data):
    """(buffer, address): data at a 16-byte aligned address, as entries lie in device memory; the buffer keeps it alive"""
    buf = C.create_string_buffer(len(data) + 32)
    at = C.addressof(buf) + (-C.addressof(buf)) % 16
    C.memmove(at, data, len(data))
    return buf, at
