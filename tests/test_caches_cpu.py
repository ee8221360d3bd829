"""The two process-wide caches behind the streaming decoders (zstd-rs_amd/csrc/zg_caches.h: pinned host blocks, idle engines) under eight
holder threads and a trimming thread, as a stand-alone program under ThreadSanitizer (tests/emu/zg_emu_caches.cpp, which lists what it
holds): the templates the product instantiates with the HIP runtime's pinned memory and its engine, here over a counting allocator. Nothing
is loaded into the interpreter."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_caches_stand_alone_under_thread_sanitizer(tmp_path):
    d = os.path.join(HERE, "emu")
    subprocess.check_call(["make", "-C", d, "-s", "caches_tsan", "OUT=" + str(tmp_path)])
    p = subprocess.run([str(tmp_path / "caches_tsan")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, (p.stdout.decode()[-2000:], err[-4000:])
    assert b"caches ok" in p.stdout
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]


def test_the_product_instantiates_the_tested_templates():
    """zg_stream.cpp holds no cache of its own: its two globals are the header's templates"""
    src = open(os.path.join(os.path.dirname(HERE), "zstd-rs_amd", "csrc", "zg_stream.cpp")).read()
    assert '#include "zg_caches.h"' in src and "PinnedCache<HipHostMem> g_pinned;" in src and "IdleEngines<Engine> g_idle_engines;" in src
    assert "struct PinnedCache" not in src and "struct IdleEngines" not in src
