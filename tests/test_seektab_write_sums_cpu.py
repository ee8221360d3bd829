"""zgt::write_seek_table_sums (zstd-rs_amd/csrc/zg_seektab.h), the serialiser behind zgpu_seek_index_export_seek_table_ex with
ZGPU_EXPORT_CHECKSUMS, without a GPU: a harness (tests/emu/zg_lane_seektab_write_sums.cpp over tests/emu/zg_lane_mem.h, built by
tests/lanesuite.py) writes every case into a guarded block of exactly 17 + 12 * nrows bytes, once as a shared library and once as
lanesuite's stand-alone AddressSanitizer program (its own main: nothing is loaded into the interpreter). What it wrote must be
zgpu.seek_table_frame(csizes, dsizes, checksums=sums) byte for byte — rows of 12 bytes, Frame_Size = 12 * nrows + 9, descriptor 0x80 —, and
a c or d above 0xFFFFFFFF is ZGPU_E_SEEK_TABLE with nothing written."""
import ctypes as C
import os
import random
import struct

import pytest

import lanesuite
import zgpu

E_SEEK_TABLE = 72


def _cases():
    """(name, csizes, dsizes, sums, refused)"""
    rng = random.Random(0x5EE8)

    def rows(n):
        return ([rng.randrange(0, 1 << 20) for _ in range(n)], [rng.choice((0, 1, rng.randrange(0, 1 << 22))) for _ in range(n)],
                [rng.getrandbits(32) for _ in range(n)])
    out = [("rows_%d" % n,) + rows(n) + (False,) for n in (0, 1, 64, 65)]
    out.append(("row_u32_max", [5, 0xFFFFFFFF], [0xFFFFFFFF, 7], [0xFFFFFFFF, 0], False))
    out.append(("c_past_u32", [5, 0x100000000, 6], [1, 2, 3], [1, 2, 3], True))
    out.append(("d_past_u32", [5, 6], [1, 0x100000000], [1, 2], True))
    return out


def _case_bytes(cs, ds, sums):
    C_, D_ = [0], [0]
    for c, d in zip(cs, ds):
        C_.append(C_[-1] + c)
        D_.append(D_[-1] + d)
    return (struct.pack("<I", len(cs)) + b"".join(struct.pack("<QQ", c, d) for c, d in zip(C_, D_)) +
            struct.pack("<%dI" % len(sums), *sums))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("seektab_write_sums")
    L, asan = lanesuite.build(d, "zg_lane_seektab_write_sums.cpp", "seektab_write_sums", "SEEKTAB_WRITE_SUMS_MAIN")
    L.stws_run.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint32)]
    return d, L, asan


@pytest.mark.parametrize("which", ["library", "asan"])
def test_checksummed_serialiser_equals_seek_table_frame(programs, which):
    d, L, asan = programs
    cases = _cases()
    src, dst = os.path.join(str(d), "cases.bin"), os.path.join(str(d), "out_%s.bin" % which)
    with open(src, "wb") as f:
        f.write(b"".join(_case_bytes(cs, ds, sums) for _, cs, ds, sums, _ in cases))
    if which == "library":
        n = C.c_uint32(0)
        assert L.stws_run(src.encode(), dst.encode(), C.byref(n)) == 0 and n.value == len(cases)
    else:
        lanesuite.run_stand_alone(asan, [src, dst], b"seektab_write_sums ok: %d cases" % len(cases), 120)
    got, at = open(dst, "rb").read(), 0
    for name, cs, ds, sums, refused in cases:
        st, untouched, n = struct.unpack_from("<IIQ", got, at)
        body = got[at + 16:at + 16 + n]
        at += 16 + n
        if refused:
            assert (st, untouched, n) == (E_SEEK_TABLE, 1, 0), name
            continue
        want = zgpu.seek_table_frame(cs, ds, checksums=sums)
        assert st == 0 and n == 17 + 12 * len(cs) == len(want) and body == want, name
        assert struct.unpack_from("<I", body, 4)[0] == 12 * len(cs) + 9 and body[-5] == 0x80, name
        assert not untouched
    assert at == len(got)
