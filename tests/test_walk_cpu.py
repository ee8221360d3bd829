"""zg_k_walk's lane routine (zstd-rs_amd/csrc/zg_walk.h) and the host's parse of its skeleton records (zg_host_parse.cpp), compiled with g++ and
run on the CPU: for every input the lane runs twice, count pass and emit pass, over a reader that counts every access outside [0, len) and a
writer that counts every store outside the lane's own record range (which lies between guard records); then parse_frames_skel and
plaintext_bound_skel over the records must give exactly what parse_frames and plaintext_bound give over the bytes — the walk status, the
bound, every FrameInfo field, the BatchBuilder's blocks and frames byte for byte after finish(), and its counters. The corpus: every golden
frame, the seqframes families, hand-built frames at the section headers' edges, every prefix (of the first 4 KiB), fixed-seed single-byte
edits aimed at the headers, concatenations with skippable frames, the empty input. tests/emu/zg_lane_walk.cpp is the harness, built by tests/lanesuite.py. And
zgpu_decode_frames_device_src's argument rules."""
import ctypes as C
import os
import struct

import lanesuite
import seqframes
from golden_io import GOLDEN_DIR, read_pack

MAX_WINDOW = 128 << 20          # the engine's default (frame_decoder.rs:25)
MAGIC = struct.pack("<I", 0xFD2FB528)


def _declare(L):
    u64, vp = C.c_uint64, C.c_void_p
    L.wk_check.argtypes = [vp, u64, u64]
    L.wk_check.restype = C.c_uint32
    L.wk_prefixes.argtypes = [vp, u64, u64, u64, C.POINTER(u64)]
    L.wk_prefixes.restype = C.c_uint32
    L.wk_edits.argtypes = [vp, u64, u64, u64, u64, C.POINTER(u64), C.POINTER(u64)]
    L.wk_edits.restype = C.c_uint32
    L.wk_coverage.argtypes = [C.POINTER(u64)] * 6


lib = lanesuite.built_fixture("zg_lane_walk.cpp", "walk_lane", extra_sources=lanesuite.HOST_PARSE, declare=_declare)


def block(body, btype=2, last=True, size=None):
    """a block header + body; size: the Block_Size field when it is not len(body) (RLE blocks, lies)"""
    n = len(body) if size is None else size
    return struct.pack("<I", (n << 3) | (btype << 1) | (1 if last else 0))[:3] + body


def frame(blocks, checksum=None, window=0x00):
    """a frame with a Window_Descriptor and no content size; checksum: 4 bytes behind the last block"""
    return MAGIC + bytes([0x04 if checksum is not None else 0x00, window]) + b"".join(blocks) + (checksum or b"")


def skippable(payload, magic=0x184D2A50, length=None):
    return struct.pack("<II", magic, len(payload) if length is None else length) + payload


def hand_built():
    """frames at the edges of the two section headers and of the frame layer (the host's verdicts only: nothing here is decoded)"""
    out = {}
    out["seq_header_missing"] = frame([block(b"\x00")])                               # raw literals of 0 bytes fill the block: SequencesHeader
    out["seq_extra_bits"] = frame([block(b"\x00\x00\x00")])                            # 0 sequences and bytes behind them
    out["seq_none"] = frame([block(b"\x00\x00")])
    out["seq_1byte"] = frame([block(b"\x00\x05\x00\x00")], checksum=b"\x01\x02\x03\x04")
    out["seq_1byte_short"] = frame([block(b"\x00\x05")])
    out["seq_2byte"] = frame([block(b"\x00\x80\x01\x00\x00")])
    out["seq_2byte_zero"] = frame([block(b"\x00\x80\x00")])
    out["seq_2byte_short"] = frame([block(b"\x00\x80\x01")])
    out["seq_3byte"] = frame([block(b"\x00\xff\x01\x00\x00\x00")])
    out["seq_3byte_short"] = frame([block(b"\x00\xff\x01\x00")])
    out["lit_treeless_first"] = frame([block(b"\x03\x00\x00\x00")])                    # Treeless with no table: UninitializedHuffmanTable
    out["lit_leaves_block"] = frame([block(b"\x50\x00")])                              # 10 raw literals in a block of 2: MalformedSectionHeader
    out["lit_header_empty"] = frame([block(b"")])
    out["lit_header_short"] = frame([block(b"\x04")])                                  # a 2-byte header, 1 byte there
    out["lit_raw_2byte"] = frame([block(b"\x24\x00" + b"ab" + b"\x00")])
    out["lit_raw_3byte"] = frame([block(b"\x2c\x00\x00" + b"ab" + b"\x00")])
    out["lit_rle_1byte"] = frame([block(b"\x29" + b"z" + b"\x00")])
    out["lit_huf_sf0"] = frame([block(b"\x02\x40\x00" + b"q" + b"\x00")])               # compressed size 1, one stream
    out["lit_huf_sf1"] = frame([block(b"\x06\x40\x00" + b"q" + b"\x00")])
    out["lit_huf_sf2"] = frame([block(b"\x0a\x00\x04\x00" + b"q" + b"\x00")])
    out["lit_huf_sf3"] = frame([block(b"\x0e\x00\x40\x00\x00" + b"q" + b"\x00")])
    out["raw_rle_blocks"] = frame([block(b"abc", btype=0, last=False), block(b"x", btype=1, size=77)], checksum=b"\x00\x00\x00\x00")
    out["reserved_block"] = frame([block(b"abc", btype=3)])
    out["block_too_large"] = frame([block(b"abc", btype=2, size=(128 << 10) + 1)])
    out["block_max_rle"] = frame([block(b"x", btype=1, size=128 << 10)])
    out["body_past_end"] = frame([block(b"abc", btype=0, size=9)])
    out["checksum_short"] = frame([block(b"abc", btype=0)], checksum=b"\x01\x02")
    out["no_last_block"] = frame([block(b"abc", btype=0, last=False)])
    out["window_too_big_spec"] = frame([block(b"abc", btype=0)], window=0xFF)
    out["window_over_max"] = frame([block(b"abc", btype=0)], window=0xB0)             # 2^32: beyond the 128 MiB the decoder allows
    out["dict_frame"] = MAGIC + bytes([0x01, 0x00, 0x07]) + block(b"abc", btype=0, last=False) + block(b"\x00\x00") + b"tail"
    out["single_segment_fcs8"] = MAGIC + bytes([0xE0]) + struct.pack("<Q", 3) + block(b"abc", btype=0)
    out["fcs2_dict4"] = MAGIC + bytes([0x43, 0x00]) + struct.pack("<IH", 0, 3) + block(b"abc", btype=0)   # dictionary id 0 means none
    out["bad_magic"] = b"\x28\xb5\x2f\xfc" + b"\x00" * 20
    out["empty"] = b""
    good = out["raw_rle_blocks"]
    out["skip_then_frame"] = skippable(b"hello") + good
    out["frame_skip_frame"] = good + skippable(b"", magic=0x184D2A5F) + out["seq_1byte"] + skippable(b"xyz")
    out["skip_only"] = skippable(b"abc") + skippable(b"")
    out["skip_past_end"] = good + skippable(b"abc", length=4)
    out["skip_huge"] = skippable(b"abc", length=0xFFFFFFFF)
    out["skip_header_short"] = good + struct.pack("<I", 0x184D2A50) + b"\x01\x00"
    out["frames_then_garbage"] = good + good + b"\x00\x01\x02\x03\x04\x05"
    out["defect_then_frame"] = out["seq_extra_bits"] + good                             # the lane walks on where the host's walk has stopped
    return out


def corpus():
    out = []
    for pack in sorted(f for f in os.listdir(GOLDEN_DIR) if f.endswith(".pack")):
        for name, z in sorted(read_pack(pack).items()):
            if name.endswith(".zst") or pack == "fuzz_artifacts.pack":
                out.append((pack + ":" + name, z))
    for sub in ("regress", "verdict_order"):
        for f in sorted(os.listdir(os.path.join(GOLDEN_DIR, sub))):
            if f.endswith(".zst"):
                out.append((sub + ":" + f, open(os.path.join(GOLDEN_DIR, sub, f), "rb").read()))
    for fam, name, z, _ in seqframes.all_frames():
        out.append(("seqframes:" + fam + ":" + name, z))
    hb = hand_built()
    out += [("hand:" + k, v) for k, v in sorted(hb.items())]
    # concatenations: golden frames with skippable frames between them, a frame behind a dictionary frame
    fx = read_pack("decodecorpus.pack")
    names = sorted(n for n in fx if n.endswith(".zst"))[:6]
    out.append(("concat:golden+skip", b"".join(fx[n] + skippable(bytes([i]) * i) for i, n in enumerate(names))))
    out.append(("concat:golden+skip_past_end", fx[names[0]] + skippable(b"", length=1)))
    out.append(("concat:dict+golden", hb["dict_frame"][:-4] + fx[names[1]]))
    return out


def test_skeleton_parse_equals_byte_parse_everywhere(lib):
    where, nedits = C.c_uint64(0), C.c_uint64(0)
    total_edits = 0
    cases = corpus()
    assert len(cases) > 300
    for seed, (name, z) in enumerate(cases):
        buf = lanesuite.exact_buffer(z)
        assert lib.wk_check(buf, len(z), MAX_WINDOW) == 0, name
        assert lib.wk_check(buf, len(z), 1 << 41) == 0, name
        bad = lib.wk_prefixes(buf, len(z), 4096, MAX_WINDOW, C.byref(where))
        assert bad == 0, (name, "prefix", where.value, bad)
        bad = lib.wk_edits(buf, len(z), MAX_WINDOW, 0x5EED + seed, 400, C.byref(where), C.byref(nedits))
        assert bad == 0, (name, "edit at", where.value, bad)
        assert buf.raw == z
        total_edits += nedits.value
    assert total_edits > 20000
    # what the set reached
    u64 = C.c_uint64
    status, why, lit, seq, ck, n = (u64 * 256)(), (u64 * 16)(), (u64 * 8)(), (u64 * 4)(), (u64 * 2)(), u64(0)
    lib.wk_coverage(status, why, lit, seq, ck, C.byref(n))
    assert n.value > 100000
    # every status parse_frames can return (WindowTooSmall cannot happen with a 10-bit base, MissingMode and Internal not in a walk that
    # stops at the first defect): ok, BadMagic, HeaderRead, WindowTooBig, WindowSizeTooBig, DictNotProvided, block header / body / checksum
    # not read, FailedSkipFrame, ReservedBlock, BlockSizeTooLarge, MalformedSectionHeader, LiteralsHeader, SequencesHeader,
    # UninitializedHuffmanTable, ExtraBits
    for st in (0, 2, 3, 4, 6, 7, 9, 10, 11, 13, 20, 21, 22, 23, 24, 30, 47):
        assert status[st] > 0, ("status never reached", st)
    assert all(why[k] > 0 for k in range(9)), list(why)[:9]     # every reason a lane stops for
    # every literals size format in frames the walk accepts: Raw / RLE with 1-, 2- and 3-byte headers (size formats 0 and 2 are both the
    # 1-byte form), Compressed / Treeless with each of the four
    raw, huf = list(lit)[:4], list(lit)[4:]
    assert raw[0] + raw[2] > 0 and raw[0] > 0 and raw[2] > 0 and raw[1] > 0 and raw[3] > 0, raw
    assert all(x > 0 for x in huf), huf
    assert all(x > 0 for x in seq), list(seq)                   # 0 sequences, the 1-, 2- and 3-byte counts
    assert ck[0] > 0 and ck[1] > 0, list(ck)                    # a last block without and with a checksum behind it


def test_device_src_argument_rules_need_no_gpu():
    import zgpu
    L = zgpu.load_library()
    n = 1
    srcs, lens = (C.c_void_p * n)(), (C.c_size_t * n)()
    dsts, caps = (C.c_void_p * n)(), (C.c_size_t * n)()
    res = (zgpu.DeviceEntryResultC * n)()
    opts = zgpu.DeviceOptsC(0, 0, 0)
    assert L.zgpu_decode_frames_device_src(None, srcs, lens, n, dsts, caps, C.byref(opts), res) == 93     # ZGPU_E_BAD_ARG, no GPU touched
    assert L.zgpu_decode_frames_device_src(None, None, None, 0, None, None, None, None) == 93
    fake = C.create_string_buffer(4096)   # null arrays with n > 0: refused before the context is looked at (this one is not a context)
    for k in range(5):
        a = [srcs, lens, dsts, caps, res]
        a[k] = None
        assert L.zgpu_decode_frames_device_src(fake, a[0], a[1], n, a[2], a[3], None, a[4]) == 93, k
    out = (C.c_uint64 * 6)()
    assert L.zgpu_debug_frames_device_src_stats(None, out, 6) == 0
    for sym in ("zgpu_decode_frames_device_src", "zgpu_debug_frames_device_src_stats"):
        assert sym in zgpu.EXPORTS and hasattr(L, sym)
    for dev in (False, True):
        lib_ = zgpu.load_library(dev=dev)
        for sym in zgpu.EXPORTS:
            assert hasattr(lib_, sym), sym
    for m in ("decode_frames_device_src", "decode_tensors", "frames_device_src_stats"):
        assert hasattr(zgpu.Context, m)
