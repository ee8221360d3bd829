"""zg_k_walk's lane routine (zstd-rs_amd/csrc/zg_walk.h) and the host's parse of its skeleton records (zg_host_parse.cpp), compiled with g++ and
run on the CPU: for every input the lane runs twice, count pass and emit pass, over a reader that counts every access outside [0, len) and a
writer that counts every store outside the lane's own record range (which lies between guard records); then parse_frames_skel and
plaintext_bound_skel over the records must give exactly what parse_frames and plaintext_bound give over the bytes — the walk status, the
bound, every FrameInfo field, the BatchBuilder's blocks and frames byte for byte after finish(), and its counters. The corpus: every golden
frame, the seqframes families, hand-built frames at the section headers' edges, every prefix (of the first 4 KiB), fixed-seed single-byte
edits aimed at the headers, concatenations with skippable frames, the empty input. And zgpu_decode_frames_device_src's argument rules."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import seqframes
from golden_io import GOLDEN_DIR, read_pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstd-rs_amd", "csrc")
HARNESS = r'''
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zg_host_parse.h"
using namespace zg;
namespace {
struct Count { uint64_t bad_reads = 0, bad_writes = 0, written = 0; };
struct Reader {   // the entry as a lane may see it: bytes [0, len), nothing else
  const uint8_t* p; uint64_t len; Count* c;
  uint8_t ld1(uint64_t off) const { if (off >= len) { c->bad_reads++; return 0; } return p[off]; }
};
struct Writer {   // the lane's record range [lo, hi) of recs
  zgw::Rec* recs; uint64_t lo, hi; Count* c;
  void put(uint64_t i, const zgw::Rec& x) const { if (i < lo || i >= hi) { c->bad_writes++; return; } recs[i] = x; c->written++; }
};
constexpr uint64_t kGuard = 4, kBase = 64;
// coverage, over every input checked so far
uint64_t g_status[256], g_why[16], g_lit[2][4], g_seq[4], g_cksum[2], g_cases;

bool same_info(const FrameInfo& a, const FrameInfo& b) {
  return a.header.descriptor == b.header.descriptor && a.header.window_descriptor == b.header.window_descriptor &&
         a.header.has_dict_id == b.header.has_dict_id && a.header.dict_id == b.header.dict_id &&
         a.header.frame_content_size == b.header.frame_content_size && a.header.header_size == b.header.header_size &&
         a.window_size == b.window_size && a.src_begin == b.src_begin && a.src_end == b.src_end && a.has_checksum == b.has_checksum &&
         a.checksum == b.checksum && a.nblocks == b.nblocks && a.host_status == b.host_status;
}

// one input: 0 if everything agrees, else a bit per kind of disagreement
uint32_t check(const uint8_t* data, uint64_t len, uint64_t max_window) {
  uint32_t bad = 0;
  Count c;
  const uint8_t* own = data;
  const Reader r{own, len, &c};
  const Writer none{nullptr, 0, 0, &c};
  const zgw::End e0 = zgw::walk_entry<false>(r, none, len, 0, 0);
  if (c.written || c.bad_writes) bad |= 1u;
  std::vector<zgw::Rec> recs(e0.nrec + 2 * kGuard);
  memset(recs.data(), 0xEE, recs.size() * sizeof(zgw::Rec));
  const Writer w{recs.data(), kGuard, kGuard + e0.nrec, &c};
  const zgw::End e1 = zgw::walk_entry<true>(r, w, len, kGuard, e0.nrec);
  if (e1.nrec != e0.nrec || e1.why != e0.why || e1.stop_off != e0.stop_off) bad |= 2u;
  if (c.written != e0.nrec) bad |= 4u;                      // the emit pass writes exactly the count pass's number of records
  if (c.bad_reads) bad |= 8u;
  if (c.bad_writes) bad |= 16u;
  for (uint64_t g = 0; g < kGuard; g++) {
    const uint8_t* a = (const uint8_t*)&recs[g];
    const uint8_t* b = (const uint8_t*)&recs[kGuard + e0.nrec + g];
    for (size_t k = 0; k < sizeof(zgw::Rec); k++) if (a[k] != 0xEE || b[k] != 0xEE) bad |= 16u;
  }
  if (e0.stop_off > len || (e0.why == zgw::kEnd && e0.stop_off != len)) bad |= 32u;
  if (e0.nrec > 1) {   // a lane whose range is shorter than its records (a source that changed between the passes) still stays inside it
    Count c2;
    std::vector<zgw::Rec> few(e0.nrec - 1 + 2 * kGuard);
    const Writer w2{few.data(), kGuard, kGuard + e0.nrec - 1, &c2};
    (void)zgw::walk_entry<true>(Reader{own, len, &c2}, w2, len, kGuard, e0.nrec - 1);
    if (c2.bad_writes || c2.bad_reads || c2.written != e0.nrec - 1) bad |= 16u;
  }
  const zgw::Rec* sk = recs.data() + kGuard;
  BatchBuilder a, b;
  std::vector<FrameInfo> ia, ib;
  bool ok1 = false, ok2 = false;
  const int sa = parse_frames(data, len, max_window, &a, &ia, kBase);
  const int sb = parse_frames_skel(sk, e0.nrec, len, max_window, &b, &ib, kBase, &ok1);
  if (sa != sb) bad |= 64u;
  if (!ok1) bad |= 128u;
  const uint64_t pa = plaintext_bound(data, len), pb = plaintext_bound_skel(sk, e0.nrec, len, &ok2);
  if (pa != pb) bad |= 256u;
  if (!ok2) bad |= 512u;
  if (ia.size() != ib.size()) bad |= 1024u;
  else for (size_t i = 0; i < ia.size(); i++) if (!same_info(ia[i], ib[i])) bad |= 1024u;
  a.finish(); b.finish();
  if (a.blocks.size() != b.blocks.size() || (a.blocks.size() && memcmp(a.blocks.data(), b.blocks.data(), a.blocks.size() * sizeof(ZgBlock)))) bad |= 2048u;
  if (a.frames.size() != b.frames.size() || (a.frames.size() && memcmp(a.frames.data(), b.frames.data(), a.frames.size() * sizeof(ZgFrame)))) bad |= 4096u;
  if (a.lit_bytes != b.lit_bytes || a.seq_count != b.seq_count || a.out_bound != b.out_bound || a.nhuf_slots != b.nhuf_slots) bad |= 8192u;
  // coverage
  g_cases++;
  g_status[sa & 255]++;
  g_why[e0.why & 15]++;
  if (sa == 0) {   // formats are counted in inputs the host's walk accepts from end to end
    for (uint32_t k = 0; k < e0.nrec; k++) {
      const zgw::Rec& x = sk[k];
      if (x.kind != zgw::kBlock || ((x.b[0] >> 1) & 3) != 2 || !x.have) continue;
      g_lit[(x.b[3] & 3) >= 2][(x.b[3] >> 2) & 3]++;
      if (x.have2) g_seq[x.b[8] == 0 ? 0 : x.b[8] < 128 ? 1 : x.b[8] < 255 ? 2 : 3]++;
    }
    for (const FrameInfo& f : ia) g_cksum[f.has_checksum]++;
  }
  return bad;
}
}  // namespace

extern "C" uint32_t wk_check(const uint8_t* data, uint64_t len, uint64_t max_window) { return check(data, len, max_window); }
// every prefix of the first `upto` bytes; returns the first failing length + 1 in *where
extern "C" uint32_t wk_prefixes(const uint8_t* data, uint64_t len, uint64_t upto, uint64_t max_window, uint64_t* where) {
  const uint64_t n = len < upto ? len : upto;
  for (uint64_t k = 0; k <= n; k++) { const uint32_t bad = check(data, k, max_window); if (bad) { *where = k; return bad; } }
  return 0;
}
// single-byte edits at the bytes the host reads: frame headers, block headers, the first 5 body bytes and the 4 at the sequences section
// header of every block, each set to 0x00, 0xFF, one flipped bit and one random value (fixed seed); at most `budget` positions per input,
// evenly spread
extern "C" uint32_t wk_edits(uint8_t* data, uint64_t len, uint64_t max_window, uint64_t seed, uint64_t budget, uint64_t* where, uint64_t* nedits) {
  BatchBuilder bb;
  std::vector<FrameInfo> info;
  (void)parse_frames(data, len, 1ull << 62, &bb, &info, 0);
  std::vector<uint64_t> pos;
  for (const FrameInfo& f : info) for (uint64_t k = 0; k < f.header.header_size + 3u; k++) pos.push_back(f.src_begin + k);
  for (const ZgBlock& b : bb.blocks) {
    if (b.src_off < 3) continue;
    for (uint64_t k = 0; k < 3; k++) pos.push_back(b.src_off - 3 + k);
    if (b.btype != ZG_BT_COMPRESSED) continue;
    for (uint64_t k = 0; k < 5 && k < b.src_len; k++) pos.push_back(b.src_off + k);
    uint32_t at = 0, avail = 0;
    uint8_t head[5] = {0, 0, 0, 0, 0};
    memcpy(head, data + b.src_off, b.src_len < 5 ? b.src_len : 5);
    if (zgw::seq_header_at(head, b.src_len, &at, &avail)) for (uint64_t k = 0; k < avail; k++) pos.push_back(b.src_off + at + k);
  }
  uint64_t x = seed * 6364136223846793005ull + 1442695040888963407ull;
  const uint64_t step = pos.size() > budget ? (pos.size() + budget - 1) / budget : 1;
  *nedits = 0;
  for (uint64_t q = 0; q < pos.size(); q += step) {
    const uint64_t p = pos[q];
    if (p >= len) continue;
    const uint8_t keep = data[p];
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    const uint8_t vals[4] = {0x00, 0xFF, (uint8_t)(keep ^ (1u << ((x >> 33) & 7))), (uint8_t)(x >> 41)};
    for (uint8_t v : vals) {
      if (v == keep) continue;
      data[p] = v;
      const uint32_t bad = check(data, len, max_window);
      (*nedits)++;
      if (bad) { *where = p; data[p] = keep; return bad; }
    }
    data[p] = keep;
  }
  return 0;
}
extern "C" void wk_coverage(uint64_t* status, uint64_t* why, uint64_t* lit, uint64_t* seq, uint64_t* cksum, uint64_t* cases) {
  memcpy(status, g_status, sizeof g_status); memcpy(why, g_why, sizeof g_why); memcpy(lit, g_lit, sizeof g_lit);
  memcpy(seq, g_seq, sizeof g_seq); memcpy(cksum, g_cksum, sizeof g_cksum); *cases = g_cases;
}
'''
MAX_WINDOW = 128 << 20          # the engine's default (frame_decoder.rs:25)
MAGIC = struct.pack("<I", 0xFD2FB528)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk")
    src, so = d / "walk_lane.cpp", d / "libwalk_lane.so"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src),
                           os.path.join(CSRC, "zg_host_parse.cpp")])
    L = C.CDLL(str(so))
    u64, vp = C.c_uint64, C.c_void_p
    L.wk_check.argtypes = [vp, u64, u64]
    L.wk_check.restype = C.c_uint32
    L.wk_prefixes.argtypes = [vp, u64, u64, u64, C.POINTER(u64)]
    L.wk_prefixes.restype = C.c_uint32
    L.wk_edits.argtypes = [vp, u64, u64, u64, u64, C.POINTER(u64), C.POINTER(u64)]
    L.wk_edits.restype = C.c_uint32
    L.wk_coverage.argtypes = [C.POINTER(u64)] * 6
    return L


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
        buf = C.create_string_buffer(z, len(z))
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
