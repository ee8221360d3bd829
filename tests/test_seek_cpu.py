"""zg_k_seek's lane routine (zstd-rs_amd/csrc/zg_seek.h), compiled with g++ and run on the CPU. For every input and every range the routine
runs over a reader that counts every access outside [anchor_src, len) and every access to a byte of a block body (the bodies as
zgw::walk_entry's records give them), and every field of its record is compared with a model computed from zgi::index_entry<true>'s frame
records and frame_fields — existing code, not the routine under test. Demanded of every case:
  - reads outside [anchor_src, len) 0, reads of a block body 0;
  - the record equals the model's, field for field;
  - bound == plaintext_bound(bytes[src_lo:src_hi]);
  - [src_lo, src_hi) starts and ends on frame-record boundaries (src_hi == len where the chain broke);
  - a run anchored at a frame boundary in front of the selection gives the src_lo / src_hi / plain_lo / flags of the unanchored one, with
    nblocks no larger.
Ranges per input: begin at 0, at every frame's declared boundary - 1, + 0, + 1, at the declared total and at the total + 5; len 1, 2, to the
end, 2^63 (and 0, which must read nothing). Each range runs unanchored and anchored at every frame boundary at which an anchor is valid: in
front of begin with every frame in front of it skipped by the unanchored run (a boundary behind an unsized or a taken frame is no anchor:
anchor_plain would not be known, or would lie behind begin).
The corpus is tests/test_walk_cpu.py's and concatenations of 2-6 of its inputs with skippable frames between them. The same ranges run once
more in a stand-alone AddressSanitizer program (its own main, no Python in the process) in which every entry lies in a heap block of exactly
its length."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

import zgpu
from test_walk_cpu import MAGIC, block, corpus, hand_built, skippable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstd-rs_amd", "csrc")
HARNESS = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zg_host_parse.h"
#include "zg_seek.h"
using namespace zg;
namespace {
struct Count { uint64_t bad_reads = 0, body_reads = 0; };
struct Reader {   // the entry as a lane may see it: bytes [lo, len), and none that belongs to a block body
  const uint8_t* p; uint64_t lo, len; const uint8_t* body; Count* c;
  uint8_t ld1(uint64_t off) const {
    if (off < lo || off >= len) { c->bad_reads++; return 0; }
    if (body && body[off]) c->body_reads++;
    return p[off];
  }
};
struct NoCount { uint8_t ld1(uint64_t off) const { return p[off]; } const uint8_t* p; };
struct WalkWriter { zgw::Rec* recs; void put(uint64_t i, const zgw::Rec& x) const { recs[i] = x; } };
struct RecWriter { zgi::FrameRec* recs; void put(uint64_t i, const zgi::FrameRec& x) const { recs[i] = x; } };
// [0] cases [1] open-ended [2] the chain broke in front of the range [3] it broke inside the selection [4] an empty frame at a boundary
// [5] bit 2 [6] anchored runs [7] ranges of length 0 [8] refused anchors
uint64_t g_cov[16];

bool same(const zgk::Seek& a, const zgk::Seek& b) {
  return a.src_lo == b.src_lo && a.src_hi == b.src_hi && a.plain_lo == b.plain_lo && a.bound == b.bound && a.plain_seen == b.plain_seen &&
         a.status == b.status && a.frames_skipped == b.frames_skipped && a.frames_taken == b.frames_taken && a.nblocks == b.nblocks &&
         a.why == b.why && a.flags == b.flags;
}
bool readable(const zgi::FrameRec& x) { FrameFields f; frame_fields(x.b, x.have, &f); return f.header_status == ZG_OK; }

// The rule of zg_seek.h over the frame records of the whole entry, from record `start` (the one that begins at anchor_src) on.
zgk::Seek model(const zgi::FrameRec* fr, uint32_t nrec, uint32_t ewhy, uint64_t len, uint64_t begin, uint64_t rlen, uint32_t start,
                uint64_t anchor_src, uint64_t anchor_plain, bool* empty_at_boundary, bool* broke_in_front) {
  zgk::Seek o;
  memset(&o, 0, sizeof o);
  if (!rlen) return o;
  if (anchor_src > len || anchor_plain > begin) { o.status = 93; return o; }
  const unsigned __int128 end = (unsigned __int128)begin + rlen;
  unsigned __int128 pos = anchor_plain;
  uint64_t lo = 0, plo = 0, hi = anchor_src;
  bool taken = false, open = false;
  uint32_t why = 0;
  const uint64_t top = ~0ull;
  for (uint32_t k = start; k < nrec; k++) {
    const zgi::FrameRec& x = fr[k];
    FrameFields f;
    frame_fields(x.b, x.have, &f);
    const bool z = f.header_status == ZG_OK, sized = (f.flags & 2u) != 0;
    o.nblocks += x.nblocks;
    hi = x.end;
    if (k + 1 == nrec && ewhy) {
      why = ewhy;
      if (!taken) { taken = true; lo = x.begin; plo = (uint64_t)pos; *broke_in_front = true; }
      if (z) { o.frames_taken++; o.bound += x.bound; }
      break;
    }
    if (!z) continue;
    if (!taken && sized && pos + f.frame_content_size <= begin) {
      if (f.frame_content_size == 0 && pos == begin) *empty_at_boundary = true;
      o.frames_skipped++; pos += f.frame_content_size;
      continue;
    }
    if (!taken) { taken = true; lo = x.begin; plo = (uint64_t)pos; }
    o.frames_taken++; o.bound += x.bound;
    if (sized) { pos += f.frame_content_size; if (pos > top) pos = top; } else open = true;
    if (!open && pos >= (end > top ? (unsigned __int128)top : end)) break;
  }
  o.src_lo = taken ? lo : hi; o.src_hi = why ? len : hi;
  o.plain_lo = taken ? plo : (uint64_t)pos; o.plain_seen = (uint64_t)pos;
  o.why = why;
  o.flags = (open ? 1u : 0u) | (why ? 2u : 0u) | (taken ? 0u : 4u);
  return o;
}

struct Input {
  const uint8_t* data; uint64_t len;
  zgi::Entry e;
  std::vector<zgi::FrameRec> fr;
  std::vector<uint8_t> body;
  std::vector<uint64_t> plain_at;   // declared plaintext offset at record k's begin (unsized frames count nothing)
  std::vector<uint8_t> sized_front; // every zstd frame in front of record k declares a size
};
void prepare(Input& in, bool bodies) {
  const NoCount nr{in.data};
  in.e = zgi::index_entry<false>(nr, RecWriter{nullptr}, in.len, 0, 0);
  in.fr.resize(in.e.nrec + 1);
  (void)zgi::index_entry<true>(nr, RecWriter{in.fr.data()}, in.len, 0, in.e.nrec);
  in.fr.resize(in.e.nrec);
  in.plain_at.assign(in.e.nrec + 1, 0);
  in.sized_front.assign(in.e.nrec + 1, 1);
  for (uint32_t k = 0; k < in.e.nrec; k++) {
    FrameFields f;
    frame_fields(in.fr[k].b, in.fr[k].have, &f);
    const bool z = f.header_status == ZG_OK, sized = (f.flags & 2u) != 0;
    uint64_t next = in.plain_at[k] + (z && sized ? f.frame_content_size : 0);
    if (next < in.plain_at[k]) next = ~0ull;
    in.plain_at[k + 1] = next;
    in.sized_front[k + 1] = in.sized_front[k] && (!z || sized);
  }
  if (!bodies) return;
  const zgw::End w0 = zgw::walk_entry<false>(nr, WalkWriter{nullptr}, in.len, 0, 0);
  std::vector<zgw::Rec> wrecs(w0.nrec + 1);
  (void)zgw::walk_entry<true>(nr, WalkWriter{wrecs.data()}, in.len, 0, w0.nrec);
  in.body.assign(in.len + 1, 0);
  for (uint32_t k = 0; k < w0.nrec; k++) {
    const zgw::Rec& x = wrecs[k];
    if (x.kind != zgw::kBlock) continue;
    const uint32_t type = (x.b[0] >> 1) & 3u, size = (uint32_t)(x.b[0] >> 3) | ((uint32_t)x.b[1] << 5) | ((uint32_t)x.b[2] << 13);
    if (type == 3 || size > zgw::kBlockMax) continue;
    const uint64_t n = type == 1 ? 1 : size;
    for (uint64_t q = x.off; q < x.off + n && q < in.len; q++) in.body[q] = 1;
  }
}
// every (begin, len) of the input, f(begin, len)
template <class F> void ranges(const Input& in, F f) {
  std::vector<uint64_t> begins{0};
  const uint64_t total = in.plain_at[in.e.nrec];
  for (uint32_t k = 0; k <= in.e.nrec; k++) for (int d = -1; d <= 1; d++) {
    const uint64_t b = in.plain_at[k];
    if (d < 0 && !b) continue;
    begins.push_back(b + (uint64_t)d);
  }
  begins.push_back(total); begins.push_back(total + 5);
  for (uint64_t b : begins) {
    const uint64_t lens[5] = {1, 2, total > b ? total - b : 0, 1ull << 63, 0};
    for (uint64_t l : lens) f(b, l);
  }
}

// one input: 0 if everything agrees, else a bit per kind of disagreement (*where: the begin of the range that disagreed)
uint32_t check(const uint8_t* data, uint64_t len, uint64_t* where) {
  Input in{data, len};
  prepare(in, true);
  const uint32_t nrec = in.e.nrec;
  uint32_t bad = 0;
  ranges(in, [&](uint64_t begin, uint64_t rlen) {
    if (bad) return;
    Count c;
    const zgk::Seek un = zgk::seek_entry(Reader{data, 0, len, in.body.data(), &c}, len, begin, rlen, 0, 0);
    bool empty = false, front = false;
    const zgk::Seek m = model(in.fr.data(), nrec, in.e.why, len, begin, rlen, 0, 0, 0, &empty, &front);
    if (!same(un, m)) bad |= 1u;
    if (c.bad_reads) bad |= 2u;
    if (c.body_reads) bad |= 4u;
    if (un.src_lo > un.src_hi || un.src_hi > len) bad |= 8u;
    else if (un.bound != plaintext_bound(data + un.src_lo, (size_t)(un.src_hi - un.src_lo))) bad |= 16u;
    g_cov[0]++;
    if (!rlen) { g_cov[7]++; zgk::Seek z; memset(&z, 0, sizeof z); if (!same(un, z) || c.bad_reads || c.body_reads) bad |= 32u; if (bad) *where = begin; return; }
    bool lo_ok = un.src_lo == len && !nrec, hi_ok = (un.flags & zgk::kBroken) ? un.src_hi == len : (un.src_hi == 0 && !nrec);
    for (uint32_t k = 0; k < nrec; k++) {
      if (in.fr[k].begin == un.src_lo || in.fr[k].end == un.src_lo) lo_ok = true;
      if (in.fr[k].begin == un.src_hi || in.fr[k].end == un.src_hi) hi_ok = true;
    }
    if (!lo_ok || !hi_ok) bad |= 64u;
    if (un.flags & zgk::kOpenEnded) g_cov[1]++;
    if ((un.flags & zgk::kBroken) && front && un.frames_skipped) g_cov[2]++;
    if ((un.flags & zgk::kBroken) && !front) g_cov[3]++;
    if (empty) g_cov[4]++;
    if (un.flags & zgk::kNothing) g_cov[5]++;
    // anchored at every boundary in front of the selection
    for (uint32_t k = 1; k <= nrec && !bad; k++) {
      const uint64_t at = k < nrec ? in.fr[k].begin : in.fr[nrec - 1].end;
      if (k == nrec && (in.e.why || at != len)) continue;
      if (k < nrec && in.fr[k].begin == in.fr[k].end && k + 1 == nrec && in.fr[k - 1].end != at) continue;
      if (!in.sized_front[k] || at > un.src_lo || in.plain_at[k] > begin) continue;
      Count c2;
      const zgk::Seek an = zgk::seek_entry(Reader{data, at, len, in.body.data(), &c2}, len, begin, rlen, at, in.plain_at[k]);
      bool e2 = false, f2 = false;
      const zgk::Seek m2 = model(in.fr.data(), nrec, in.e.why, len, begin, rlen, k, at, in.plain_at[k], &e2, &f2);
      if (!same(an, m2)) bad |= 128u;
      if (c2.bad_reads) bad |= 256u;
      if (c2.body_reads) bad |= 512u;
      if (an.src_lo != un.src_lo || an.src_hi != un.src_hi || an.plain_lo != un.plain_lo || an.flags != un.flags || an.nblocks > un.nblocks ||
          an.bound != un.bound || an.status)
        bad |= 1024u;
      g_cov[6]++;
    }
    // anchors the call refuses: behind the entry, behind begin
    {
      Count c3;
      const zgk::Seek r1 = zgk::seek_entry(Reader{data, 0, len, in.body.data(), &c3}, len, begin, rlen, len + 1, 0);
      zgk::Seek z; memset(&z, 0, sizeof z); z.status = 93;
      if (!same(r1, z) || c3.bad_reads) bad |= 2048u;
      if (begin != ~0ull) {
        const zgk::Seek r2 = zgk::seek_entry(Reader{data, 0, len, in.body.data(), &c3}, len, begin, rlen, 0, begin + 1);
        if (!same(r2, z) || c3.bad_reads) bad |= 2048u;
      }
      g_cov[8]++;
    }
    if (bad) *where = begin;
  });
  return bad;
}
}  // namespace

extern "C" uint32_t sk_check(const uint8_t* data, uint64_t len, uint64_t* where) { return check(data, len, where); }
extern "C" void sk_coverage(uint64_t* out) { memcpy(out, g_cov, sizeof g_cov); }
extern "C" void sk_one(const uint8_t* data, uint64_t len, uint64_t begin, uint64_t rlen, uint64_t anchor_src, uint64_t anchor_plain, void* out) {
  const zgk::Seek s = zgk::seek_entry(NoCount{data}, len, begin, rlen, anchor_src, anchor_plain);
  memcpy(out, &s, sizeof s);
}

#ifdef SEEK_MAIN
// The same ranges and anchors over entries that lie in heap blocks of exactly their length, read directly: an access outside an entry is an
// AddressSanitizer report. The file holds [u64 length][bytes] per entry.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t n = 0, runs = 0, sum = 0;
  for (uint64_t len; fread(&len, 8, 1, f) == 1; n++) {
    uint8_t* e = (uint8_t*)malloc(len ? len : 1);
    if (len && fread(e, 1, len, f) != len) return 2;
    if (!len) { free(e); e = (uint8_t*)malloc(0); }
    Input in{e, len};
    prepare(in, false);
    ranges(in, [&](uint64_t begin, uint64_t rlen) {
      const zgk::Seek un = zgk::seek_entry(NoCount{e}, len, begin, rlen, 0, 0);
      runs++; sum += un.src_hi + un.nblocks;
      for (uint32_t k = 1; k < in.e.nrec; k++) {
        const uint64_t at = in.fr[k].begin;
        if (!in.sized_front[k] || at > un.src_lo || in.plain_at[k] > begin) continue;
        const zgk::Seek an = zgk::seek_entry(NoCount{e}, len, begin, rlen, at, in.plain_at[k]);
        runs++; sum += an.src_hi + an.nblocks;
      }
    });
    free(e);
  }
  fclose(f);
  printf("seek_asan ok: %llu entries, %llu runs (%llu)\n", (unsigned long long)n, (unsigned long long)runs, (unsigned long long)sum);
  return 0;
}
#endif
'''


class SeekC(C.Structure):
    _fields_ = [("src_lo", C.c_uint64), ("src_hi", C.c_uint64), ("plain_lo", C.c_uint64), ("bound", C.c_uint64), ("plain_seen", C.c_uint64),
                ("status", C.c_uint32), ("frames_skipped", C.c_uint32), ("frames_taken", C.c_uint32), ("nblocks", C.c_uint32),
                ("why", C.c_uint32), ("flags", C.c_uint32)]


def sized_frame(payload, checksum=False):
    """a single-segment frame with a 1-byte Frame_Content_Size and one raw block (payload up to 255 bytes)"""
    return MAGIC + bytes([0x20 | (0x04 if checksum else 0), len(payload)]) + block(payload, btype=0) + (b"\x00\x00\x00\x00" if checksum else b"")


def inputs():
    out = list(corpus())
    base = [z for _, z in out]
    hb = hand_built()
    rng = random.Random(0x5EEC)
    small = [z for z in base if 0 < len(z) <= 1 << 16]
    for k in range(60):
        parts = [rng.choice(small) for _ in range(rng.randint(2, 6))]
        out.append(("cat:%d" % k, b"".join(p + skippable(bytes([k & 255]) * rng.randint(0, 9)) for p in parts)))
    # sized frames, so that there are frames to skip: in front of an unsized frame, of a defect, of an empty frame
    a, b, e = sized_frame(b"a" * 100), sized_frame(b"b" * 255, checksum=True), sized_frame(b"")
    out.append(("sized:plain", a + b + a + skippable(b"xy") + b + a))
    out.append(("sized:empty_between", a + e + b + e + e + a))
    out.append(("sized:then_unsized", a + b + hb["raw_rle_blocks"] + a))
    out.append(("sized:broken_behind", a + b + a + hb["body_past_end"]))
    out.append(("sized:broken_in_skipped", a + b + a[:-40] ))
    out.append(("sized:garbage_behind", a + b + b"\x00\x01\x02\x03\x04\x05"))
    out.append(("sized:skip_past_end", a + b + skippable(b"abc", length=40) ))
    out.append(("sized:fcs8", hb["single_segment_fcs8"] + a + hb["fcs2_dict4"] + b))
    out.append(("sized:lie_small", MAGIC + bytes([0x20, 3]) + block(b"q" * 50, btype=0) + a + b))
    out.append(("sized:huge", MAGIC + bytes([0xE0]) + struct.pack("<Q", 2 ** 64 - 2) + block(b"abc", btype=0) + a + b))
    return out


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("seek")
    src, so, exe = d / "seek_lane.cpp", d / "libseek_lane.so", d / "seek_asan"
    src.write_text(HARNESS)
    flags = ["-std=c++17", "-Wall", "-Wno-unused-function", "-I", CSRC]
    subprocess.check_call(["g++", "-O2", *flags, "-shared", "-fPIC", "-o", str(so), str(src), os.path.join(CSRC, "zg_host_parse.cpp")])
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address", "-static-libasan", "-fno-omit-frame-pointer", "-DSEEK_MAIN", *flags, "-o", str(exe), str(src),
                           os.path.join(CSRC, "zg_host_parse.cpp")])
    L = C.CDLL(str(so))
    L.sk_check.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sk_check.restype = C.c_uint32
    L.sk_coverage.argtypes = [C.POINTER(C.c_uint64)]
    L.sk_one.argtypes = [C.c_void_p] + [C.c_uint64] * 5 + [C.c_void_p]
    return L, str(exe), d


def test_seek_equals_the_model_on_every_range(built):
    L, _, _ = built
    where = C.c_uint64(0)
    cases = inputs()
    assert len(cases) > 370
    for name, z in cases:
        buf = C.create_string_buffer(z, len(z))
        bad = L.sk_check(buf, len(z), C.byref(where))
        assert bad == 0, (name, "begin", where.value, "bits", bad)
    cov = (C.c_uint64 * 16)()
    L.sk_coverage(cov)
    assert cov[0] > 20000 and cov[6] > 2000, list(cov)
    assert cov[1] > 0, "an open-ended selection"
    assert cov[2] > 0, "a broken chain in front of the range"
    assert cov[3] > 0, "a broken chain inside the selection"
    assert cov[4] > 0, "an empty frame at a boundary"
    assert cov[5] > 0, "bit 2: nothing taken"
    assert cov[7] > 0 and cov[8] > 0


def test_seek_pinned_examples(built):
    L, _, _ = built
    a, b = sized_frame(b"a" * 100), sized_frame(b"b" * 255, checksum=True)
    z = a + b + skippable(b"xy") + a + b
    buf = C.create_string_buffer(z, len(z))
    s = SeekC()

    def one(begin, n, asrc=0, aplain=0):
        L.sk_one(buf, len(z), begin, n, asrc, aplain, C.byref(s))
        return (s.src_lo, s.src_hi, s.plain_lo, s.bound, s.status, s.frames_skipped, s.frames_taken, s.flags)

    la, lb, ls = len(a), len(b), 10
    assert one(0, 1) == (0, la, 0, 100, 0, 0, 1, 0)
    assert one(99, 2) == (0, la + lb, 0, 355, 0, 0, 2, 0)
    assert one(100, 1) == (la, la + lb, 100, 255, 0, 1, 1, 0)
    assert one(355, 1) == (la + lb + ls, 2 * la + lb + ls, 355, 100, 0, 2, 1, 0)      # the skippable frame lies in front of the selection
    assert one(354, 2) == (la, 2 * la + lb + ls, 100, 355, 0, 1, 2, 0)                # ... and inside it
    assert one(355, 1, la + lb, 355) == one(355, 1)[:5] + (0, 1, 0)
    assert one(710, 1) == (len(z), len(z), 710, 0, 0, 4, 0, 4)
    assert one(0, 2 ** 64 - 1) == (0, len(z), 0, 710, 0, 0, 4, 0)
    assert one(5, 0) == (0,) * 8
    assert one(5, 1, len(z) + 1, 0)[4] == 93 and one(5, 1, 0, 6)[4] == 93


def test_seek_under_address_sanitizer_stand_alone(built):
    _, exe, d = built
    path = d / "entries.bin"
    with open(path, "wb") as f:
        for _, z in inputs():
            f.write(struct.pack("<Q", len(z)) + z)
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    assert b"seek_asan ok" in p.stdout and b"AddressSanitizer" not in p.stderr


def test_ranges_argument_rules_need_no_gpu():
    L = zgpu.load_library()
    n = 1
    srcs, lens, dsts, caps = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_void_p * n)(), (C.c_size_t * n)()
    rg, sk, res = (zgpu.RangeC * n)(), (zgpu.SeekC * n)(), (zgpu.RangeResultC * n)()
    assert C.sizeof(zgpu.RangeC) == 32 and C.sizeof(zgpu.SeekC) == 64 and C.sizeof(zgpu.RangeResultC) == 40 + 64
    assert [f[0] for f in zgpu.SeekC._fields_] == [f[0] for f in SeekC._fields_]
    assert L.zgpu_frames_seek_device(None, srcs, lens, n, rg, sk) == 93          # ZGPU_E_BAD_ARG, no GPU touched
    assert L.zgpu_decode_ranges_device_src(None, srcs, lens, n, rg, dsts, caps, None, res) == 93
    fake = C.create_string_buffer(4096)   # null arrays with n > 0: refused before the context is looked at (this one is not a context)
    for k in range(4):
        a = [srcs, lens, rg, sk]
        a[k] = None
        assert L.zgpu_frames_seek_device(fake, *a[:2], n, *a[2:]) == 93, k
    for k in range(6):
        a = [srcs, lens, rg, dsts, caps, res]
        a[k] = None
        assert L.zgpu_decode_ranges_device_src(fake, a[0], a[1], n, a[2], a[3], a[4], None, a[5]) == 93, k
    out = (C.c_uint64 * 8)()
    assert L.zgpu_debug_ranges_stats(None, out, 8) == 0
    assert zgpu.E_CONTENT_SIZE_MISMATCH == 71
    for dev in (False, True):
        lib_ = zgpu.load_library(dev=dev)
        assert lib_.zgpu_status_name(71) == b"ContentSizeMismatch"
        for sym in ("zgpu_frames_seek_device", "zgpu_decode_ranges_device_src", "zgpu_debug_ranges_stats"):
            assert sym in zgpu.EXPORTS and hasattr(lib_, sym), sym
    for m in ("frames_seek_device", "decode_ranges_device_src", "ranges_stats", "decode_tensor_ranges"):
        assert hasattr(zgpu.Context, m)
    assert callable(zgpu.anchor_before)
