"""zg_k_index's lane routine (zstd-rs_amd/csrc/zg_index.h) and the host's reading of its frame records (zg_host_parse.cpp: frame_fields),
compiled with g++ and run on the CPU. For every input the lane runs twice, summary pass and emit pass, over a reader that counts every
access outside [0, len) and every access to a byte of a block body (the bodies as zgw::walk_entry's records give them), and a writer that
counts every store outside the lane's own record range (which lies between guard records). Demanded of every input:
  - bound == plaintext_bound(bytes);
  - chain_end and why are zgw::walk_entry's stop_off and why;
  - nframes, nskippable and nblocks are a count over the walk's records;
  - the frame records' bounds sum to the entry's bound, their extents tile [0, chain_end) in order, their header fields are what
    read_frame_header gives on the walk's frame records, and — on inputs parse_frames accepts — what parse_frames' FrameInfo says;
  - reads outside the entry 0, reads of a block body 0, stores outside the range 0; the emit pass says what the summary pass said.
The corpus is tests/test_walk_cpu.py's (every golden pack: decodecorpus, dictionary fixtures, fuzz artefacts, synthetic; the regress and
verdict_order frames; the seqframes families; hand-built frames; concatenations with skippable frames), every prefix of its small
inputs, and single-byte edits aimed at every frame-header and block-header byte of them. Two edges are pinned besides: an emit pass over
an input that changed since the summary pass ends in a count the host refuses and no stray store, and a frame table that is too small is
answered with the count needed."""
import ctypes as C
import os
import subprocess

import pytest

import zgpu
from test_walk_cpu import MAX_WINDOW, corpus, hand_built, skippable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstd-rs_amd", "csrc")
HARNESS = r'''
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zg_host_parse.h"
#include "zg_index.h"
using namespace zg;
namespace {
struct Count { uint64_t bad_reads = 0, body_reads = 0, bad_writes = 0, written = 0; };
struct Reader {   // the entry as a lane may see it: bytes [0, len), and none that belongs to a block body
  const uint8_t* p; uint64_t len; const uint8_t* body; Count* c;
  uint8_t ld1(uint64_t off) const {
    if (off >= len) { c->bad_reads++; return 0; }
    if (body && body[off]) c->body_reads++;
    return p[off];
  }
};
struct Writer {   // the lane's record range [lo, hi) of recs
  zgi::FrameRec* recs; uint64_t lo, hi; Count* c;
  void put(uint64_t i, const zgi::FrameRec& x) const { if (i < lo || i >= hi) { c->bad_writes++; return; } recs[i] = x; c->written++; }
};
struct NoCount { uint8_t ld1(uint64_t off) const { return p[off]; } const uint8_t* p; };
struct WalkWriter { zgw::Rec* recs; void put(uint64_t i, const zgw::Rec& x) const { recs[i] = x; } };
constexpr uint64_t kGuard = 4;
uint64_t g_why[16], g_cases, g_flagbits[4], g_recflags[5], g_unreadable;

// one input: 0 if everything agrees, else a bit per kind of disagreement
uint32_t check(const uint8_t* data, uint64_t len, uint64_t max_window) {
  uint32_t bad = 0;
  // the reference: the walk's records and where it stopped
  const NoCount nr{data};
  const zgw::End w0 = zgw::walk_entry<false>(nr, WalkWriter{nullptr}, len, 0, 0);
  std::vector<zgw::Rec> wrecs(w0.nrec + 1);
  (void)zgw::walk_entry<true>(nr, WalkWriter{wrecs.data()}, len, 0, w0.nrec);
  std::vector<uint8_t> body(len + 1, 0);
  uint32_t wframes = 0, wskip = 0, wblocks = 0;
  std::vector<const zgw::Rec*> wfr;
  for (uint32_t k = 0; k < w0.nrec; k++) {
    const zgw::Rec& x = wrecs[k];
    if (x.kind == zgw::kFrame) {
      FrameFields f;
      frame_fields(x.b, x.have, &f);
      wframes += f.header_status == ZG_OK; wskip += f.header_status == ZG_SKIP_FRAME;
      wfr.push_back(&x);
    } else if (x.kind == zgw::kBlock) {
      wblocks++;
      const uint32_t type = (x.b[0] >> 1) & 3u, size = (uint32_t)(x.b[0] >> 3) | ((uint32_t)x.b[1] << 5) | ((uint32_t)x.b[2] << 13);
      if (type == 3 || size > zgw::kBlockMax) continue;
      const uint64_t n = type == 1 ? 1 : size;
      for (uint64_t q = x.off; q < x.off + n && q < len; q++) body[q] = 1;
    }
  }
  Count c;
  const Reader r{data, len, body.data(), &c};
  const Writer none{nullptr, 0, 0, &c};
  const zgi::Entry e0 = zgi::index_entry<false>(r, none, len, 0, 0);
  if (c.written || c.bad_writes) bad |= 1u;
  std::vector<zgi::FrameRec> recs(e0.nrec + 2 * kGuard);
  memset((void*)recs.data(), 0xEE, recs.size() * sizeof(zgi::FrameRec));
  const Writer w{recs.data(), kGuard, kGuard + e0.nrec, &c};
  const zgi::Entry e1 = zgi::index_entry<true>(r, w, len, kGuard, e0.nrec);
  if (!zgi::same_entry(e0, e1)) bad |= 2u;
  if (c.written != e0.nrec) bad |= 4u;
  if (c.bad_reads) bad |= 8u;
  if (c.bad_writes) bad |= 16u;
  if (c.body_reads) bad |= 32u;
  for (uint64_t g = 0; g < kGuard; g++) {
    const uint8_t* a = (const uint8_t*)&recs[g];
    const uint8_t* b = (const uint8_t*)&recs[kGuard + e0.nrec + g];
    for (size_t k = 0; k < sizeof(zgi::FrameRec); k++) if (a[k] != 0xEE || b[k] != 0xEE) bad |= 16u;
  }
  if (e0.nrec > 1) {   // a lane whose range is shorter than its records still stays inside it, and says how many it has
    Count c2;
    std::vector<zgi::FrameRec> few(e0.nrec - 1 + 2 * kGuard);
    const Writer w2{few.data(), kGuard, kGuard + e0.nrec - 1, &c2};
    const zgi::Entry e2 = zgi::index_entry<true>(Reader{data, len, body.data(), &c2}, w2, len, kGuard, e0.nrec - 1);
    if (c2.bad_writes || c2.bad_reads || c2.body_reads || c2.written != e0.nrec - 1 || e2.nrec != e0.nrec) bad |= 16u;
  }
  if (e0.bound != plaintext_bound(data, len)) bad |= 64u;
  if (e0.chain_end != w0.stop_off || e0.why != w0.why) bad |= 128u;
  if (e0.nframes != wframes || e0.nskippable != wskip || e0.nblocks != wblocks) bad |= 256u;
  if (e0.nrec != wfr.size() || e0.pad != 0) bad |= 512u;
  // the frame records: bounds, extents, header fields
  const zgi::FrameRec* fr = recs.data() + kGuard;
  uint64_t sum = 0, at = 0, blocks = 0;
  uint32_t flags = e0.nframes ? (zgi::kAllSized | zgi::kAllComplete) : 0u;
  for (uint32_t k = 0; k < e0.nrec && k < wfr.size(); k++) {
    const zgi::FrameRec& x = fr[k];
    sum += x.bound; blocks += x.nblocks;
    if (x.begin != at || x.end < x.begin || x.end > len || x.begin != wfr[k]->off) bad |= 1024u;
    at = x.end;
    FrameFields a, b;
    frame_fields(x.b, x.have, &a);
    frame_fields(wfr[k]->b, wfr[k]->have, &b);
    if (memcmp(&a, &b, sizeof a)) bad |= 2048u;
    for (uint32_t q = x.have; q < sizeof x.b; q++) if (x.b[q]) bad |= 2048u;
    if (((x.flags & zgi::kSkippable) != 0) != (a.header_status == ZG_SKIP_FRAME) || (x.flags & ~(zgi::kSkippable | zgi::kComplete))) bad |= 2048u;
    if (a.header_status == ZG_OK) {
      if (!(a.flags & 2u)) flags &= ~zgi::kAllSized;
      if (a.dict_id) flags |= zgi::kAnyDict;
      if (a.flags & 4u) flags |= zgi::kAnyChecksum;
      if (!(x.flags & zgi::kComplete)) flags &= ~zgi::kAllComplete;
      if ((a.flags & 2u) && x.bound > a.frame_content_size) bad |= 4096u;
    } else {
      if (x.bound || x.nblocks || (x.flags & zgi::kComplete)) bad |= 4096u;
      if (a.header_status != ZG_SKIP_FRAME) { g_unreadable++; if (x.begin != x.end || k + 1 != e0.nrec) bad |= 4096u; }
    }
    for (int q = 0; q < 5; q++) if ((x.flags | a.flags) & (1u << q)) g_recflags[q]++;
  }
  if (sum != e0.bound || blocks != e0.nblocks) bad |= 8192u;
  if (at != e0.chain_end) bad |= 16384u;
  if (flags != e0.flags) bad |= 32768u;
  // against the host's parse, where it accepts the whole input: one record per frame or skippable frame, fields as FrameInfo has them
  BatchBuilder bb;
  std::vector<FrameInfo> info;
  if (parse_frames(data, len, max_window, &bb, &info, 0) == ZG_OK) {
    size_t f = 0;
    if (e0.why != zgw::kEnd || !(e0.nframes == 0 || (e0.flags & zgi::kAllComplete))) bad |= 65536u;
    for (uint32_t k = 0; k < e0.nrec; k++) {
      const zgi::FrameRec& x = fr[k];
      if (x.flags & zgi::kSkippable) continue;
      FrameFields a;
      frame_fields(x.b, x.have, &a);
      if (f >= info.size()) { bad |= 65536u; break; }
      const FrameInfo& fi = info[f++];
      if (x.begin != fi.src_begin || x.end != fi.src_end || x.nblocks != fi.nblocks || a.window_size != fi.window_size ||
          a.frame_content_size != fi.header.frame_content_size || ((a.flags & 4u) != 0) != fi.has_checksum || !(x.flags & zgi::kComplete))
        bad |= 65536u;
    }
    if (f != info.size() || e0.nframes != info.size()) bad |= 65536u;
  }
  g_cases++;
  g_why[e0.why & 15]++;
  for (int q = 0; q < 4; q++) if (e0.flags & (1u << q)) g_flagbits[q]++;
  return bad;
}
}  // namespace

extern "C" uint32_t ix_check(const uint8_t* data, uint64_t len, uint64_t max_window) { return check(data, len, max_window); }
extern "C" uint32_t ix_prefixes(const uint8_t* data, uint64_t len, uint64_t upto, uint64_t max_window, uint64_t* where) {
  const uint64_t n = len < upto ? len : upto;
  for (uint64_t k = 0; k <= n; k++) { const uint32_t bad = check(data, k, max_window); if (bad) { *where = k; return bad; } }
  return 0;
}
// single-byte edits at every frame-header byte (and the three bytes behind the header) and every block-header byte, each set to 0x00, 0xFF,
// one flipped bit and one random value (fixed seed); at most `budget` positions per input, evenly spread (0: every one)
extern "C" uint32_t ix_edits(uint8_t* data, uint64_t len, uint64_t max_window, uint64_t seed, uint64_t budget, uint64_t* where, uint64_t* nedits) {
  const NoCount nr{data};
  const zgw::End w0 = zgw::walk_entry<false>(nr, WalkWriter{nullptr}, len, 0, 0);
  std::vector<zgw::Rec> wrecs(w0.nrec + 1);
  (void)zgw::walk_entry<true>(nr, WalkWriter{wrecs.data()}, len, 0, w0.nrec);
  std::vector<uint64_t> pos;
  for (uint32_t k = 0; k < w0.nrec; k++) {
    const zgw::Rec& x = wrecs[k];
    if (x.kind == zgw::kFrame) for (uint64_t q = 0; q < x.have; q++) pos.push_back(x.off + q);
    else if (x.kind == zgw::kBlock) for (uint64_t q = 0; q < 3; q++) pos.push_back(x.off - 3 + q);
  }
  uint64_t x = seed * 6364136223846793005ull + 1442695040888963407ull;
  const uint64_t step = budget && pos.size() > budget ? (pos.size() + budget - 1) / budget : 1;
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
extern "C" void ix_coverage(uint64_t* why, uint64_t* flagbits, uint64_t* recflags, uint64_t* unreadable, uint64_t* cases) {
  memcpy(why, g_why, sizeof g_why); memcpy(flagbits, g_flagbits, sizeof g_flagbits); memcpy(recflags, g_recflags, sizeof g_recflags);
  *unreadable = g_unreadable; *cases = g_cases;
}
// The emit pass over `now` with the ranges the summary pass took from `then`: out[0] stores outside the range, [1] reads outside the entry,
// [2] records written, [3] the limit, [4] whether the host would accept the pass (same_entry), [5] the count the pass reports
extern "C" void ix_changed(const uint8_t* then, uint64_t then_len, const uint8_t* now, uint64_t now_len, uint64_t* out) {
  Count c;
  const Writer none{nullptr, 0, 0, &c};
  const zgi::Entry e0 = zgi::index_entry<false>(Reader{then, then_len, nullptr, &c}, none, then_len, 0, 0);
  std::vector<zgi::FrameRec> recs(e0.nrec + 2 * kGuard);
  const Writer w{recs.data(), kGuard, kGuard + e0.nrec, &c};
  const zgi::Entry e1 = zgi::index_entry<true>(Reader{now, now_len, nullptr, &c}, w, now_len, kGuard, e0.nrec);
  out[0] = c.bad_writes; out[1] = c.bad_reads; out[2] = c.written; out[3] = e0.nrec; out[4] = zgi::same_entry(e0, e1); out[5] = e1.nrec;
}
// The host's prefix sum over the summaries of n entries: first[0 .. n], returns the records a table needs
extern "C" uint64_t ix_ranges(const uint8_t* const* data, const uint64_t* lens, uint32_t n, uint64_t* first) {
  Count c;
  std::vector<zgi::Entry> e(n);
  for (uint32_t i = 0; i < n; i++) e[i] = zgi::index_entry<false>(Reader{data[i], lens[i], nullptr, &c}, Writer{nullptr, 0, 0, &c}, lens[i], 0, 0);
  return zgi::frame_ranges(e.data(), n, first);
}
'''
SMALL = 4096   # inputs up to this long: every prefix, and every header byte edited


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("index")
    src, so = d / "index_lane.cpp", d / "libindex_lane.so"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src),
                           os.path.join(CSRC, "zg_host_parse.cpp")])
    L = C.CDLL(str(so))
    u64, vp = C.c_uint64, C.c_void_p
    L.ix_check.argtypes = [vp, u64, u64]
    L.ix_check.restype = C.c_uint32
    L.ix_prefixes.argtypes = [vp, u64, u64, u64, C.POINTER(u64)]
    L.ix_prefixes.restype = C.c_uint32
    L.ix_edits.argtypes = [vp, u64, u64, u64, u64, C.POINTER(u64), C.POINTER(u64)]
    L.ix_edits.restype = C.c_uint32
    L.ix_coverage.argtypes = [C.POINTER(u64)] * 5
    L.ix_changed.argtypes = [vp, u64, vp, u64, C.POINTER(u64)]
    L.ix_changed.restype = None
    L.ix_ranges.argtypes = [C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64)]
    L.ix_ranges.restype = u64
    return L


def test_index_equals_walk_and_bound_everywhere(lib):
    where, nedits = C.c_uint64(0), C.c_uint64(0)
    total_edits = small = 0
    cases = corpus()
    assert len(cases) > 300
    packs = set(name.split(":")[0] for name, _ in cases)
    for need in ("decodecorpus.pack", "dict_tests.pack", "fuzz_artifacts.pack", "synthetic.pack", "seqframes", "hand", "concat"):
        assert need in packs, need
    for seed, (name, z) in enumerate(cases):
        buf = C.create_string_buffer(z, len(z))
        assert lib.ix_check(buf, len(z), MAX_WINDOW) == 0, name
        bad = lib.ix_prefixes(buf, len(z), SMALL, MAX_WINDOW, C.byref(where))
        assert bad == 0, (name, "prefix", where.value, bad)
        every = len(z) <= SMALL
        small += every
        bad = lib.ix_edits(buf, len(z), MAX_WINDOW, 0x1DE5 + seed, 0 if every else 400, C.byref(where), C.byref(nedits))
        assert bad == 0, (name, "edit at", where.value, bad)
        assert buf.raw == z
        total_edits += nedits.value
    assert small > 100 and total_edits > 20000
    u64 = C.c_uint64
    why, fb, rf, unread, n = (u64 * 16)(), (u64 * 4)(), (u64 * 5)(), u64(0), u64(0)
    lib.ix_coverage(why, fb, rf, C.byref(unread), C.byref(n))
    assert n.value > 100000
    assert all(why[k] > 0 for k in range(9)), list(why)[:9]       # every reason a chain ends for
    assert all(x > 0 for x in fb), list(fb)                       # every entry flag seen set
    assert all(x > 0 for x in rf), list(rf)                       # every frame flag seen set
    assert unread.value > 0                                       # records of headers the chain could not read


def test_emit_pass_over_a_changed_input_is_refused_without_a_stray_store(lib):
    hb = hand_built()
    good = hb["raw_rle_blocks"]
    out = (C.c_uint64 * 6)()
    changes = [(good, good * 5),                                    # more frames than the summary pass counted
               (good * 3, good),                                    # fewer
               (good + skippable(b"abc"), skippable(b"abc") * 9),   # other kinds
               (good * 2, good + hb["bad_magic"]),                  # the same count, another end
               (b"", good * 2)]
    for then, now in changes:
        a, b = C.create_string_buffer(then, len(then)), C.create_string_buffer(now, len(now))
        lib.ix_changed(a, len(then), b, len(now), out)
        assert out[0] == 0 and out[1] == 0, (then, now, list(out))
        assert out[2] <= out[3], list(out)
        assert out[4] == 0, list(out)                               # the host refuses the pass (ZGPU_E_INTERNAL)
    same = C.create_string_buffer(good * 3, len(good) * 3)
    lib.ix_changed(same, len(good) * 3, same, len(good) * 3, out)
    assert list(out) == [0, 0, 3, 3, 1, 3]


def test_a_table_that_is_too_small_is_answered_with_the_count_needed(lib):
    hb = hand_built()
    ents = [hb["frame_skip_frame"], b"", hb["raw_rle_blocks"] * 7, hb["skip_only"], hb["frames_then_garbage"], hb["empty"]]
    want = [4, 0, 7, 2, 3, 0]          # (frames_then_garbage: two frames and the header that cannot be read)
    n = len(ents)
    bufs = [C.create_string_buffer(e, len(e)) for e in ents]
    ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_uint64 * n)(*[len(e) for e in ents])
    first = (C.c_uint64 * (n + 1))()
    need = lib.ix_ranges(ptrs, lens, n, first)
    assert need == sum(want) and list(first) == [sum(want[:i]) for i in range(n + 1)]


def test_index_argument_rules_need_no_gpu():
    L = zgpu.load_library()
    n = 1
    srcs, lens = (C.c_void_p * n)(), (C.c_size_t * n)()
    ents = (zgpu.EntryIndexC * n)()
    first = (C.c_uint64 * (n + 1))()
    frames = (zgpu.FrameIndexC * 4)()
    need = C.c_size_t(0)
    assert C.sizeof(zgpu.EntryIndexC) == 40 and C.sizeof(zgpu.FrameIndexC) == 64
    assert L.zgpu_frames_index_device(None, srcs, lens, n, ents) == 93          # ZGPU_E_BAD_ARG, no GPU touched
    assert L.zgpu_frames_table_device(None, srcs, lens, n, ents, first, frames, 4, C.byref(need)) == 93
    fake = C.create_string_buffer(4096)   # null arrays with n > 0: refused before the context is looked at (this one is not a context)
    for k in range(3):
        a = [srcs, lens, ents]
        a[k] = None
        assert L.zgpu_frames_index_device(fake, a[0], a[1], n, a[2]) == 93, k
        assert L.zgpu_frames_table_device(fake, a[0], a[1], n, a[2], first, frames, 4, C.byref(need)) == 93, k
    assert L.zgpu_frames_table_device(fake, srcs, lens, n, ents, None, frames, 4, C.byref(need)) == 93
    assert L.zgpu_frames_table_device(fake, srcs, lens, n, ents, first, None, 4, C.byref(need)) == 93
    assert L.zgpu_frames_table_device(fake, srcs, lens, n, ents, first, frames, 4, None) == 93
    out = (C.c_uint64 * 4)()
    assert L.zgpu_debug_frames_index_stats(None, out, 4) == 0
    for dev in (False, True):
        lib_ = zgpu.load_library(dev=dev)
        for sym in ("zgpu_frames_index_device", "zgpu_frames_table_device", "zgpu_debug_frames_index_stats"):
            assert sym in zgpu.EXPORTS and hasattr(lib_, sym), sym
    for m in ("frames_index_device", "frames_table_device", "frames_index_stats", "split_tensor_frames", "decode_tensors"):
        assert hasattr(zgpu.Context, m)
    # the stop reasons are public under the lanes' values
    assert [zgpu.CHAIN_END, zgpu.CHAIN_SHORT_HEADER, zgpu.CHAIN_BAD_MAGIC, zgpu.CHAIN_SKIP_PAST_END, zgpu.CHAIN_SHORT_BLOCK_HEADER,
            zgpu.CHAIN_RESERVED_BLOCK, zgpu.CHAIN_BLOCK_TOO_LARGE, zgpu.CHAIN_BODY_PAST_END, zgpu.CHAIN_SHORT_CHECKSUM] == list(range(9))
