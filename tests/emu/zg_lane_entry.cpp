// zg_lane_entry.cpp — TEST-ONLY: runs zstd-rs_amd/csrc/zg_entry.h on the CPU — the facts of a decoded entry turned into its result (ladder,
// verify_fails, table_fails, fill, compare_list) and the pieces its clips take of its frames (clip_pieces). tests/test_entry_verdict_cpu.py
// builds this file (tests/lanesuite.py) as a shared library and — with -DENTRY_MAIN — as a stand-alone AddressSanitizer program in which the
// frames, the clips and every clip's destination lie in heap blocks of exactly their length (zg_lane_mem.h); both read the same case
// records and write the same result records, which the test compares with a restatement of include/zgpu.h in Python. Not part of the product.
//
// The steps are taken in the order an entry decoded alone takes them in one go and a submit takes them spread over its launches and waits
// (zg_frames.cpp): the ladder; ZGPU_DEVICE_VERIFY on what stands; the table's record on what still stands; the fill of what still stands.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zg_entry.h"
#include "zg_lane_mem.h"

namespace {
// A verdict case. head: nframes, nclips, flags (1 verify, 2 no_hash, 4 a record follows, 8 frames not known, 16 dict, 32 bound_buffer, 64 ranges,
// 128 promise), decode, walk, nframes counted from headers; then sound, total, cap, declared; frames x {begin, clen, yielded, declared, digest,
// checksum | hashed << 32 | has_checksum << 33 | declares << 34}; clips x {skip, len, cap}; the record (8 x u32) if flagged.
struct Head { uint32_t nframes, nclips, flags; int32_t decode, walk; uint32_t counted; uint64_t sound, total, cap, declared; };
enum { kVerify = 1, kNoHash = 2, kRecord = 4, kUnknown = 8, kDict = 16, kBoundBuffer = 32, kRanges = 64, kPromise = 128 };
constexpr uint32_t kOut = 14;   // status, written, nframes, checksums, mismatches, from_data, calculated, unverified, first_hashed, frames hashed,
                                // not hashed, the call's error (a record with a why), compare-list length, compare-list frames listed as hashed

// raw: the case's frames (6 u64 each) and clips (3 u64 each) where the caller put them; out: kOut u64, then {written, small} per clip
void settle(const Head& h, const uint64_t* raw_frames, const uint64_t* raw_clips, const zgv::Sums* rec, uint64_t hash_max, uint64_t* out) {
  std::vector<zge::Frame> fr(h.nframes);
  uint64_t cat = 0;
  for (uint32_t f = 0; f < h.nframes; f++) {
    const uint64_t* r = raw_frames + 6 * f;
    cat += r[2];
    fr[f] = zge::Frame{r[0], r[1], r[2], cat, r[3], r[4], (uint32_t)r[5], f, ((r[5] >> 34) & 1) != 0, ((r[5] >> 33) & 1) != 0, ((r[5] >> 32) & 1) != 0};
  }
  std::vector<zge::Clip> clips(h.nclips);
  for (uint32_t q = 0; q < h.nclips; q++) clips[q] = zge::Clip{raw_clips[3 * q], raw_clips[3 * q + 1], nullptr, raw_clips[3 * q + 2], 0, false};
  zge::Entry e;
  e.decode = h.decode; e.walk = h.walk; e.dict = (h.flags & kDict) != 0; e.known = !(h.flags & kUnknown); e.bound_buffer = (h.flags & kBoundBuffer) != 0;
  e.total = h.total; e.sound = h.sound; e.nframes = e.known ? h.nframes : h.counted; e.fr = fr.data();
  zge::Mode m;
  m.ranges = (h.flags & kRanges) != 0; m.promise = (h.flags & kPromise) != 0; m.cap = h.cap; m.declared = h.declared;
  m.clip = clips.data(); m.nclips = h.nclips;
  memset(out, 0, kOut * 8);
  zgpu_device_entry_result d;
  const zge::Verdict v = zge::ladder(e, m);
  zge::fail_entry(d, v.status);
  if (!d.r.status && (h.flags & kVerify)) zge::verify_fails(d, e);
  if (!d.r.status && e.nframes && rec) {
    std::vector<zgv::Frame> list;
    zge::compare_list(e, [&](const zge::Frame& f) { return hash_max == 0 || f.yielded <= hash_max; }, &list);
    out[12] = list.size();
    for (const zgv::Frame& x : list) out[13] += x.slot != zgv::kNotHashed;
    if (rec->why) out[11] = 1;
    else zge::table_fails(d, *rec, e.nframes);
  }
  if (!d.r.status && !out[11]) {
    d.r.written = v.written; d.r.nframes = e.nframes;
    const zge::Hashed hf = zge::fill(e, (h.flags & kNoHash) != 0, &d.r, &d.checksums_unverified, &d.first_hashed);
    out[9] = hf.hashed; out[10] = hf.not_hashed;
  }
  out[0] = (uint64_t)(int64_t)d.r.status; out[1] = d.r.written; out[2] = d.r.nframes; out[3] = d.r.checksums; out[4] = d.r.checksum_mismatches;
  out[5] = d.r.checksum_from_data; out[6] = d.r.calculated_checksum; out[7] = d.checksums_unverified; out[8] = d.first_hashed;
  for (uint32_t q = 0; q < h.nclips; q++) { out[kOut + 2 * q] = clips[q].written; out[kOut + 2 * q + 1] = clips[q].small; }
}

// A pieces case: frames of sizes[0 .. n) whose bytes are 1, 2, 3 ... in the concatenation; clips x {skip, len, small}. Clip q's destination is
// dst[q], room[q] bytes: every piece is applied to it, a piece that leaves it is counted in *outside and not applied. Returns per clip the count.
void pieces(const uint64_t* sizes, uint32_t n, const uint64_t* raw_clips, uint32_t nclips, uint8_t* const* dst, const uint64_t* room, uint64_t* at, uint64_t* outside) {
  std::vector<zge::Frame> fr(n);
  std::vector<uint8_t> concat;
  uint64_t cat = 0;
  for (uint32_t f = 0; f < n; f++) {
    cat += sizes[f];
    fr[f] = zge::Frame{};
    fr[f].yielded = sizes[f]; fr[f].end = cat;
    for (uint64_t k = 0; k < sizes[f]; k++) concat.push_back((uint8_t)(concat.size() + 1));
  }
  for (uint32_t q = 0; q < nclips; q++) {
    const zge::Clip cl{raw_clips[3 * q], raw_clips[3 * q + 1], dst[q], room[q], 0, raw_clips[3 * q + 2] != 0};
    uint64_t expect_at = 0;
    at[q] = zge::clip_pieces(fr.data(), n, cl, [&](const zge::Piece& p) {
      const uint64_t start = p.frame ? fr[p.frame - 1].end : 0;
      if (p.frame >= n || p.in_frame + p.len > fr[p.frame].yielded || p.cat != start + p.in_frame || p.at != expect_at || !p.len || p.at + p.len > room[q]) { (*outside)++; return; }
      memcpy(cl.dst + p.at, concat.data() + p.cat, p.len);
      expect_at += p.len;
    });
  }
}
}  // namespace

// cases: n records back to back as the Head comment says; out: per case kOut + 2 * nclips u64. Returns the bytes of `cases` consumed.
extern "C" uint64_t ze_settle(const uint8_t* cases, uint64_t n, uint64_t hash_max, uint64_t* out) {
  const uint8_t* p = cases;
  for (uint64_t c = 0; c < n; c++) {
    Head h;
    memcpy(&h, p, sizeof h);
    p += sizeof h;
    std::vector<uint64_t> fr(6 * (size_t)h.nframes + 1), cl(3 * (size_t)h.nclips + 1);
    memcpy(fr.data(), p, 48 * (size_t)h.nframes); p += 48 * (size_t)h.nframes;
    memcpy(cl.data(), p, 24 * (size_t)h.nclips); p += 24 * (size_t)h.nclips;
    zgv::Sums rec;
    if (h.flags & kRecord) { memcpy(&rec, p, 32); p += 32; }
    settle(h, fr.data(), cl.data(), (h.flags & kRecord) ? &rec : nullptr, hash_max, out);
    out += kOut + 2 * h.nclips;
  }
  return (uint64_t)(p - cases);
}
// one pieces case; dst: nclips blocks of `room` bytes each, back to back, which the caller filled
extern "C" uint64_t ze_pieces(const uint64_t* sizes, uint32_t n, const uint64_t* clips, uint32_t nclips, uint8_t* dst, uint64_t room, uint64_t* at) {
  std::vector<uint8_t*> d(nclips + 1);
  std::vector<uint64_t> r(nclips + 1, room);
  for (uint32_t q = 0; q < nclips; q++) d[q] = dst + q * room;
  uint64_t outside = 0;
  pieces(sizes, n, clips, nclips, d.data(), r.data(), at, &outside);
  return outside;
}

#ifdef ENTRY_MAIN
// argv[1]: verdict cases, each behind a u32 1, and pieces cases, each behind a u32 2: [u32 n][u32 nclips][n x u64 sizes][nclips x 3 u64]; argv[2]:
// the records — a verdict case's as ze_settle writes them, a pieces case's [nclips x u64 count][every clip's bytes]. Frames, clips and every
// clip's destination — exactly the bytes [skip, skip + len) of the concatenation has — lie in heap blocks of exactly their length.
int main(int argc, char** argv) {
  lane::CaseFile f(argc > 2 ? argv[1] : nullptr, "rb"), g(argc > 2 ? argv[2] : nullptr, "wb");
  uint64_t cases = 0, outside = 0;
  uint32_t kind;
  for (; f.next(&kind, 4); cases++) {
    if (kind == 1) {
      Head h;
      f.read(&h, sizeof h, 1);
      uint64_t* fr = (uint64_t*)f.block(48 * (uint64_t)h.nframes);
      uint64_t* cl = (uint64_t*)f.block(24 * (uint64_t)h.nclips);
      zgv::Sums rec;
      if (h.flags & kRecord) f.read(&rec, 32, 1);
      std::vector<uint64_t> out(kOut + 2 * (size_t)h.nclips);
      settle(h, fr, cl, (h.flags & kRecord) ? &rec : nullptr, 0, out.data());
      g.write(out.data(), 8, out.size());
      free(cl); free(fr);
    } else {
      uint32_t hd[2];
      f.read(hd, 4, 2);
      uint64_t* sizes = (uint64_t*)f.block(8 * (uint64_t)hd[0]);
      uint64_t* cl = (uint64_t*)f.block(24 * (uint64_t)hd[1]);
      uint64_t total = 0;
      for (uint32_t k = 0; k < hd[0]; k++) total += sizes[k];
      std::vector<uint8_t*> dst(hd[1] + 1);
      std::vector<uint64_t> room(hd[1] + 1), at(hd[1] + 1);
      for (uint32_t q = 0; q < hd[1]; q++) {
        const uint64_t rest = total > cl[3 * q] ? total - cl[3 * q] : 0;
        room[q] = cl[3 * q + 2] ? 0 : rest < cl[3 * q + 1] ? rest : cl[3 * q + 1];
        dst[q] = (uint8_t*)malloc((size_t)room[q]);
        if (room[q] && !dst[q]) return lane::kExitIO;
      }
      pieces(sizes, hd[0], cl, hd[1], dst.data(), room.data(), at.data(), &outside);
      g.write(at.data(), 8, hd[1]);
      for (uint32_t q = 0; q < hd[1]; q++) { g.write(dst[q], 1, (size_t)(at[q] < room[q] ? at[q] : room[q])); free(dst[q]); }
      free(cl); free(sizes);
    }
  }
  f.close();
  g.close();
  if (outside) return lane::kExitLanes;
  printf("entry_asan ok: %llu cases\n", (unsigned long long)cases);
  return 0;
}
#endif
