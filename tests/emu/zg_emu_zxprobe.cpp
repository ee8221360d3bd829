// zg_emu_zxprobe.cpp — TEST-ONLY: runs the SOURCE of zg_k_zxprobe (zstd-rs_amd/csrc/zg_zxprobe.h: one zx_* primitive per run, one workgroup of
// 64 or 256 threads) on the CPU through the SIMT emulator of zg_simt.h, behind the argument rules zgpu_debug_zx_probe has (zxp::args_ok). The
// operands, the result words and the memory arena live in heap blocks of exactly their sizes, so that under AddressSanitizer an access the rules
// should have stopped is a report. tests/test_zxprobe_cpu.py builds this file (tests/lanesuite.py; it is not in the Makefile's library) as a
// shared library and, with -DZXP_MAIN, as a stand-alone program that runs a file of cases and compares them with the results the file holds.
// Not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_types.h"
#include "zg_simt.h"
#include "../../zstd-rs_amd/csrc/zg_zxprobe.h"

// 0, or -1 where zgpu_debug_zx_probe answers ZGPU_E_BAD_ARG. out[] is taken as the caller filled it; arena_out = the whole arena afterwards
extern "C" int zxp_run(uint32_t op, uint32_t threads, uint32_t flags, uint32_t res_off, uint32_t res_bytes, const uint32_t* in, uint32_t* out,
                       const uint8_t* arena_in, uint8_t* arena_out, uint32_t arena_bytes) {
  if (!in || !out || !arena_in || !arena_out || !zxp::args_ok(op, threads, flags, res_off, res_bytes, in, arena_bytes)) return -1;
  const size_t in_bytes = (size_t)threads * zxp::kIn * 4, out_bytes = (size_t)threads * zxp::kOut * 4;
  uint32_t* h_in = (uint32_t*)malloc(in_bytes);
  uint32_t* h_out = (uint32_t*)malloc(out_bytes);
  void* h_arena = nullptr;
  if (!h_in || !h_out || posix_memalign(&h_arena, 16, arena_bytes)) abort();
  memcpy(h_in, in, in_bytes); memcpy(h_out, out, out_bytes); memcpy(h_arena, arena_in, arena_bytes);
  static zxp::Lds lds;
  memset(&lds, 0xEE, sizeof lds);
  simt::run(threads, [&]() { zxp::probe(op, flags, h_in, h_out, (uint8_t*)h_arena, res_off, res_bytes, lds); });
  const bool in_kept = memcmp(h_in, in, in_bytes) == 0;
  memcpy(out, h_out, out_bytes); memcpy(arena_out, h_arena, arena_bytes);
  free(h_in); free(h_out); free(h_arena);
  return in_kept ? 0 : -2;
}
extern "C" uint32_t zxp_ops(void) { return zxp::kOps; }

#ifdef ZXP_MAIN
// a file of cases (tests/zxprobe.py: write_cases), little-endian words: "ZXPC", the number of cases; per case op, threads, flags, res_off, res_bytes,
// arena_bytes, then in[8 T], out[4 T] as it goes in, the arena, out[4 T] as the model wants it, the arena as the model wants it
static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }
// `--outside WHAT`: the two kinds of domain abort no case file can reach — the probe's DPP routines have no early return and zxp::args_ok
// refuses the offsets — called directly, past the argument rules. Each must end in the emulator's abort; "dword" is the one offset above
// 0xFFFFFFF0 that is inside a domain (zg_simt.h: zx_ld32 at a multiple of 4) and must read 0.
static int outside(const char* what) {
  static uint32_t got[64];
  uint8_t* block = (uint8_t*)malloc(16);
  memset(block, 0x5A, 16);
  const ZxBuf b = zx_buf(block, 16);
  if (!strcmp(what, "dpp-step")) simt::run(64, [&]() { if (zx_tid() == 5) return; got[zx_tid()] = zx_scan_src<0>(zx_tid(), 7u); });
  else if (!strcmp(what, "dpp-scan")) simt::run(256, [&]() { if (zx_tid() == 64 + 63) return; got[zx_tid() & 63u] = zx_scan_incl_add(zx_tid()); });
  else if (!strcmp(what, "dpp-shr1")) simt::run(64, [&]() { if (zx_tid() & 1u) return; got[zx_tid()] = zx_shr1(zx_tid(), 7u); });
  else if (!strcmp(what, "dpp-partial-wave")) simt::run(32, [&]() { got[zx_tid()] = zx_shr1(zx_tid(), 7u); });
  else if (!strcmp(what, "ld128")) simt::run(64, [&]() { got[zx_tid()] = zx_ld128(b, 0xFFFFFFF0u).x; });
  else if (!strcmp(what, "ld96")) simt::run(64, [&]() { got[zx_tid()] = zx_ld96(b, 0xFFFFFFF8u).x; });
  else if (!strcmp(what, "ld64")) simt::run(64, [&]() { got[zx_tid()] = zx_ld64(b, 0xFFFFFFFCu).x; });
  else if (!strcmp(what, "ld32-unaligned")) simt::run(64, [&]() { got[zx_tid()] = zx_ld32(b, 0xFFFFFFFDu); });
  else if (!strcmp(what, "ld8")) simt::run(64, [&]() { got[zx_tid()] = zx_ld8(b, 0xFFFFFFF0u); });
  else if (!strcmp(what, "st8")) simt::run(64, [&]() { zx_st8(b, 0xFFFFFFFFu, 1u); });
  else if (!strcmp(what, "st32")) simt::run(64, [&]() { zx_st32(b, 0xFFFFFFF0u, 1u); });
  else if (!strcmp(what, "dword")) {
    simt::run(64, [&]() { got[zx_tid()] = zx_ld32(b, 0xFFFFFFF0u + 4u * (zx_tid() & 3u)) | zx_ld32(b, 0xFFFFFFECu) | (zx_ld32(b, 12u) ^ 0x5A5A5A5Au); });
    for (uint32_t t = 0; t < 64; t++) if (got[t]) { printf("lane %u read 0x%08X\n", t, got[t]); return 1; }
    free(block);
    printf("zxprobe ok: dword\n");
    return 0;
  } else return 2;
  printf("zxprobe: %s came back\n", what);   // (not reached)
  free(block);
  return 1;
}
int main(int argc, char** argv) {
  if (argc > 2 && !strcmp(argv[1], "--outside")) return outside(argv[2]);
  FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  uint32_t magic = 0, n = 0;
  if (!f || !rd(f, &magic, 4) || !rd(f, &n, 4) || magic != 0x4350585Au) { fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
  for (uint32_t i = 0; i < n; i++) {
    uint32_t h[6];
    if (!rd(f, h, sizeof h) || (h[1] != 64 && h[1] != 256) || h[5] > zxp::kArenaMax) { fprintf(stderr, "case %u: bad header\n", i); return 2; }
    const size_t T = h[1];
    std::vector<uint32_t> in(T * zxp::kIn), out(T * zxp::kOut), want(T * zxp::kOut);
    std::vector<uint8_t> arena(h[5]), arena_out(h[5]), arena_want(h[5]);
    if (!rd(f, in.data(), in.size() * 4) || !rd(f, out.data(), out.size() * 4) || !rd(f, arena.data(), arena.size()) ||
        !rd(f, want.data(), want.size() * 4) || !rd(f, arena_want.data(), arena_want.size())) { fprintf(stderr, "case %u: short file\n", i); return 2; }
    const int st = zxp_run(h[0], h[1], h[2], h[3], h[4], in.data(), out.data(), arena.data(), arena_out.data(), h[5]);
    if (st) { printf("case %u (op %u): refused (%d)\n", i, h[0], st); return 1; }
    if (out != want) { printf("case %u (op %u): results differ from the model\n", i, h[0]); return 1; }
    if (arena_out != arena_want) { printf("case %u (op %u): the arena differs from the model\n", i, h[0]); return 1; }
  }
  fclose(f);
  printf("zxprobe ok: %u cases\n", n);
  return 0;
}
#endif
