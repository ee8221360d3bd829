// zg_lane_seektab_write_sums.cpp — TEST-ONLY: zgt::write_seek_table_sums (zstd-rs_amd/csrc/zg_seektab.h), the serialiser behind
// zgpu_seek_index_export_seek_table_ex with ZGPU_EXPORT_CHECKSUMS. tests/test_seektab_write_sums_cpu.py builds it through tests/lanesuite.py: as
// a shared library (stws_run, no sanitizer) and, with -DSEEKTAB_WRITE_SUMS_MAIN, as a stand-alone AddressSanitizer program. It reads cases
// from a file — a u32 row count, the 2 * (nrows + 1) 64-bit prefix sums C[k], D[k], the nrows sums — and runs each twice: into a lane::Guarded
// block of exactly seek_table_sums_bytes(nrows) bytes between two bands of kFill, whose bands must stay intact, and into a heap block of
// exactly that size, where a sanitizer sees any store outside. Per case it writes to a second file: the status, whether a refused case left
// every byte of the block untouched, the byte count and the bytes. The test compares them with zgpu.seek_table_frame. Not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zg_seektab.h"
#include "zg_lane_mem.h"

static int run_cases(const char* src, const char* dst, uint32_t* ncases) {
  lane::CaseFile in(src, "rb"), out(dst, "wb");
  uint32_t nrows = 0, cases = 0;
  while (in.next(&nrows, sizeof nrows)) {
    std::vector<uint64_t> cd(2 * ((size_t)nrows + 1), 0);
    in.read(cd.data(), 8, cd.size());
    uint32_t* sums = (uint32_t*)in.block((uint64_t)nrows * 4);   // (exactly nrows sums: a read behind them is a sanitizer report)
    const uint64_t need = zgt::seek_table_sums_bytes(nrows);
    lane::Guarded<uint8_t> g(need, 64);
    const uint32_t st = zgt::write_seek_table_sums(cd.data(), sums, nrows, g.mid());
    uint8_t* exact = (uint8_t*)malloc((size_t)need);
    if (!exact) return lane::kExitIO;
    memset(exact, lane::kFill, (size_t)need);
    const uint32_t st2 = zgt::write_seek_table_sums(cd.data(), sums, nrows, exact);
    uint32_t untouched = 1;
    for (uint64_t k = 0; k < need; k++) untouched &= g.mid()[k] == lane::kFill && exact[k] == lane::kFill;
    if (!g.intact() || st != st2 || memcmp(g.mid(), exact, (size_t)need)) { fprintf(stderr, "case %u: the two runs differ, or a guard band changed\n", cases); return 1; }
    const uint64_t nout = st ? 0 : need;
    out.write(&st, 4, 1); out.write(&untouched, 4, 1); out.write(&nout, 8, 1); out.write(exact, 1, (size_t)nout);
    free(exact); free(sums);
    cases++;
  }
  out.close();
  *ncases = cases;
  return 0;
}
extern "C" int stws_run(const char* src, const char* dst, uint32_t* ncases) { return run_cases(src, dst, ncases); }

#ifdef SEEKTAB_WRITE_SUMS_MAIN
int main(int argc, char** argv) {
  if (argc < 3) return lane::kExitIO;
  uint32_t cases = 0;
  const int rc = run_cases(argv[1], argv[2], &cases);
  if (rc) return rc;
  printf("seektab_write_sums ok: %u cases\n", cases);
  return 0;
}
#endif
