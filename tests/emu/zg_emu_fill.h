// zg_emu_fill.h — TEST-ONLY: what the harness's buffers hold where no stage of the submit has written yet. On the GPU that is whatever an
// earlier submit left in a grow-only arena; here every site had one fixed value of its own (0xAA in the output, 0xEEEEEEEE in the flatten
// scratch, 0x55 / 0xEE in the literals, zeros in the record arrays), so a routine that reads such a byte has been checked against one
// history only. emufill::set(v) — zgemu_set_fill / sz_set_fill from Python — replaces those of the arenas a kernel's source runs on by the
// byte v (0 .. 255); a negative v, the default, keeps every site's own value. Not under the fill: temporaries of the serial model itself
// (k_huf's tmp[] in zg_emu.cpp, the plan-only entry point's pos, zg_emu_map.cpp), which no kernel source reads. What the design DEFINES
// stays as it is whatever the fill: the zero pads around the input of zgemu_decode* (the engine's two memsets), what zg_k_reset clears
// (status words, slot logs, max_bits, totals). The seqsize harness's input pads DO follow the fill: its kernel reads the input through a
// buffer resource that ends with the stream, and the harness counts every dword served from outside it — the pads there are what a wrong
// read would return, never zeros by design (its own value is 0x5A; a fill of 0x00 is for that reason not among the tests' fills there).
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

namespace emufill {
inline int g_fill = -1;
inline void set(int v) { g_fill = v < 0 ? -1 : (v & 255); }
inline bool on() { return g_fill >= 0; }
inline uint8_t byte(uint8_t own) { return on() ? (uint8_t)g_fill : own; }
inline uint16_t half(uint16_t own) { return on() ? (uint16_t)(0x0101u * (unsigned)g_fill) : own; }
inline uint32_t word(uint32_t own) { return on() ? 0x01010101u * (uint32_t)g_fill : own; }
// an array of records that was value-initialised (zeros): every byte of it, padding included, becomes the fill
template <class T> inline void records(std::vector<T>& v) { if (on() && !v.empty()) memset((void*)v.data(), g_fill, v.size() * sizeof(T)); }
template <class T> inline void records(T* p, size_t n) { if (on() && n) memset((void*)p, g_fill, n * sizeof(T)); }
}  // namespace emufill
