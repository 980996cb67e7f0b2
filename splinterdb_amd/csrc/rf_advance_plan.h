// rf_advance_plan.h -- host-only sizing and argument checks of the stepwise hand-out of per-key
// candidates (rf_amd_found_advance, kernels in rf_advance.hip). Plain C++ like rf_per_key_plan.h:
// no HIP calls, no engine types -- tests/c/advance_check.cpp checks it without a GPU.
//
// A call walks its n keys in tiles of PER_KEY_TILE, the tile of the call that wrote the CSR. Its
// scratch holds, in this order, one 64-bit output offset per tile and one 32-bit record count per
// tile; both sections start on an 8-byte boundary. Nothing is kept per key: the emit kernel reads
// the offsets, the cursor and the done byte again (13 bytes a key) where a parked 32-bit take would
// cost a 4-byte store and a 4-byte load and still need the offset and the cursor for the source.
#pragma once
#include <stdint.h>

#include "rf_per_key_plan.h"

namespace rf {

constexpr uint32_t ADVANCE_FIRST = 1u;            // RF_AMD_ADVANCE_FIRST
constexpr uint32_t ADVANCE_FLAGS = ADVANCE_FIRST;  // every flag the call knows

// A key takes at most PER_KEY_MAX_KEY_CANDS records per call, whatever width and the offsets say:
// the call does not validate the offsets, and the bound keeps a tile's sum in its 32-bit word.
constexpr uint64_t ADVANCE_MAX_TAKE = PER_KEY_MAX_KEY_CANDS;
static_assert((uint64_t)PER_KEY_TILE * ADVANCE_MAX_TAKE < (1ull << 32), "a tile's records fit 32 bits");
static_assert((uint64_t)64 * ADVANCE_MAX_TAKE < (1ull << 32), "a row's records fit 32 bits");

// the records key i takes: off = d_key_off[i], end = d_key_off[i + 1], cursor = d_cursor[i] (0
// under FIRST), done = the key's byte (0 without d_done). The kernels and the check program call
// this one function.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t advance_take(uint64_t off, uint64_t end, uint32_t cursor, bool done, uint64_t cand_cap,
                             uint32_t width) {
  const uint64_t a = off + cursor, e = end < cand_cap ? end : cand_cap;
  if (done || a >= e || a < off) return 0;  // a < off: the sum wrapped, on offsets nobody wrote
  uint64_t t = e - a;
  if (t > width) t = width;
  if (t > ADVANCE_MAX_TAKE) t = ADVANCE_MAX_TAKE;
  return (uint32_t)t;
}

// byte offsets of the scratch sections and the size of the whole
struct AdvanceScratch {
  uint64_t o_tile_off, o_tile_cnt, bytes;
};

inline AdvanceScratch advance_scratch(uint64_t n) {
  const uint64_t tiles = per_key_tiles(n);
  AdvanceScratch s;
  s.o_tile_off = 0;
  s.o_tile_cnt = 8 * tiles;
  s.bytes = s.o_tile_cnt + ((4 * tiles + 7) & ~7ull) + 8;  // never 0: n == 0 has a buffer too
  return s;
}

inline uint64_t advance_scratch_bytes(uint64_t n) { return advance_scratch(n).bytes; }

// what the call refuses, in the header's order: the message, or nullptr
inline const char* advance_refusal(const void* engine, const void* d_key_off, const void* d_cand, uint64_t cand_cap,
                                   uint64_t n, uint32_t width, uint32_t flags, const void* d_cursor,
                                   const void* d_out_cand, uint64_t out_cap, const void* d_out_count,
                                   const void* d_scratch) {
  if (!engine) return "null engine";
  if (n >= PER_KEY_MAX_N) return "n >= 2^56";
  if (width == 0) return "width == 0";
  if (flags & ~ADVANCE_FLAGS) return "unknown flag bits";
  if (!d_out_count) return "null output count";
  if (out_cap && !d_out_cand) return "null output records";
  if ((uintptr_t)d_scratch & 7) return "scratch not 8-byte aligned";
  if (n == 0) return nullptr;
  if (!d_key_off || !d_cursor || !d_scratch) return "null key offsets / cursors / scratch";
  if (cand_cap && !d_cand) return "null candidate records";
  return nullptr;
}

}  // namespace rf
