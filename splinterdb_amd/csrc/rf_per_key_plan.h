// rf_per_key_plan.h -- host-only sizing and argument checks of the key-aware compaction
// (rf_amd_found_per_key / _ragged, kernels in rf_per_key.hip). Plain C++ like rf_range_plan.h: no
// HIP calls, no engine types -- tests/c/per_key_check.cpp checks it without a GPU.
//
// A call walks its n keys in tiles of PER_KEY_TILE. Its scratch holds, in this order, one 64-bit
// candidate offset per tile, one 32-bit candidate count per tile and one 32-bit candidate count
// per key; every section starts on an 8-byte boundary.
#pragma once
#include <stdint.h>

#include "rf_range_plan.h"

namespace rf {

constexpr uint32_t PER_KEY_TILE = RANGE_TILE;          // keys per tile: the route call's
constexpr uint32_t PER_KEY_MAX_LIST = RANGE_MAX_LIST;  // ids per key: the ragged probe's limit
constexpr uint64_t PER_KEY_MAX_N = 1ull << 56;         // n (and n * K) stay below it

// A found word has at most 64 values, so a key has at most PER_KEY_MAX_LIST * 64 < 2^22
// candidates and a tile at most PER_KEY_TILE times that: 2^32 - 65,536 for 1,024 keys. The
// per-key and per-tile counts are 32-bit words; a larger tile would not fit.
constexpr uint64_t PER_KEY_MAX_KEY_CANDS = (uint64_t)PER_KEY_MAX_LIST * 64;
constexpr uint64_t PER_KEY_MAX_TILE_CANDS = (uint64_t)PER_KEY_TILE * PER_KEY_MAX_KEY_CANDS;
static_assert(PER_KEY_MAX_KEY_CANDS < (1ull << 22), "a key's candidates fit 22 bits");
static_assert(PER_KEY_MAX_TILE_CANDS < (1ull << 32), "a tile's candidates fit 32 bits");
// a row of 64 keys spans fewer than 2^32 pairs: pair offsets relative to the row are 32-bit
static_assert((uint64_t)64 * PER_KEY_MAX_LIST < (1ull << 32), "a row's pairs fit 32 bits");

inline uint64_t per_key_tiles(uint64_t n) { return (n + PER_KEY_TILE - 1) / PER_KEY_TILE; }

// byte offsets of the scratch sections and the size of the whole
struct PerKeyScratch {
  uint64_t o_tile_off, o_tile_cnt, o_key_cnt, bytes;
};

inline PerKeyScratch per_key_scratch(uint64_t n) {
  const uint64_t tiles = per_key_tiles(n);
  PerKeyScratch s;
  s.o_tile_off = 0;
  s.o_tile_cnt = 8 * tiles;
  s.o_key_cnt = s.o_tile_cnt + ((4 * tiles + 7) & ~7ull);
  s.bytes = s.o_key_cnt + ((4 * n + 7) & ~7ull) + 8;  // never 0: n == 0 has a buffer too
  return s;
}

inline uint64_t per_key_scratch_bytes(uint64_t n) { return per_key_scratch(n).bytes; }

// what both calls refuse, in the header's order: the message, or nullptr. ragged: the form with
// d_member_off; the fixed form takes K.
inline const char* per_key_refusal(bool ragged, const void* engine, const void* d_found, const void* d_member,
                                   const void* d_member_off, uint32_t K, uint64_t n, const void* d_key_off,
                                   const void* d_cand, uint64_t cap, const void* d_count, const void* d_scratch) {
  if (!engine) return "null engine";
  if (n >= PER_KEY_MAX_N) return "n >= 2^56";
  if (!d_key_off || !d_count) return "null key offsets / count";
  if (!ragged && (K == 0 || K > PER_KEY_MAX_LIST)) return "K == 0 or K > 65,535";
  if (!ragged && n > (PER_KEY_MAX_N - 1) / K) return "n * K >= 2^56";
  if (cap && !d_cand) return "null candidate buffer";
  if ((uintptr_t)d_scratch & 7) return "scratch not 8-byte aligned";
  if (n == 0) return nullptr;
  if (!d_found || !d_scratch) return "null found words / scratch";
  if (ragged && (!d_member || !d_member_off)) return "null member ids / offsets";
  return nullptr;
}

}  // namespace rf
