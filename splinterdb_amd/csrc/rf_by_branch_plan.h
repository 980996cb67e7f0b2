// rf_by_branch_plan.h -- host-only sizing and argument checks of the group-by-branch call
// (rf_amd_found_by_branch, kernels in rf_by_branch.hip). Plain C++ like rf_per_key_plan.h: no HIP
// calls, no engine types -- tests/c/by_branch_check.cpp checks it without a GPU.
//
// The call is a least-significant-digit radix sort of the records' 32-bit sort keys, stable, in
// digits of BY_BRANCH_DIGIT_BITS bits, over tiles of BY_BRANCH_TILE records. The sort key of a
// record c is ((c >> 8) & (2^mb - 1)) << 6 | (c & 63) with mb the bit width of num_members - 1: mb
// + 6 bits, at most 32. Its scratch holds, in this order, two record buffers of cap 64-bit
// (key32 << 32 | index32) pairs that the passes ping-pong between, one 32-bit count per (digit,
// tile), one 32-bit offset per (digit, tile), and one 32-bit total and one 32-bit offset per chunk
// of BY_BRANCH_SCAN_CHUNK counts (a pass's scan has two levels); every section starts on an 8-byte
// boundary. The run table's per-tile head counts and offsets reuse the first words of the count
// and offset sections.
#pragma once
#include <stdint.h>

namespace rf {

constexpr uint32_t BY_BRANCH_TILE = 4096;       // records per tile
constexpr uint32_t BY_BRANCH_DIGIT_BITS = 8;    // bits per pass
constexpr uint32_t BY_BRANCH_BINS = 1u << BY_BRANCH_DIGIT_BITS;
constexpr uint32_t BY_BRANCH_SCAN_CHUNK = 8192;  // counts per workgroup of the scan's first level
constexpr uint32_t BY_BRANCH_VALUE_BITS = 6;    // a found word has 64 values
constexpr uint32_t BY_BRANCH_MAX_MEMBERS = 1u << 26;
constexpr uint64_t BY_BRANCH_MAX_CAP = (1ull << 32) - 1;  // cap stays at or below it

// every 32-bit quantity of the kernels: a tile's digit count, a record's position (below cap), the
// index of a (digit, tile) count of the largest cap, and the key of the largest num_members
static_assert(BY_BRANCH_TILE < (1ull << 32), "a tile's count fits 32 bits");
static_assert(BY_BRANCH_MAX_CAP < (1ull << 32), "positions and record indices fit 32 bits");
static_assert(((BY_BRANCH_MAX_CAP + BY_BRANCH_TILE - 1) / BY_BRANCH_TILE) * BY_BRANCH_BINS < (1ull << 32),
              "the counts array of the largest cap is indexed in 32 bits");
static_assert(26 + BY_BRANCH_VALUE_BITS <= 32, "the sort key of 2^26 members fits 32 bits");
static_assert(BY_BRANCH_TILE % 256 == 0, "whole records per thread of a 256-thread workgroup");

// bit width of num_members - 1 (0 for one member); num_members >= 1
inline uint32_t by_branch_member_bits(uint32_t num_members) {
  uint32_t mb = 0;
  for (uint32_t x = num_members - 1; x; x >>= 1) mb++;
  return mb;
}
inline uint32_t by_branch_key_bits(uint32_t num_members) {
  return by_branch_member_bits(num_members) + BY_BRANCH_VALUE_BITS;
}
// digit passes of the sort: 1 up to 4 members, 2 up to 1,024, 3 up to 2^18, 4 up to 2^26
inline uint32_t by_branch_passes(uint32_t num_members) {
  return (by_branch_key_bits(num_members) + BY_BRANCH_DIGIT_BITS - 1) / BY_BRANCH_DIGIT_BITS;
}
// stream-ordered launches of one call: four per digit pass (histogram, the scan's two levels,
// scatter) and three for the run table
inline uint32_t by_branch_launches(uint32_t num_members) { return 4 * by_branch_passes(num_members) + 3; }

// constexpr: the kernels call it too, on the record count they read
constexpr uint64_t by_branch_tiles(uint64_t cap) { return (cap + BY_BRANCH_TILE - 1) / BY_BRANCH_TILE; }

constexpr uint64_t by_branch_scan_chunks(uint64_t counts) {
  return (counts + BY_BRANCH_SCAN_CHUNK - 1) / BY_BRANCH_SCAN_CHUNK;
}

// byte offsets of the scratch sections and the size of the whole
struct ByBranchScratch {
  uint64_t o_buf_a, o_buf_b, o_cnt, o_off, o_chunk_tot, o_chunk_off, bytes;
};

inline ByBranchScratch by_branch_scratch(uint64_t cap) {
  const uint64_t words = by_branch_tiles(cap) * BY_BRANCH_BINS;  // 32-bit, an even number
  ByBranchScratch s;
  s.o_buf_a = 0;
  s.o_buf_b = 8 * cap;
  s.o_cnt = 16 * cap;
  s.o_off = s.o_cnt + 4 * words;
  const uint64_t cbytes = (4 * by_branch_scan_chunks(words) + 7) & ~7ull;
  s.o_chunk_tot = s.o_off + 4 * words;
  s.o_chunk_off = s.o_chunk_tot + cbytes;
  s.bytes = s.o_chunk_off + cbytes + 8;  // never 0: cap == 0 has a buffer too
  return s;
}

// num_members is not part of the layout: the sections are sized for any pass count
inline uint64_t by_branch_scratch_bytes(uint64_t cap, uint32_t num_members) {
  (void)num_members;
  return by_branch_scratch(cap).bytes;
}

// what the call refuses, in the header's order: the message, or nullptr
inline const char* by_branch_refusal(const void* engine, const void* d_cand, const void* d_cand_key,
                                     const void* d_count, uint64_t cap, uint32_t num_members, const void* d_order,
                                     const void* d_order_key, const void* d_branch, const void* d_branch_off,
                                     uint64_t branch_cap, const void* d_num_branches, const void* d_scratch) {
  if (!engine) return "null engine";
  if (!d_count || !d_num_branches) return "null count / number of branches";
  if (num_members == 0 || num_members > BY_BRANCH_MAX_MEMBERS) return "num_members == 0 or > 2^26";
  if (cap > BY_BRANCH_MAX_CAP) return "cap >= 2^32";
  if (cap && (!d_cand || !d_order || !d_scratch)) return "null records / order / scratch";
  if (branch_cap && (!d_branch || !d_branch_off)) return "null branch table";
  if ((uintptr_t)d_scratch & 7) return "scratch not 8-byte aligned";
  if (!d_cand_key != !d_order_key) return "d_cand_key and d_order_key: both or neither";
  return nullptr;
}

}  // namespace rf
