// rf_range_plan.h -- host-only planning of a range map (rf_amd_range_map_create): the
// validation of the caller's table, the packed image that goes to the device in one copy, the
// search accelerator the routing kernel reads, max_list and the scratch size of a route call.
// Plain C++ like rf_set_plan.h: no HIP calls, no engine types -- tests/c/range_plan_check.cpp
// checks it without a GPU. plan_range_map returns 0 or the RF_AMD_E* code with the message in
// *err; a refused call has allocated nothing.
//
// A range map is R ranges cut by R - 1 boundary keys, strictly ascending under the reference's
// default key order (slice_lex_cmp, src/util.h:67-81: unsigned memcmp over the common length,
// then the shorter key first). Range r holds the keys k with boundary[r-1] <= k < boundary[r]:
// r = the number of boundaries <= k, which is find_pivot with less_than_or_equal over the pivots
// (-inf, boundary[0], ...) (src/trunk.c:5886-5932).
//
// The accelerator: each boundary's first 8 bytes as a big-endian uint64, zero-padded. Where two
// prefixes differ their order is slice_lex_cmp's (a padded zero can only lose to a real byte of
// the longer key, which is the lexicographic order), so the prefixes are non-decreasing and a
// key's range lies in [lower bound, upper bound] of its own prefix; only the run of boundaries
// with an equal prefix needs the bytes.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/rf_amd.h"

namespace rf {

constexpr uint32_t RANGE_TILE = 1024;       // keys per scan tile of a route call
constexpr uint32_t RANGE_MAX_LIST = 65535;  // ids per list: the ragged probe's limit
// the most ranges whose R - 1 prefixes the routing kernel keeps in LDS (32 KiB of a workgroup);
// above it the search reads them through L2
constexpr uint32_t RANGE_LDS_RANGES = 4097;

// slice_lex_cmp(a, b) <= 0
inline bool range_key_le(const uint8_t* a, uint64_t al, const uint8_t* b, uint64_t bl) {
  const uint64_t m = al < bl ? al : bl;
  const int c = m ? memcmp(a, b, m) : 0;
  return c ? c < 0 : al <= bl;
}

// the first 8 bytes of a key, big-endian, zero-padded
inline uint64_t range_prefix(const uint8_t* k, uint64_t len) {
  uint64_t p = 0;
  for (uint64_t i = 0; i < 8; i++) p = (p << 8) | (i < len ? k[i] : 0u);
  return p;
}

// The device image, one block: every section starts on an 8-byte boundary.
//   prefix   R - 1 uint64   big-endian 8-byte prefixes of the boundaries
//   boff     R uint64       byte offsets of the boundaries in `bytes`, boff[0] = 0
//   loff     R + 1 uint64   list offsets, loff[0] = 0
//   list     loff[R] uint32 the ids
//   bytes    boff[R-1] bytes
struct RangePlan {
  uint32_t num_ranges = 0, max_list = 0;
  uint64_t o_prefix = 0, o_boff = 0, o_loff = 0, o_list = 0, o_bytes = 0;
  std::vector<uint8_t> image;
};

// the image's sections by device address: what a route launch reads
struct RangeDev {
  uint32_t num_ranges;
  const uint64_t *prefix, *boff, *loff;
  const uint32_t* list;
  const uint8_t* bytes;
};

inline uint64_t range_route_tiles(uint64_t n) { return (n + RANGE_TILE - 1) / RANGE_TILE; }
// 8 bytes of offset and 4 of pair count per tile, and slack to keep both aligned
inline uint64_t range_route_scratch_bytes(uint64_t n) { return ((12 * range_route_tiles(n) + 15) & ~15ull) + 16; }

// what both creates refuse about the R - 1 boundaries of R >= 1 ranges: the message, or nullptr
inline const char* range_bounds_refusal(uint32_t R, const uint8_t* bound_bytes, const uint64_t* bound_off) {
  if (R > 1 && !bound_off) return "null boundary offsets";
  for (uint32_t j = 0; j + 1 < R; j++)
    if (bound_off[j + 1] < bound_off[j]) return "boundary offsets decrease";
  const uint64_t nbytes = R > 1 ? bound_off[R - 1] - bound_off[0] : 0;
  if (nbytes && !bound_bytes) return "null boundary bytes";
  for (uint32_t j = 0; j + 2 < R; j++) {
    const uint64_t a = bound_off[j], b = bound_off[j + 1], c = bound_off[j + 2];
    // strictly ascending: NOT (boundary[j + 1] <= boundary[j])
    if (range_key_le(bound_bytes + b, c - b, bound_bytes + a, b - a)) return "boundaries not strictly ascending";
  }
  return nullptr;
}

inline int plan_range_map(uint32_t num_ranges, const uint8_t* bound_bytes, const uint64_t* bound_off,
                          const uint32_t* list, const uint64_t* list_off, RangePlan* plan, std::string* err) {
  auto refuse = [&](const char* m) {
    if (err) *err = m;
    return RF_AMD_EINVAL;
  };
  if (!plan) return refuse("null plan");
  const uint32_t R = num_ranges;
  if (R == 0) return refuse("num_ranges == 0");
  if (!list_off) return refuse("null list offsets");
  if (const char* m = range_bounds_refusal(R, bound_bytes, bound_off)) return refuse(m);
  const uint64_t nbytes = R > 1 ? bound_off[R - 1] - bound_off[0] : 0;
  uint32_t max_list = 0;
  for (uint32_t r = 0; r < R; r++) {
    if (list_off[r + 1] < list_off[r]) return refuse("list offsets decrease");
    const uint64_t len = list_off[r + 1] - list_off[r];
    if (len > RANGE_MAX_LIST) return refuse("a list longer than 65,535 ids");
    if (len > max_list) max_list = (uint32_t)len;
  }
  const uint64_t nids = list_off[R] - list_off[0];
  if (nids && !list) return refuse("null list");
  // nothing above has written anything
  RangePlan p;
  p.num_ranges = R;
  p.max_list = max_list;
  p.o_prefix = 0;
  p.o_boff = p.o_prefix + 8ull * (R - 1);
  p.o_loff = p.o_boff + 8ull * R;
  p.o_list = p.o_loff + 8ull * (R + 1);
  p.o_bytes = (p.o_list + 4 * nids + 7) & ~7ull;
  p.image.assign(p.o_bytes + nbytes + 8, 0);
  uint64_t* prefix = reinterpret_cast<uint64_t*>(p.image.data() + p.o_prefix);
  uint64_t* boff = reinterpret_cast<uint64_t*>(p.image.data() + p.o_boff);
  uint64_t* loff = reinterpret_cast<uint64_t*>(p.image.data() + p.o_loff);
  for (uint32_t j = 0; j < R; j++) boff[j] = R > 1 ? bound_off[j] - bound_off[0] : 0;
  for (uint32_t j = 0; j + 1 < R; j++)
    prefix[j] = range_prefix(bound_bytes + bound_off[j], bound_off[j + 1] - bound_off[j]);
  for (uint32_t r = 0; r <= R; r++) loff[r] = list_off[r] - list_off[0];
  if (nids) memcpy(p.image.data() + p.o_list, list + list_off[0], 4 * nids);
  if (nbytes) memcpy(p.image.data() + p.o_bytes, bound_bytes + bound_off[0], nbytes);
  *plan = std::move(p);
  return 0;
}

// the host's routing of one key over a plan's image, step for step what the kernel does: upper
// and lower bound of the key's prefix, then the tie run by full compares
inline uint32_t range_route_one(const RangePlan& p, const uint8_t* k, uint64_t len) {
  const uint64_t* prefix = reinterpret_cast<const uint64_t*>(p.image.data() + p.o_prefix);
  const uint64_t* boff = reinterpret_cast<const uint64_t*>(p.image.data() + p.o_boff);
  const uint8_t* bytes = p.image.data() + p.o_bytes;
  const uint32_t nb = p.num_ranges - 1;
  const uint64_t kp = range_prefix(k, len);
  uint32_t lo = 0, hi = nb;
  while (lo < hi) {  // hi = boundaries with prefix <= kp
    const uint32_t mid = lo + (hi - lo) / 2;
    if (prefix[mid] <= kp) lo = mid + 1;
    else hi = mid;
  }
  if (hi == 0 || prefix[hi - 1] != kp) return hi;
  uint32_t a = 0, b = hi;
  while (a < b) {  // a = boundaries with prefix < kp
    const uint32_t mid = a + (b - a) / 2;
    if (prefix[mid] < kp) a = mid + 1;
    else b = mid;
  }
  b = hi;
  while (a < b) {  // boundaries of the tie run that are <= the key
    const uint32_t mid = a + (b - a) / 2;
    if (range_key_le(bytes + boff[mid], boff[mid + 1] - boff[mid], k, len)) a = mid + 1;
    else b = mid;
  }
  return a;
}

}  // namespace rf
