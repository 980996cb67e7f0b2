// by_branch_check -- the host-only part of the group-by-branch call
// (splinterdb_amd/csrc/rf_by_branch_plan.h) checked on the host: the key width and pass count on
// both sides of every num_members at which the count changes, the launches, the scratch layout
// (aligned sections that do not overlap, a size that is a multiple of 8 and never shrinks as cap
// grows), the widths the kernels rely on, and every refusal of rf_amd_found_by_branch with its
// neighbouring legal call. Built (with the address and undefined-behaviour sanitizers) and run by
// tests/test_by_branch_plan.py; needs no device. Prints "by_branch_check: OK".
#include <stdio.h>
#include <string.h>

#include "rf_by_branch_plan.h"

using namespace rf;

static int g_failed = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      g_failed++;                                                  \
    }                                                              \
  } while (0)

// the definition, not the formula: the least number of bits that hold every id below num_members
static uint32_t bits_by_search(uint32_t num_members) {
  uint32_t b = 0;
  while (((uint64_t)1 << b) < num_members) b++;
  return b;
}

static void check_passes() {
  CHECK(by_branch_member_bits(1) == 0 && by_branch_member_bits(2) == 1 && by_branch_member_bits(3) == 2);
  CHECK(by_branch_member_bits(4) == 2 && by_branch_member_bits(5) == 3);
  CHECK(by_branch_member_bits(1u << 26) == 26 && by_branch_key_bits(1u << 26) == 32);
  for (uint32_t nm = 1; nm < 70000; nm++) CHECK(by_branch_member_bits(nm) == bits_by_search(nm));
  for (uint32_t b = 17; b <= 26; b++) {
    CHECK(by_branch_member_bits(1u << b) == b);
    CHECK(b == 26 || by_branch_member_bits((1u << b) + 1) == b + 1);
  }
  // the boundaries: the key grows past 8, 16 and 24 bits behind 4, 1,024 and 2^18 members
  const uint32_t last_of[] = {4, 1024, 1u << 18, 1u << 26};
  uint32_t first = 1;
  for (uint32_t p = 0; p < 4; p++) {
    CHECK(by_branch_passes(first) == p + 1);
    CHECK(by_branch_passes(last_of[p]) == p + 1);
    CHECK(by_branch_key_bits(last_of[p]) == 8 * (p + 1));
    if (p < 3) CHECK(by_branch_passes(last_of[p] + 1) == p + 2);
    CHECK(by_branch_launches(last_of[p]) == 4 * (p + 1) + 3);
    first = last_of[p] + 1;
  }
  // never fewer passes for more members, and every key bit lies in some pass
  uint32_t last = 0;
  for (uint32_t nm = 1; nm <= (1u << 26); nm = nm < 3000 ? nm + 1 : nm + nm / 3) {
    const uint32_t p = by_branch_passes(nm);
    CHECK(p >= last && p >= 1 && p <= 4);
    CHECK(p * BY_BRANCH_DIGIT_BITS >= by_branch_key_bits(nm));
    CHECK((p - 1) * BY_BRANCH_DIGIT_BITS < by_branch_key_bits(nm));
    last = p;
  }
}

static void check_layout(uint64_t cap) {
  const uint64_t tiles = by_branch_tiles(cap);
  CHECK(tiles * BY_BRANCH_TILE >= cap && (tiles == 0 || (tiles - 1) * BY_BRANCH_TILE < cap));
  const ByBranchScratch s = by_branch_scratch(cap);
  CHECK(s.bytes == by_branch_scratch_bytes(cap, 1) && s.bytes == by_branch_scratch_bytes(cap, 1u << 26));
  CHECK(s.bytes % 8 == 0 && s.bytes >= 8);
  CHECK(s.o_buf_a % 8 == 0 && s.o_buf_b % 8 == 0 && s.o_cnt % 8 == 0 && s.o_off % 8 == 0);
  CHECK(s.o_buf_a + 8 * cap <= s.o_buf_b);                      // 64-bit pairs, one per record
  CHECK(s.o_buf_b + 8 * cap <= s.o_cnt);                        // the same, the other side
  CHECK(s.o_cnt + 4 * tiles * BY_BRANCH_BINS <= s.o_off);       // 32-bit counts per (digit, tile)
  CHECK(s.o_off + 4 * tiles * BY_BRANCH_BINS <= s.o_chunk_tot);  // 32-bit offsets per (digit, tile)
  const uint64_t chunks = by_branch_scan_chunks(tiles * BY_BRANCH_BINS);
  CHECK(chunks * BY_BRANCH_SCAN_CHUNK >= tiles * BY_BRANCH_BINS);
  CHECK(s.o_chunk_tot % 8 == 0 && s.o_chunk_off % 8 == 0);
  CHECK(s.o_chunk_tot + 4 * chunks <= s.o_chunk_off);           // 32-bit totals per scan chunk
  CHECK(s.o_chunk_off + 4 * chunks <= s.bytes);                 // 32-bit offsets per scan chunk
  CHECK(tiles <= tiles * BY_BRANCH_BINS);                       // the run table's tile words fit both
}

static void check_sizing() {
  const uint64_t T = BY_BRANCH_TILE;
  const uint64_t caps[] = {0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 77, 1u << 20, (1u << 24) + 1,
                           1ull << 31, BY_BRANCH_MAX_CAP};
  uint64_t last = 0;
  for (uint64_t cap : caps) {
    check_layout(cap);
    CHECK(by_branch_scratch_bytes(cap, 7) >= last);
    last = by_branch_scratch_bytes(cap, 7);
  }
  for (uint64_t cap = 0; cap < 3 * T; cap++) {
    check_layout(cap);
    CHECK(by_branch_scratch_bytes(cap + 1, 1) >= by_branch_scratch_bytes(cap, 1));
  }
  CHECK(by_branch_tiles(0) == 0 && by_branch_tiles(1) == 1 && by_branch_tiles(T) == 1 && by_branch_tiles(T + 1) == 2);
  // the widths: the index of the last count of the largest cap, and the largest key
  CHECK(BY_BRANCH_MAX_CAP == 0xFFFFFFFFull && BY_BRANCH_BINS == 256);
  CHECK(by_branch_tiles(BY_BRANCH_MAX_CAP) * BY_BRANCH_BINS < (1ull << 32));
  CHECK(by_branch_key_bits(BY_BRANCH_MAX_MEMBERS) == 32);
}

static void check_refusals() {
  int x;  // any non-null address: nothing is read through it
  void* const P = &x;
  alignas(8) char buf[16];
  void* const S = buf;
  const uint64_t cap = 100, bc = 10;
  // the legal calls
  CHECK(by_branch_refusal(P, P, P, P, cap, 5, P, P, P, P, bc, P, S) == nullptr);
  CHECK(by_branch_refusal(P, P, nullptr, P, cap, 5, P, nullptr, P, P, bc, P, S) == nullptr);
  CHECK(by_branch_refusal(P, P, P, P, cap, 1, P, P, P, P, bc, P, S) == nullptr);
  CHECK(by_branch_refusal(P, P, P, P, cap, 1u << 26, P, P, P, P, bc, P, S) == nullptr);
  CHECK(by_branch_refusal(P, P, P, P, BY_BRANCH_MAX_CAP, 5, P, P, P, P, bc, P, S) == nullptr);
  CHECK(by_branch_refusal(P, nullptr, nullptr, P, 0, 5, nullptr, nullptr, P, P, bc, P, nullptr) == nullptr);
  CHECK(by_branch_refusal(P, P, P, P, cap, 5, P, P, nullptr, nullptr, 0, P, S) == nullptr);
  // each refusal
  const char* m;
  m = by_branch_refusal(nullptr, P, P, P, cap, 5, P, P, P, P, bc, P, S);
  CHECK(m && strstr(m, "engine"));
  m = by_branch_refusal(P, P, P, nullptr, cap, 5, P, P, P, P, bc, P, S);
  CHECK(m && strstr(m, "count"));
  m = by_branch_refusal(P, P, P, P, cap, 5, P, P, P, P, bc, nullptr, S);
  CHECK(m && strstr(m, "number of branches"));
  m = by_branch_refusal(P, P, P, P, cap, 0, P, P, P, P, bc, P, S);
  CHECK(m && strstr(m, "num_members"));
  m = by_branch_refusal(P, P, P, P, cap, (1u << 26) + 1, P, P, P, P, bc, P, S);
  CHECK(m && strstr(m, "num_members"));
  m = by_branch_refusal(P, P, P, P, 1ull << 32, 5, P, P, P, P, bc, P, S);
  CHECK(m && strstr(m, "cap"));
  m = by_branch_refusal(P, nullptr, P, P, cap, 5, P, P, P, P, bc, P, S);
  CHECK(m && strstr(m, "records"));
  m = by_branch_refusal(P, P, P, P, cap, 5, nullptr, P, P, P, bc, P, S);
  CHECK(m && strstr(m, "order"));
  m = by_branch_refusal(P, P, P, P, cap, 5, P, P, P, P, bc, P, nullptr);
  CHECK(m && strstr(m, "scratch"));
  m = by_branch_refusal(P, P, P, P, cap, 5, P, P, nullptr, P, bc, P, S);
  CHECK(m && strstr(m, "branch table"));
  m = by_branch_refusal(P, P, P, P, cap, 5, P, P, P, nullptr, bc, P, S);
  CHECK(m && strstr(m, "branch table"));
  m = by_branch_refusal(P, P, P, P, cap, 5, P, P, P, P, bc, P, buf + 4);
  CHECK(m && strstr(m, "aligned"));
  m = by_branch_refusal(P, P, nullptr, P, cap, 5, P, P, P, P, bc, P, S);
  CHECK(m && strstr(m, "both or neither"));
  m = by_branch_refusal(P, P, P, P, cap, 5, P, nullptr, P, P, bc, P, S);
  CHECK(m && strstr(m, "both or neither"));
  // the order of the header: the engine before everything, the count before num_members
  m = by_branch_refusal(nullptr, nullptr, nullptr, nullptr, 1ull << 32, 0, nullptr, nullptr, nullptr, nullptr, bc,
                        nullptr, buf + 4);
  CHECK(m && strstr(m, "engine"));
  m = by_branch_refusal(P, P, P, nullptr, cap, 0, P, P, P, P, bc, P, S);
  CHECK(m && strstr(m, "count"));
}

int main() {
  check_passes();
  check_sizing();
  check_refusals();
  if (g_failed) {
    printf("by_branch_check: %d checks failed\n", g_failed);
    return 1;
  }
  printf("by_branch_check: OK\n");
  return 0;
}
