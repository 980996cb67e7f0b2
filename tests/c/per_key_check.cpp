// per_key_check -- the host-only part of the key-aware compaction
// (splinterdb_amd/csrc/rf_per_key_plan.h) checked on the host: the tile counts, the scratch
// layout (aligned sections that do not overlap, a size that is a multiple of 8 and never shrinks
// as n grows), the widths the kernels rely on, and every refusal of rf_amd_found_per_key /
// _ragged with its neighbouring legal call. Built (with the address and undefined-behaviour
// sanitizers) and run by tests/test_found_per_key_host.py; needs no device. Prints
// "per_key_check: OK".
#include <stdio.h>
#include <string.h>

#include "rf_per_key_plan.h"

using namespace rf;

static int g_failed = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      g_failed++;                                                  \
    }                                                              \
  } while (0)

static void check_layout(uint64_t n) {
  const uint64_t tiles = per_key_tiles(n);
  CHECK(tiles * PER_KEY_TILE >= n && (tiles == 0 || (tiles - 1) * PER_KEY_TILE < n));
  const PerKeyScratch s = per_key_scratch(n);
  CHECK(s.bytes == per_key_scratch_bytes(n));
  CHECK(s.bytes % 8 == 0 && s.bytes >= 8);
  CHECK(s.o_tile_off % 8 == 0 && s.o_tile_cnt % 8 == 0 && s.o_key_cnt % 8 == 0);
  CHECK(s.o_tile_off + 8 * tiles <= s.o_tile_cnt);  // 64-bit offsets, one per tile
  CHECK(s.o_tile_cnt + 4 * tiles <= s.o_key_cnt);   // 32-bit counts, one per tile
  CHECK(s.o_key_cnt + 4 * n <= s.bytes);            // 32-bit counts, one per key
}

static void check_sizing() {
  const uint64_t T = PER_KEY_TILE;
  const uint64_t ns[] = {0, 1, 63, 64, 65, T - 1, T, T + 1, 2381, 3 * T + 77, 1u << 20, (1u << 24) + 1,
                         1ull << 40, (1ull << 56) - 1};
  uint64_t last = 0;
  for (uint64_t n : ns) {
    check_layout(n);
    CHECK(per_key_scratch_bytes(n) >= last);
    last = per_key_scratch_bytes(n);
  }
  for (uint64_t n = 0; n < 5000; n++) {
    check_layout(n);
    CHECK(per_key_scratch_bytes(n + 1) >= per_key_scratch_bytes(n));
  }
  CHECK(per_key_tiles(0) == 0 && per_key_tiles(1) == 1 && per_key_tiles(T) == 1 && per_key_tiles(T + 1) == 2);
  // the widths: a key's and a tile's candidates, and what one key more per tile would need
  CHECK(PER_KEY_MAX_KEY_CANDS == 65535ull * 64 && PER_KEY_MAX_KEY_CANDS < (1ull << 22));
  CHECK(PER_KEY_MAX_TILE_CANDS == (1ull << 32) - 65536);
  CHECK((uint64_t)(PER_KEY_TILE + 1) * PER_KEY_MAX_KEY_CANDS >= (1ull << 32));
}

static void check_refusals() {
  int x;  // any non-null address: nothing is read through it
  void* const P = &x;
  alignas(8) char buf[16];
  void* const S = buf;
  const uint64_t n = 10;
  auto fixed = [&](const void* e, const void* f, const void* m, uint32_t K, uint64_t nn, const void* ko,
                   const void* c, uint64_t cap, const void* cnt, const void* s) {
    return per_key_refusal(false, e, f, m, nullptr, K, nn, ko, c, cap, cnt, s);
  };
  auto ragged = [&](const void* e, const void* f, const void* m, const void* mo, uint64_t nn, const void* ko,
                    const void* c, uint64_t cap, const void* cnt, const void* s) {
    return per_key_refusal(true, e, f, m, mo, 0, nn, ko, c, cap, cnt, s);
  };
  auto has = [](const char* m, const char* what) { return m && strstr(m, what); };
  // the legal calls
  CHECK(!fixed(P, P, P, 4, n, P, P, 8, P, S));
  CHECK(!fixed(P, P, nullptr, 4, n, P, P, 8, P, S));              // d_member NULL: the id is the slot
  CHECK(!fixed(P, P, P, 1, n, P, nullptr, 0, P, S));              // cap 0: d_cand may be NULL
  CHECK(!fixed(P, P, P, 65535, n, P, P, 8, P, S));
  CHECK(!fixed(P, nullptr, nullptr, 4, 0, P, nullptr, 0, P, nullptr));  // n == 0: the outputs it writes only
  CHECK(!fixed(P, P, P, 1, (1ull << 56) - 1, P, P, 8, P, S));
  CHECK(!ragged(P, P, P, P, n, P, P, 8, P, S));
  CHECK(!ragged(P, P, P, P, n, P, nullptr, 0, P, S));
  CHECK(!ragged(P, nullptr, nullptr, nullptr, 0, P, nullptr, 0, P, nullptr));
  // always refused
  CHECK(has(fixed(nullptr, P, P, 4, n, P, P, 8, P, S), "engine"));
  CHECK(has(ragged(nullptr, P, P, P, 0, P, P, 8, P, S), "engine"));
  CHECK(has(fixed(P, P, P, 4, 1ull << 56, P, P, 8, P, S), "2^56"));
  CHECK(has(ragged(P, P, P, P, 1ull << 56, P, P, 8, P, S), "2^56"));
  CHECK(has(fixed(P, P, P, 4, 0, nullptr, P, 8, P, S), "offsets"));
  CHECK(has(fixed(P, P, P, 4, 0, P, P, 8, nullptr, S), "count"));
  CHECK(has(ragged(P, P, P, P, n, nullptr, P, 8, P, S), "offsets"));
  CHECK(has(ragged(P, P, P, P, n, P, P, 8, nullptr, S), "count"));
  CHECK(has(fixed(P, P, P, 4, 0, P, nullptr, 1, P, S), "candidate"));
  CHECK(has(ragged(P, P, P, P, n, P, nullptr, 1, P, S), "candidate"));
  CHECK(has(fixed(P, P, P, 4, n, P, P, 8, P, buf + 4), "aligned"));
  // the fixed form's K, also with n == 0
  CHECK(has(fixed(P, P, P, 0, n, P, P, 8, P, S), "K"));
  CHECK(has(fixed(P, P, P, 0, 0, P, P, 8, P, S), "K"));
  CHECK(has(fixed(P, P, P, 65536, n, P, P, 8, P, S), "K"));
  CHECK(has(fixed(P, P, P, 0xffffffffu, n, P, P, 8, P, S), "K"));
  CHECK(has(fixed(P, P, P, 2, 1ull << 55, P, P, 8, P, S), "n * K"));
  CHECK(!fixed(P, P, P, 2, (1ull << 55) - 1, P, P, 8, P, S));
  CHECK(!ragged(P, P, P, P, n, P, P, 8, P, S));  // the ragged form takes no K
  // with n > 0 only
  CHECK(has(fixed(P, nullptr, P, 4, n, P, P, 8, P, S), "found"));
  CHECK(has(fixed(P, P, P, 4, n, P, P, 8, P, nullptr), "scratch"));
  CHECK(has(ragged(P, nullptr, P, P, n, P, P, 8, P, S), "found"));
  CHECK(has(ragged(P, P, P, P, n, P, P, 8, P, nullptr), "scratch"));
  CHECK(has(ragged(P, P, nullptr, P, n, P, P, 8, P, S), "member"));
  CHECK(has(ragged(P, P, P, nullptr, n, P, P, 8, P, S), "member"));
}

int main() {
  check_sizing();
  check_refusals();
  if (g_failed) {
    printf("per_key_check: %d FAILED\n", g_failed);
    return 1;
  }
  printf("per_key_check: OK\n");
  return 0;
}
