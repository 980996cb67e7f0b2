// advance_check -- the host-only part of the stepwise hand-out
// (splinterdb_amd/csrc/rf_advance_plan.h) checked on the host: the scratch layout (aligned sections
// that do not overlap, a size that is a multiple of 8, never 0 and never shrinks as n grows), the
// take of one key against its definition, the widths the kernels rely on, and every refusal of
// rf_amd_found_advance in the header's order, each beside its neighbouring legal call. Built (with
// the address and undefined-behaviour sanitizers) and run by tests/test_advance_plan.py; needs no
// device. Prints "advance_check: OK".
#include <stdio.h>
#include <string.h>

#include "rf_advance_plan.h"

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
  const AdvanceScratch s = advance_scratch(n);
  CHECK(s.bytes == advance_scratch_bytes(n));
  CHECK(s.bytes % 8 == 0 && s.bytes >= 8);
  CHECK(s.o_tile_off % 8 == 0 && s.o_tile_cnt % 8 == 0);
  CHECK(s.o_tile_off + 8 * tiles <= s.o_tile_cnt);  // 64-bit offsets, one per tile
  CHECK(s.o_tile_cnt + 4 * tiles <= s.bytes);       // 32-bit counts, one per tile
}

static void check_sizing() {
  const uint64_t T = PER_KEY_TILE;
  const uint64_t ns[] = {0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 77, 1u << 20, (1u << 24) + 1,
                         1ull << 40, PER_KEY_MAX_N - 1};
  uint64_t last = 0;
  for (uint64_t n : ns) {
    check_layout(n);
    CHECK(advance_scratch_bytes(n) >= last);
    last = advance_scratch_bytes(n);
  }
  for (uint64_t n = 0; n < 5 * T; n++) {
    check_layout(n);
    CHECK(advance_scratch_bytes(n + 1) >= advance_scratch_bytes(n));
  }
  CHECK(advance_scratch_bytes(0) == 8);
  // the widths: a tile of keys that all take the most, and a row of them, stay in 32 bits
  CHECK(ADVANCE_MAX_TAKE == 65535ull * 64);
  CHECK(PER_KEY_TILE * ADVANCE_MAX_TAKE < (1ull << 32) && 64 * ADVANCE_MAX_TAKE < (1ull << 32));
  CHECK(ADVANCE_FIRST == 1u && ADVANCE_FLAGS == 1u);
}

// the definition, word for word
static uint64_t take_by_definition(uint64_t off, uint64_t end, uint32_t cursor, bool done, uint64_t cand_cap,
                                   uint32_t width) {
  const unsigned __int128 a = (unsigned __int128)off + cursor;
  const uint64_t e = end < cand_cap ? end : cand_cap;
  if (done || a >= e) return 0;
  uint64_t t = e - (uint64_t)a;
  if (width < t) t = width;
  if (65535ull * 64 < t) t = 65535ull * 64;
  return t;
}

static void check_take() {
  const uint64_t offs[] = {0, 1, 5, 1000, 1ull << 32, (1ull << 56) - 3, ~0ull - 5};
  const uint64_t lens[] = {0, 1, 2, 3, 64, 5000, 65535ull * 64 - 1, 65535ull * 64, 65535ull * 64 + 1, 1ull << 33};
  const uint32_t curs[] = {0, 1, 2, 3, 63, 4999, 5000, 5001, 0xFFFFFFFFu};
  const uint32_t widths[] = {1, 2, 3, 64, 65535u * 64, 0xFFFFFFFFu};
  for (uint64_t off : offs)
    for (uint64_t len : lens) {
      const uint64_t end = off + len < off ? ~0ull : off + len;
      const uint64_t caps[] = {0, off, off + 1, off + len / 2, end, end + 1, ~0ull};
      for (uint32_t cur : curs)
        for (uint32_t w : widths)
          for (uint64_t cap : caps)
            for (int done = 0; done < 2; done++) {
              const uint32_t t = advance_take(off, end, cur, done != 0, cap, w);
              CHECK(t == take_by_definition(off, end, cur, done != 0, cap, w));
              CHECK(t <= w && t <= ADVANCE_MAX_TAKE);
              if (t) CHECK(!done && off + cur + t <= end && off + cur + t <= cap);  // every read below both
            }
    }
  // offsets that run backwards take nothing
  CHECK(advance_take(10, 5, 0, false, 100, 4) == 0);
  CHECK(advance_take(3, 8, 2, false, 100, 1) == 1 && advance_take(3, 8, 5, false, 100, 1) == 0);
  CHECK(advance_take(3, 8, 0, false, 5, 64) == 2 && advance_take(3, 8, 0, false, 3, 64) == 0);
}

static void check_refusals() {
  int x;  // any non-null address: nothing is read through it
  void* const P = &x;
  alignas(8) char buf[16];
  void* const S = buf;
  const uint64_t cc = 100, oc = 10, n = 7;
  // the legal calls
  CHECK(advance_refusal(P, P, P, cc, n, 1, 0, P, P, oc, P, S) == nullptr);
  CHECK(advance_refusal(P, P, P, cc, n, 0xFFFFFFFFu, ADVANCE_FIRST, P, P, oc, P, S) == nullptr);
  CHECK(advance_refusal(P, P, P, cc, PER_KEY_MAX_N - 1, 1, 0, P, P, oc, P, S) == nullptr);
  CHECK(advance_refusal(P, P, P, cc, n, 1, 0, P, nullptr, 0, P, S) == nullptr);        // out_cap 0: no output
  CHECK(advance_refusal(P, P, nullptr, 0, n, 1, 0, P, P, oc, P, S) == nullptr);        // cand_cap 0: no records
  CHECK(advance_refusal(P, nullptr, nullptr, cc, 0, 1, 0, nullptr, P, oc, P, nullptr) == nullptr);  // n == 0
  CHECK(advance_refusal(P, nullptr, nullptr, cc, 0, 1, 0, nullptr, nullptr, 0, P, nullptr) == nullptr);
  // each refusal
  const char* m;
  m = advance_refusal(nullptr, P, P, cc, n, 1, 0, P, P, oc, P, S);
  CHECK(m && strstr(m, "engine"));
  m = advance_refusal(P, P, P, cc, PER_KEY_MAX_N, 1, 0, P, P, oc, P, S);
  CHECK(m && strstr(m, "2^56"));
  m = advance_refusal(P, P, P, cc, n, 0, 0, P, P, oc, P, S);
  CHECK(m && strstr(m, "width"));
  m = advance_refusal(P, P, P, cc, n, 1, 2, P, P, oc, P, S);
  CHECK(m && strstr(m, "flag"));
  m = advance_refusal(P, P, P, cc, n, 1, ADVANCE_FIRST | 0x80000000u, P, P, oc, P, S);
  CHECK(m && strstr(m, "flag"));
  m = advance_refusal(P, P, P, cc, n, 1, 0, P, P, oc, nullptr, S);
  CHECK(m && strstr(m, "count"));
  m = advance_refusal(P, P, P, cc, n, 1, 0, P, nullptr, oc, P, S);
  CHECK(m && strstr(m, "output records"));
  m = advance_refusal(P, P, P, cc, n, 1, 0, P, P, oc, P, buf + 4);
  CHECK(m && strstr(m, "aligned"));
  m = advance_refusal(P, nullptr, nullptr, cc, 0, 1, 0, nullptr, P, oc, P, buf + 4);  // with n == 0 too
  CHECK(m && strstr(m, "aligned"));
  m = advance_refusal(P, nullptr, P, cc, n, 1, 0, P, P, oc, P, S);
  CHECK(m && strstr(m, "key offsets"));
  m = advance_refusal(P, P, P, cc, n, 1, 0, nullptr, P, oc, P, S);
  CHECK(m && strstr(m, "cursors"));
  m = advance_refusal(P, P, P, cc, n, 1, 0, P, P, oc, P, nullptr);
  CHECK(m && strstr(m, "scratch"));
  m = advance_refusal(P, P, nullptr, cc, n, 1, 0, P, P, oc, P, S);
  CHECK(m && strstr(m, "candidate records"));
  // the order of the header: each refusal wins over every later one
  m = advance_refusal(nullptr, nullptr, nullptr, cc, PER_KEY_MAX_N, 0, 2, nullptr, nullptr, oc, nullptr, buf + 4);
  CHECK(m && strstr(m, "engine"));
  m = advance_refusal(P, nullptr, nullptr, cc, PER_KEY_MAX_N, 0, 2, nullptr, nullptr, oc, nullptr, buf + 4);
  CHECK(m && strstr(m, "2^56"));
  m = advance_refusal(P, nullptr, nullptr, cc, n, 0, 2, nullptr, nullptr, oc, nullptr, buf + 4);
  CHECK(m && strstr(m, "width"));
  m = advance_refusal(P, nullptr, nullptr, cc, n, 1, 2, nullptr, nullptr, oc, nullptr, buf + 4);
  CHECK(m && strstr(m, "flag"));
  m = advance_refusal(P, nullptr, nullptr, cc, n, 1, 0, nullptr, nullptr, oc, nullptr, buf + 4);
  CHECK(m && strstr(m, "count"));
  m = advance_refusal(P, nullptr, nullptr, cc, n, 1, 0, nullptr, nullptr, oc, P, buf + 4);
  CHECK(m && strstr(m, "output records"));
  m = advance_refusal(P, nullptr, nullptr, cc, n, 1, 0, nullptr, P, oc, P, buf + 4);
  CHECK(m && strstr(m, "aligned"));
  m = advance_refusal(P, nullptr, nullptr, cc, n, 1, 0, nullptr, P, oc, P, S);
  CHECK(m && strstr(m, "key offsets"));
}

int main() {
  check_sizing();
  check_take();
  check_refusals();
  if (g_failed) {
    printf("advance_check: %d checks failed\n", g_failed);
    return 1;
  }
  printf("advance_check: OK\n");
  return 0;
}
