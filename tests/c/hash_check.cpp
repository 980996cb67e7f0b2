// hash_check -- the global-memory XXH32 helpers of splinterdb_amd/csrc/rf_device.h, run on the
// host. Built (with the address and undefined-behaviour sanitizers) and run by
// tests/test_key_hash_host.py; makes no HIP call and needs no device.
//
// For every key length 0..300 and four seeds, each helper that applies to the length is compared
// with a byte-at-a-time XXH32 written here. Every key is its own malloc(len) -- or, for a base
// that is not 16-byte aligned, the last len bytes of a malloc(shift + len) -- so a load past the
// key's last byte is a heap overflow the sanitizer reports: the header's claim that every load
// stays inside the key's own bytes is checked, not only the hash values. The dispatch is checked
// the same way: fixed_kind() (rf_plan.h) picks the reader of several keys laid back to back, and a
// reader whose loads are less aligned than it needs, or run past the last key, stops the run.
// Prints "ref <len> <seed> <hash>" for a handful of lengths (compared with the CPU oracle by the
// test, which rebuilds the same key bytes), then "hash_check: OK".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rf_device.h"
#include "rf_plan.h"

static int g_failed = 0;

// byte i of the check's key of length len (tests/test_key_hash_host.py: key_bytes)
static uint8_t key_byte(uint32_t len, uint32_t i) { return (uint8_t)(((i + 1) * 2654435761u + len * 40503u) >> 24); }

static uint32_t rd32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
static uint32_t rol(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// XXH32 as published, one byte at a time (own constants: nothing shared with the header)
static uint32_t xxh32_bytes(const uint8_t* p, uint32_t len, uint32_t seed) {
  const uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
  uint32_t h, i = 0;
  if (len >= 16) {
    uint32_t v[4] = {seed + P1 + P2, seed + P2, seed, seed - P1};
    for (; i + 16 <= len; i += 16)
      for (int k = 0; k < 4; k++) v[k] = rol(v[k] + rd32(p + i + 4 * k) * P2, 13) * P1;
    h = rol(v[0], 1) + rol(v[1], 7) + rol(v[2], 12) + rol(v[3], 18);
  } else {
    h = seed + P5;
  }
  h += len;
  for (; i + 4 <= len; i += 4) h = rol(h + rd32(p + i) * P3, 17) * P4;
  for (; i < len; i++) h = rol(h + p[i] * P5, 11) * P1;
  h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
  return h;
}

static void expect(const char* what, uint32_t len, uint32_t shift, uint32_t seed, uint32_t got, uint32_t want) {
  if (got != want) {
    if (g_failed < 20) printf("MISMATCH %s len %u shift %u seed %u: %08x, want %08x\n", what, len, shift, seed, got, want);
    g_failed++;
  }
}

int main() {
  const uint32_t seeds[4] = {42u, 0u, 0xFFFFFFFFu, 7u};
  const uint32_t shifts[6] = {0, 1, 2, 3, 4, 8};
  const uint32_t ref_lens[] = {1, 3, 4, 15, 16, 17, 24, 31, 33, 100, 127, 128, 129, 300};
  uint32_t checks = 0;
  for (uint32_t len = 0; len <= 300; len++) {
    for (uint32_t shift : shifts) {
      uint8_t* block = static_cast<uint8_t*>(malloc(shift + len));  // the key ends where the block ends
      if (!block && shift + len) return 2;
      uint8_t* key = block + shift;
      for (uint32_t i = 0; i < shift; i++) block[i] = 0xA5;
      for (uint32_t i = 0; i < len; i++) key[i] = key_byte(len, i);
      for (uint32_t seed : seeds) {
        const uint32_t want = xxh32_bytes(key, len, seed);
        expect("xxh32_unaligned", len, shift, seed, rf::xxh32_unaligned(key, len, seed), want);
        expect("xxh32_unaligned_prefetch", len, shift, seed, rf::xxh32_unaligned_prefetch(key, len, seed), want);
        checks += 2;
        if (len % 4 == 0 && shift % 4 == 0) {  // IN_KEYS_W: whole words from a 4-byte aligned base
          expect("xxh32_words", len, shift, seed, rf::xxh32_words(reinterpret_cast<const uint32_t*>(key), len, seed), want);
          checks++;
        }
        if (len == 24 && shift % 4 == 0) {  // IN_KEYS24: the key's six words
          expect("xxh32_24", len, shift, seed, rf::xxh32_24(reinterpret_cast<const uint32_t*>(key), seed), want);
          checks++;
        }
        if (shift == 0)
          for (uint32_t rl : ref_lens)
            if (rl == len) printf("ref %u %u %u\n", len, seed, want);
      }
      free(block);
    }
  }
  // The dispatch: NKEYS keys back to back at each base, every key hashed by the reader that
  // fixed_kind() picks for the base, with the loads hash_key (rf_kernels.hip) makes for it. A
  // reader picked for a length that leaves key k = 1.. less aligned than it needs is a misaligned
  // load here, and one that reads whole words past an odd tail leaves the last key's block.
  constexpr uint32_t NKEYS = 5;
  for (uint32_t len = 1; len <= 300; len++) {
    for (uint32_t shift : shifts) {
      uint8_t* block = static_cast<uint8_t*>(malloc(shift + NKEYS * len));
      if (!block) return 2;
      uint8_t* base = block + shift;
      for (uint32_t i = 0; i < NKEYS * len; i++) base[i] = key_byte(len + i / len, i % len);
      const int kind = rf::fixed_kind(base, len);
      if (kind != rf::IN_KEYS24 && kind != rf::IN_KEYS_W && kind != rf::IN_KEYS_B) {
        printf("fixed_kind(%u, shift %u) = %d\n", len, shift, kind);
        g_failed++;
      }
      for (uint32_t k = 0; k < NKEYS; k++) {
        const uint8_t* key = base + (size_t)k * len;
        uint32_t got;
        if (kind == rf::IN_KEYS24) {  // three 8-byte loads
          const uint64_t* q = reinterpret_cast<const uint64_t*>(key);
          const uint64_t a = q[0], b = q[1], c = q[2];
          const uint32_t w[6] = {(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32), (uint32_t)c, (uint32_t)(c >> 32)};
          got = rf::xxh32_24(w, 42u);
        } else if (kind == rf::IN_KEYS_W) {
          got = rf::xxh32_words(reinterpret_cast<const uint32_t*>(key), len, 42u);
        } else {
          got = rf::xxh32_unaligned_prefetch(key, len, 42u);
        }
        expect(kind == rf::IN_KEYS24 ? "dispatch IN_KEYS24" : kind == rf::IN_KEYS_W ? "dispatch IN_KEYS_W" : "dispatch IN_KEYS_B",
               len, shift, k, got, xxh32_bytes(key, len, 42u));
        checks++;
      }
      free(block);
    }
  }
  // the kinds the key-length sweep on the device relies on
  {
    alignas(16) static uint8_t buf[64];
    const int want24[6] = {rf::IN_KEYS24, rf::IN_KEYS_B, rf::IN_KEYS_B, rf::IN_KEYS_B, rf::IN_KEYS_W, rf::IN_KEYS24};
    for (int i = 0; i < 6; i++) expect("fixed_kind 24", 24, shifts[i], 0, (uint32_t)rf::fixed_kind(buf + shifts[i], 24), (uint32_t)want24[i]);
    expect("fixed_kind 16", 16, 0, 0, (uint32_t)rf::fixed_kind(buf, 16), (uint32_t)rf::IN_KEYS_W);
    expect("fixed_kind 16", 16, 2, 0, (uint32_t)rf::fixed_kind(buf + 2, 16), (uint32_t)rf::IN_KEYS_B);
    expect("fixed_kind 18", 18, 0, 0, (uint32_t)rf::fixed_kind(buf, 18), (uint32_t)rf::IN_KEYS_B);
    expect("fixed_kind 17", 17, 0, 0, (uint32_t)rf::fixed_kind(buf, 17), (uint32_t)rf::IN_KEYS_B);
  }
  // pick4u: each selector picks its own argument
  for (uint32_t q = 0; q < 4; q++) expect("pick4u", q, 0, 0, rf::pick4u(q, 10u, 11u, 12u, 13u), 10u + q);
  expect("rotl32", 0, 0, 0, rf::rotl32(0x80000001u, 1), 3u);
  expect("xround", 0, 0, 0, rf::xround(5u, 9u), rol(5u + 9u * 2246822519u, 13) * 2654435761u);
  {
    uint32_t h = 0x12345678u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    expect("xavalanche", 0, 0, 0, rf::xavalanche(0x12345678u), h);
  }
  if (g_failed) {
    printf("hash_check: %d FAILED of %u\n", g_failed, checks);
    return 1;
  }
  printf("hash_check: OK (%u comparisons)\n", checks);
  return 0;
}
