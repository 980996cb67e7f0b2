// rf_per_key.hip -- the key-aware candidate compaction (rf_amd_found_per_key / _ragged, gfx950):
// the found words of a fan-out probe to the candidate list the trunk's lookup loop consumes
// (trunk_ondisk_bundle_merge_lookup, src/trunk.c:6057-6087) -- records member_id << 8 | value in
// the order of rf_amd_found_compact, a CSR of the records over the keys, and optionally each
// record's key. Three stream-ordered launches without communication between workgroups, like the
// compaction and the route call (rf_range.hip), whose tile and scan kernel it shares:
//   k_per_key_count<RAGGED>       popcounts every word of a tile of PER_KEY_TILE keys and sums
//                                 them per key: one 32-bit count per key and one per tile to
//                                 scratch
//   k_range_scan (rf_range.hip)   one workgroup: exclusive scan of the tile counts into 64-bit
//                                 offsets, the total to *count and to key_off[n]
//   k_per_key_emit<RAGGED, KEYS>  scans its tile's per-key counts in the workgroup and writes
//                                 key_off[i]; then walks the pairs of the rows that have records
//                                 a second time and writes each word's records below cap
// Both passes are key-tiled like k_range_emit: a wave owns a row of 64 consecutive keys and walks
// the row's pairs 64 per step, coalesced. RAGGED: key i owns the pairs [moff[i], moff[i + 1]);
// else the K pairs from i * K, and no offsets are read. Plain vector loads and stores only; both
// kernels walk their tiles in a grid-stride loop.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "rf_device.h"
#include "rf_per_key_plan.h"
#include "rf_launch.h"

using namespace rf;

namespace {

constexpr int PK_NT = 256;
constexpr int PK_PER = PER_KEY_TILE / PK_NT;  // keys per thread of a tile, k-major
constexpr int PK_NW = PK_NT / WAVE;
constexpr int PK_U = 4;                       // steps of 64 pairs whose loads are issued together
constexpr uint32_t PK_MAX_GRID = 4096;
static_assert(PER_KEY_TILE % PK_NT == 0, "whole keys per thread");

// The pair offsets of a tile's keys, loaded before anything waits for one of them: lo[q] and hi[q]
// = the first pair of key t0 + q * PK_NT + threadIdx.x and of the key behind it, both clamped to
// key n -- so a key past n has lo == hi == the last pair's end, an empty list, and lane 63's hi
// is always its row's end. The fixed form computes them.
template <bool RAGGED>
__device__ __forceinline__ void tile_pairs(const uint64_t* __restrict__ moff, uint32_t K, uint64_t n, uint64_t t0,
                                           uint64_t (&lo)[PK_PER], uint64_t (&hi)[PK_PER]) {
#pragma unroll
  for (int q = 0; q < PK_PER; q++) {
    const uint64_t i = t0 + (uint64_t)q * PK_NT + threadIdx.x;
    const uint64_t a = i < n ? i : n, b = i + 1 < n ? i + 1 : n;
    lo[q] = RAGGED ? moff[a] : a * K;
    hi[q] = RAGGED ? moff[b] : b * K;
  }
}

// Lane k of a row holds key k's pairs [lo, hi), relative to the row's first pair, and key k's
// sum. A step's popcounts are scanned over the wave and parked in LDS; key k's pairs of the step
// are consecutive lanes, so its share is the difference of two parked prefixes, and no lane looks
// for the key of its pair.
template <bool RAGGED>
__global__ __launch_bounds__(PK_NT) void k_per_key_count(const uint64_t* __restrict__ found,
                                                         const uint64_t* __restrict__ moff, uint32_t K,
                                                         uint64_t n, uint64_t ntiles,
                                                         uint32_t* __restrict__ kcnt, uint32_t* __restrict__ tcnt) {
  __shared__ uint32_t s_c[PK_NW];
  __shared__ uint32_t s_inc[PK_NW][WAVE];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wv = threadIdx.x / WAVE;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t t0 = t * PER_KEY_TILE;
    uint64_t plo[PK_PER], phi[PK_PER];
    tile_pairs<RAGGED>(moff, K, n, t0, plo, phi);
    uint32_t c = 0;
#pragma unroll
    for (int q = 0; q < PK_PER; q++) {
      // the row: keys t0 + q * PK_NT + wv * WAVE + [0, 64)
      const uint64_t pfirst = readlane64(plo[q], 0);
      const uint32_t np = (uint32_t)(readlane64(phi[q], WAVE - 1) - pfirst);
      const uint32_t lo = (uint32_t)(plo[q] - pfirst), hi = (uint32_t)(phi[q] - pfirst);
      uint32_t acc = 0;
      for (uint32_t p0 = 0; p0 < np; p0 += (uint32_t)WAVE * PK_U) {
        uint64_t w[PK_U];
#pragma unroll
        for (int u = 0; u < PK_U; u++) {
          const uint32_t p = p0 + (uint32_t)u * WAVE + lane;
          w[u] = p < np ? found[pfirst + p] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < PK_U; u++) {
          const uint32_t s0 = p0 + (uint32_t)u * WAVE;  // the step's first pair
          if (s0 >= np) break;                          // wave-uniform
          s_inc[wv][lane] = wave_incl_scan((uint32_t)__popcll(w[u]));
          wave_sync_lds();
          const uint32_t a = lo > s0 ? lo : s0, b = hi < s0 + WAVE ? hi : s0 + WAVE;
          if (a < b) acc += s_inc[wv][b - 1 - s0] - (a > s0 ? s_inc[wv][a - 1 - s0] : 0u);
          wave_sync_lds();  // the next step's prefixes overwrite this one's
        }
      }
      const uint64_t i = t0 + (uint64_t)q * PK_NT + threadIdx.x;
      if (i < n) kcnt[i] = acc;
      c += acc;
    }
    const uint32_t s = block_sum<PK_NT>(c, s_c);
    if (threadIdx.x == 0) tcnt[t] = s;
  }
}

// A pair's first record is its row's first record plus the exclusive sum of the popcounts of the
// row's earlier pairs: a wave scan per step and a carry. The pair's lane reads its member id only
// where the word is non-zero and peels the bits from the highest down, as k_found_emit does.
// KEYS (the caller wants cand_key): a pair's records all belong to the pair's key, so its key is
// the owner of its first record among the row's per-key record offsets -- the scanned counts the
// kernel holds anyway. The ragged form parks them in LDS and a lane with records finds its key
// with wave_owner_of, so that keys without records own none; the pair offsets are not read again,
// only each row's two ends, with the counts and before anything waits. The fixed form divides.
template <bool RAGGED, bool KEYS>
__global__ __launch_bounds__(PK_NT) void k_per_key_emit(const uint64_t* __restrict__ found,
                                                        const uint32_t* __restrict__ member,
                                                        const uint64_t* __restrict__ moff, uint32_t K, uint64_t n,
                                                        uint64_t ntiles, const uint32_t* __restrict__ kcnt,
                                                        const uint64_t* __restrict__ toff,
                                                        uint64_t* __restrict__ key_off, uint64_t* __restrict__ cand,
                                                        uint64_t* __restrict__ cand_key, uint64_t cap) {
  __shared__ uint32_t s_w[PK_PER * PK_NW + 1];
  __shared__ uint32_t s_off[PK_NW][RAGGED && KEYS ? WAVE : 1];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wv = threadIdx.x / WAVE;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t t0 = t * PER_KEY_TILE;
    uint32_t x[PK_PER], cnt[PK_PER];
    uint64_t rlo[PK_PER], rhi[PK_PER];  // the rows' first pairs and ends (wave-uniform)
#pragma unroll
    for (int q = 0; q < PK_PER; q++) {
      const uint64_t i = t0 + (uint64_t)q * PK_NT + threadIdx.x;
      x[q] = cnt[q] = i < n ? kcnt[i] : 0u;
      const uint64_t first = t0 + (uint64_t)q * PK_NT + wv * WAVE;
      const uint64_t a = first < n ? first : n, b = first + WAVE < n ? first + WAVE : n;
      rlo[q] = readlane64(RAGGED ? moff[a] : a * K, 0);
      rhi[q] = readlane64(RAGGED ? moff[b] : b * K, 0);
    }
    uint32_t tot;
    block_excl_scan_kmajor<PK_NT, PK_PER>(x, s_w, &tot);  // key order: k-major, thread-minor
    const uint64_t base = toff[t];
#pragma unroll
    for (int q = 0; q < PK_PER; q++) {
      const uint64_t i = t0 + (uint64_t)q * PK_NT + threadIdx.x;
      if (i < n) key_off[i] = base + x[q];
    }
    if (tot == 0 || base >= cap) continue;  // uniform over the workgroup
#pragma unroll
    for (int q = 0; q < PK_PER; q++) {
      // the row: keys t0 + q * PK_NT + wv * WAVE + [0, 64)
      const uint32_t rfirst = __builtin_amdgcn_readfirstlane(x[q]);
      const uint32_t rcnt = __builtin_amdgcn_readlane(x[q] + cnt[q], WAVE - 1) - rfirst;
      const uint64_t rbase = base + rfirst;        // the row's first record
      if (rcnt == 0 || rbase >= cap) continue;     // uniform over the wave: no word is read again
      const uint64_t first = t0 + (uint64_t)q * PK_NT + wv * WAVE;
      const uint64_t pfirst = rlo[q];
      const uint32_t np = (uint32_t)(rhi[q] - pfirst);
      if constexpr (RAGGED && KEYS) {
        s_off[wv][lane] = x[q] - rfirst;  // past n: the row's records, which no record's position reaches
        wave_sync_lds();
      }
      uint32_t carry = 0;  // the records of the row's pairs below p0
      for (uint32_t p0 = 0; p0 < np; p0 += (uint32_t)WAVE * PK_U) {
        uint64_t w[PK_U];
#pragma unroll
        for (int u = 0; u < PK_U; u++) {
          const uint32_t p = p0 + (uint32_t)u * WAVE + lane;
          w[u] = p < np ? found[pfirst + p] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < PK_U; u++) {
          const uint32_t p = p0 + (uint32_t)u * WAVE + lane;
          const uint32_t c = (uint32_t)__popcll(w[u]);
          const uint32_t inc = wave_incl_scan(c);
          const uint32_t rpos = carry + (inc - c);  // the pair's first record within the row
          uint64_t pos = rbase + rpos;
          carry += __builtin_amdgcn_readlane(inc, WAVE - 1);
          uint64_t v = w[u];  // non-zero only below np
          if (v && pos < cap) {
            uint32_t k = 0;  // the pair's key within the row
            if constexpr (RAGGED) {
              if constexpr (KEYS) k = wave_owner_of(s_off[wv], rpos);
            } else if (KEYS || !member) {
              k = p / K;
            }
            const uint64_t id = RAGGED || member ? (uint64_t)member[pfirst + p] : (uint64_t)(p - k * K);
            const uint64_t rec = id << 8, key = first + k;
            do {  // from the highest value down
              const uint32_t b = 63u - (uint32_t)__builtin_clzll(v);
              cand[pos] = rec | b;
              if constexpr (KEYS) cand_key[pos] = key;
              pos++;
              v &= ~(1ull << b);
            } while (v && pos < cap);
          }
        }
      }
      if constexpr (RAGGED && KEYS) wave_sync_lds();  // the next row's offsets overwrite this one's
    }
  }
}

// diagnostics (rf_amd_diag_fanout_max_blocks): a cap on the grids below, so that a call over a
// few tiles runs every grid-stride loop more than once per workgroup; 0 = none
std::atomic<uint32_t> g_per_key_max_blocks{0};

}  // namespace

extern "C" void rf_per_key_set_max_blocks(uint32_t blocks) {
  g_per_key_max_blocks.store(blocks, std::memory_order_relaxed);
}

extern "C" int rf_launch_found_per_key(void* stream, const uint64_t* found, const uint32_t* member,
                                       const uint64_t* moff, uint32_t K, uint64_t n, uint64_t* key_off,
                                       uint64_t* cand, uint64_t* cand_key, uint64_t cap, uint64_t* count,
                                       void* scratch) {
  const uint64_t ntiles = per_key_tiles(n);
  const PerKeyScratch lay = per_key_scratch(n);
  uint8_t* const sb = static_cast<uint8_t*>(scratch);
  uint64_t* toff = reinterpret_cast<uint64_t*>(sb + lay.o_tile_off);
  uint32_t* tcnt = reinterpret_cast<uint32_t*>(sb + lay.o_tile_cnt);
  uint32_t* kcnt = reinterpret_cast<uint32_t*>(sb + lay.o_key_cnt);
  hipStream_t st = (hipStream_t)stream;
  uint64_t nblk = ntiles < PK_MAX_GRID ? ntiles : PK_MAX_GRID;
  const uint32_t lim = g_per_key_max_blocks.load(std::memory_order_relaxed);
  if (lim && nblk > lim) nblk = lim;
  const dim3 g((uint32_t)nblk), b(PK_NT);
  if (ntiles) {
    if (moff) hipLaunchKernelGGL(k_per_key_count<true>, g, b, 0, st, found, moff, K, n, ntiles, kcnt, tcnt);
    else hipLaunchKernelGGL(k_per_key_count<false>, g, b, 0, st, found, moff, K, n, ntiles, kcnt, tcnt);
  }
  rf_launch_range_scan(st, tcnt, ntiles, toff, count, key_off + n);
  if (ntiles) {
#define L(R, Q) hipLaunchKernelGGL((k_per_key_emit<R, Q>), g, b, 0, st, found, member, moff, K, n, ntiles, kcnt, toff, key_off, cand, cand_key, cap)
    if (moff) { if (cand_key) L(true, true); else L(true, false); }
    else { if (cand_key) L(false, true); else L(false, false); }
#undef L
  }
  return launch_status();
}
