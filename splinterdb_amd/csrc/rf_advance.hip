// rf_advance.hip -- the stepwise hand-out of per-key candidates (rf_amd_found_advance, gfx950):
// for every key whose lookup is still open, its next `width` records of the list that
// rf_amd_found_per_key* wrote, in batch order and in the form rf_amd_found_by_branch takes. It is
// the early exit of the trunk's lookup loop (trunk_ondisk_bundle_merge_lookup,
// src/trunk.c:6057-6087, out at :6085) for a consumer that walks the B-trees branch by branch: it
// alternates this call, the grouping, the walk and the marking of the keys that are done. Three
// stream-ordered launches without communication between workgroups, the shape of rf_per_key.hip,
// whose tile it shares:
//   k_advance_count<FIRST>        take_i of every key of a tile of PER_KEY_TILE keys from its two
//                                 offsets, its cursor and its done byte (advance_take,
//                                 rf_advance_plan.h); one 32-bit sum per tile to scratch
//   k_range_scan (rf_range.hip)   one workgroup: exclusive scan of the tile sums into 64-bit
//                                 offsets, the total to *out_count
//   k_advance_emit<KEYS, FIRST>   computes the takes again, scans them in the workgroup, writes
//                                 the cursors, then copies: a wave owns a row of 64 keys and walks
//                                 the row's output positions 64 per step -- the stores are
//                                 coalesced, only the reads of cand gather
// Nothing is parked per key between the kernels: 13 bytes a key are read twice (two offsets, of
// which one is the neighbour's, the cursor, the done byte) and 4 are written. Plain vector loads
// and stores only; both kernels walk their tiles in a grid-stride loop.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "rf_device.h"
#include "rf_advance_plan.h"
#include "rf_launch.h"

using namespace rf;

namespace {

constexpr int AD_NT = 256;
constexpr int AD_PER = PER_KEY_TILE / AD_NT;  // keys per thread of a tile, k-major
constexpr int AD_NW = AD_NT / WAVE;
constexpr int AD_U = 4;                       // steps of 64 records whose loads are issued together
constexpr uint32_t AD_MAX_GRID = 4096;
static_assert(PER_KEY_TILE % AD_NT == 0, "whole keys per thread");

// What a tile's kernels know of key t0 + q * AD_NT + threadIdx.x: its take, and the cursor the take
// starts from. Every load -- both offsets, the cursor, the done byte -- is issued before the first
// is used. A key at or past n has both offsets clamped to key n's, no cursor and no done byte
// read, and takes nothing.
template <bool FIRST>
__device__ __forceinline__ void tile_takes(const uint64_t* __restrict__ key_off, const uint32_t* cursor,
                                           const uint8_t* __restrict__ done, uint64_t cand_cap, uint64_t n,
                                           uint32_t width, uint64_t t0, uint64_t (&lo)[AD_PER],
                                           uint32_t (&cur)[AD_PER], uint32_t (&take)[AD_PER]) {
  uint64_t hi[AD_PER];
  uint8_t dn[AD_PER];
#pragma unroll
  for (int q = 0; q < AD_PER; q++) {
    const uint64_t i = t0 + (uint64_t)q * AD_NT + threadIdx.x;
    const uint64_t a = i < n ? i : n, b = i + 1 < n ? i + 1 : n;
    lo[q] = key_off[a];
    hi[q] = key_off[b];
    cur[q] = !FIRST && i < n ? cursor[i] : 0u;
    dn[q] = done && i < n ? done[i] : (uint8_t)0;
  }
#pragma unroll
  for (int q = 0; q < AD_PER; q++) take[q] = advance_take(lo[q], hi[q], cur[q], dn[q] != 0, cand_cap, width);
}

template <bool FIRST>
__global__ __launch_bounds__(AD_NT) void k_advance_count(const uint64_t* __restrict__ key_off,
                                                         const uint32_t* __restrict__ cursor,
                                                         const uint8_t* __restrict__ done, uint64_t cand_cap,
                                                         uint64_t n, uint64_t ntiles, uint32_t width,
                                                         uint32_t* __restrict__ tcnt) {
  __shared__ uint32_t s_c[AD_NW];
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint64_t lo[AD_PER];
    uint32_t cur[AD_PER], take[AD_PER];
    tile_takes<FIRST>(key_off, cursor, done, cand_cap, n, width, t * PER_KEY_TILE, lo, cur, take);
    uint32_t c = 0;
#pragma unroll
    for (int q = 0; q < AD_PER; q++) c += take[q];
    const uint32_t s = block_sum<AD_NT>(c, s_c);
    if (threadIdx.x == 0) tcnt[t] = s;
  }
}

// Key i's records go to the positions [toff[tile] + x_i, + take_i), x_i the exclusive sum of the
// tile's takes before it; the part below out_cap is written and the cursor advances by that part
// alone, so a key that out_cap cuts gets the rest from the next call. Under FIRST every cursor
// below n is stored; else a cursor that does not move keeps its bytes without a store. A row's copy: lane k parks key k's first position within the row and
// its first source record in LDS; the lane of output position p finds its key with wave_owner_of
// (keys that take nothing own no position) and its source from the two parked words.
template <bool KEYS, bool FIRST>
__global__ __launch_bounds__(AD_NT) void k_advance_emit(const uint64_t* __restrict__ key_off,
                                                        const uint64_t* __restrict__ cand, uint64_t cand_cap,
                                                        uint64_t n, uint64_t ntiles, uint32_t width,
                                                        const uint8_t* __restrict__ done, uint32_t* cursor,
                                                        const uint64_t* __restrict__ toff,
                                                        uint64_t* __restrict__ out_cand,
                                                        uint64_t* __restrict__ out_key, uint64_t out_cap) {
  __shared__ uint32_t s_w[AD_PER * AD_NW + 1];
  __shared__ uint32_t s_off[AD_NW][WAVE];
  __shared__ uint64_t s_src[AD_NW][WAVE];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wv = threadIdx.x / WAVE;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t t0 = t * PER_KEY_TILE;
    uint64_t lo[AD_PER];
    uint32_t cur[AD_PER], take[AD_PER], x[AD_PER];
    tile_takes<FIRST>(key_off, cursor, done, cand_cap, n, width, t0, lo, cur, take);
#pragma unroll
    for (int q = 0; q < AD_PER; q++) x[q] = take[q];
    uint32_t tot;
    block_excl_scan_kmajor<AD_NT, AD_PER>(x, s_w, &tot);  // key order: k-major, thread-minor
    const uint64_t base = toff[t];
#pragma unroll
    for (int q = 0; q < AD_PER; q++) {
      const uint64_t i = t0 + (uint64_t)q * AD_NT + threadIdx.x;
      const uint64_t pos = base + x[q];
      const uint64_t room = pos < out_cap ? out_cap - pos : 0ull;
      const uint32_t wr = take[q] < room ? take[q] : (uint32_t)room;  // the records written
      if (i < n && (FIRST || wr)) cursor[i] = cur[q] + wr;
    }
    if (tot == 0 || base >= out_cap) continue;  // uniform over the workgroup
#pragma unroll
    for (int q = 0; q < AD_PER; q++) {
      // the row: keys t0 + q * AD_NT + wv * WAVE + [0, 64)
      const uint32_t rfirst = __builtin_amdgcn_readfirstlane(x[q]);
      const uint32_t rcnt = __builtin_amdgcn_readlane(x[q] + take[q], WAVE - 1) - rfirst;
      const uint64_t rbase = base + rfirst;     // the row's first output position
      if (rcnt == 0 || rbase >= out_cap) continue;  // uniform over the wave
      const uint64_t first = t0 + (uint64_t)q * AD_NT + wv * WAVE;
      // the positions of the row that exist below out_cap
      const uint32_t np = out_cap - rbase < rcnt ? (uint32_t)(out_cap - rbase) : rcnt;
      s_off[wv][lane] = x[q] - rfirst;  // a key that takes nothing, past n too: the next key's, or rcnt
      s_src[wv][lane] = lo[q] + cur[q];
      wave_sync_lds();
      for (uint32_t p0 = 0; p0 < np; p0 += (uint32_t)WAVE * AD_U) {
        uint64_t v[AD_U];
        uint32_t k[AD_U];
#pragma unroll
        for (int u = 0; u < AD_U; u++) {
          const uint32_t p = p0 + (uint32_t)u * WAVE + lane;
          v[u] = 0;
          k[u] = 0;
          if (p < np) {
            k[u] = wave_owner_of(s_off[wv], p);
            const uint64_t src = s_src[wv][k[u]] + (p - s_off[wv][k[u]]);
            if (src < cand_cap) v[u] = cand[src];  // always: a take ends at or below cand_cap
          }
        }
#pragma unroll
        for (int u = 0; u < AD_U; u++) {
          const uint32_t p = p0 + (uint32_t)u * WAVE + lane;
          const uint64_t pos = rbase + p;
          if (p < np && pos < out_cap) {
            out_cand[pos] = v[u];
            if constexpr (KEYS) out_key[pos] = first + k[u];
          }
        }
      }
      wave_sync_lds();  // the next row's words overwrite this one's
    }
  }
}

// diagnostics (rf_amd_diag_fanout_max_blocks): a cap on the grids below, so that a call over a
// few tiles runs every grid-stride loop more than once per workgroup; 0 = none
std::atomic<uint32_t> g_advance_max_blocks{0};

}  // namespace

extern "C" void rf_advance_set_max_blocks(uint32_t blocks) {
  g_advance_max_blocks.store(blocks, std::memory_order_relaxed);
}

extern "C" int rf_launch_found_advance(void* stream, const uint64_t* key_off, const uint64_t* cand, uint64_t cand_cap,
                                       uint64_t n, uint32_t width, int first, const uint8_t* done, uint32_t* cursor,
                                       uint64_t* out_cand, uint64_t* out_key, uint64_t out_cap, uint64_t* out_count,
                                       void* scratch) {
  const uint64_t ntiles = per_key_tiles(n);
  const AdvanceScratch lay = advance_scratch(n);
  uint8_t* const sb = static_cast<uint8_t*>(scratch);
  uint64_t* toff = reinterpret_cast<uint64_t*>(sb + lay.o_tile_off);
  uint32_t* tcnt = reinterpret_cast<uint32_t*>(sb + lay.o_tile_cnt);
  hipStream_t st = (hipStream_t)stream;
  uint64_t nblk = ntiles < AD_MAX_GRID ? ntiles : AD_MAX_GRID;
  const uint32_t lim = g_advance_max_blocks.load(std::memory_order_relaxed);
  if (lim && nblk > lim) nblk = lim;
  const dim3 g((uint32_t)nblk), b(AD_NT);
  if (ntiles) {
    if (first) hipLaunchKernelGGL(k_advance_count<true>, g, b, 0, st, key_off, cursor, done, cand_cap, n, ntiles, width, tcnt);
    else hipLaunchKernelGGL(k_advance_count<false>, g, b, 0, st, key_off, cursor, done, cand_cap, n, ntiles, width, tcnt);
  }
  // the scan writes its total twice; the call has one place for it
  rf_launch_range_scan(st, tcnt, ntiles, toff, out_count, out_count);
  if (ntiles) {
#define L(Q, F) hipLaunchKernelGGL((k_advance_emit<Q, F>), g, b, 0, st, key_off, cand, cand_cap, n, ntiles, width, done, cursor, toff, out_cand, out_key, out_cap)
    if (out_key) { if (first) L(true, true); else L(true, false); }
    else { if (first) L(false, true); else L(false, false); }
#undef L
  }
  return launch_status();
}
