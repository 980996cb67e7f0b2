// rf_by_branch.hip -- the group-by-branch call (rf_amd_found_by_branch, gfx950): the records
// member_id << 8 | value of rf_amd_found_per_key*, which come out key by key, to the order a
// consumer of a whole batch wants -- all records of one B-tree bundle_of[member]->branches[value]
// side by side and in batch order -- and the table of the branches that occur. A stable
// least-significant-digit radix sort of the 32-bit sort keys (rf_by_branch_plan.h) in digits of 8
// bits, then a run table over the sorted keys. Every launch is stream-ordered, no workgroup waits
// for another, and m = min(*count, cap) is read on the device by every kernel. Per digit pass:
//   k_bb_hist<FIRST>              per tile of BY_BRANCH_TILE records the count of every digit, from
//                                 per-wave counts in LDS, digit-major to cnt[digit * tiles(m) + tile]
//   k_bb_scan_local               exclusive scan of the 256 * tiles(m) counts within chunks of
//                                 8,192, a workgroup per chunk, and every chunk's total
//   k_bb_scan<false>              one workgroup: exclusive scan of the chunk totals
//   k_bb_scatter<FIRST, LAST, K>  ranks every record within its digit and moves it: a wave owns
//                                 1,024 consecutive records of the tile and walks them 64 per
//                                 step; a record's rank within the step is the popcount of its
//                                 digit's match mask below its lane, and the wave's digit
//                                 cursors in LDS carry the earlier steps, waves and tiles (a
//                                 count's offset within its chunk plus the chunk's). No
//                                 atomics: the rank is the input order.
// The first pass reads the records and forms (key32 << 32 | index32); later passes move that pair
// between the two scratch buffers; the last pass writes order[], the sorted keys (32-bit, to the
// free buffer) and the optional gather of cand_key. Then the run table:
//   k_bb_heads                    per tile the positions whose key differs from the one before
//   k_bb_scan<true>               their offsets; the total to *num_branches, m behind the last
//                                 written branch_off
//   k_bb_emit                     branch[u] and branch_off[u] of the run heads below branch_cap
// Tiles at or past m do nothing; all kernels but the scans walk their tiles in a grid-stride loop.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "rf_device.h"
#include "rf_by_branch_plan.h"
#include "rf_launch.h"

using namespace rf;

namespace {

constexpr int BB_NT = 256;
constexpr int BB_NW = BB_NT / WAVE;
constexpr int BB_PER = BY_BRANCH_TILE / BB_NT;           // records per thread of a tile
constexpr uint32_t BB_WSPAN = BY_BRANCH_TILE / BB_NW;    // consecutive records a wave owns
constexpr int BB_STEPS = BB_WSPAN / WAVE;                // steps of 64 records per wave
constexpr int BB_SCAN_NT = 1024, BB_SCAN_PER = 8;
static_assert(BB_SCAN_NT * BB_SCAN_PER == BY_BRANCH_SCAN_CHUNK, "a scan workgroup's step is one chunk");
constexpr uint32_t BB_MAX_GRID = 4096;
static_assert(BY_BRANCH_BINS == BB_NT, "one thread per digit where a tile's counts are summed");
static_assert(BB_STEPS * WAVE * BB_NW == BY_BRANCH_TILE, "whole steps per wave");

__device__ __forceinline__ uint64_t live_records(const uint64_t* __restrict__ count, uint64_t cap) {
  const uint64_t c = *count;
  return c < cap ? c : cap;
}

// (key32 << 32 | index32) of record j: formed from the record in the first pass, moved later
template <bool FIRST>
__device__ __forceinline__ uint64_t load_pair(const uint64_t* __restrict__ src, uint64_t j, uint32_t mmask) {
  const uint64_t c = src[j];
  if constexpr (!FIRST) return c;
  const uint32_t key = (((uint32_t)(c >> 8) & mmask) << BY_BRANCH_VALUE_BITS) | ((uint32_t)c & 63u);
  return (uint64_t)key << 32 | (uint32_t)j;
}

// the valid lanes of the wave whose digit equals this lane's: one ballot per digit bit. Every lane
// of the wave calls it; the result of a lane that is not valid is unspecified.
__device__ __forceinline__ uint64_t match_digit(uint32_t d, bool valid) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (uint32_t b = 0; b < BY_BRANCH_DIGIT_BITS; b++) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bm = __ballot(valid && bit);
    m &= bit ? bm : ~bm;
  }
  return m;
}

// a wave's records of tile t, every load issued before any is used; past m: 0
template <bool FIRST>
__device__ __forceinline__ void load_wave_span(const uint64_t* __restrict__ src, uint64_t w0, uint64_t m,
                                               uint32_t mmask, uint64_t (&r)[BB_STEPS]) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
#pragma unroll
  for (int s = 0; s < BB_STEPS; s++) {
    const uint64_t j = w0 + (uint64_t)s * WAVE + lane;
    r[s] = j < m ? load_pair<FIRST>(src, j, mmask) : 0ull;
  }
}

// wc[d] += the wave's records with digit d; wc is the wave's own row, zeroed and synchronised by
// the caller. The lowest lane of every match mask adds the mask's popcount: one writer per digit.
__device__ __forceinline__ void wave_digit_counts(const uint64_t (&r)[BB_STEPS], uint64_t w0, uint64_t m,
                                                  uint32_t shift, uint32_t* wc) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint64_t lt = (1ull << lane) - 1;
#pragma unroll
  for (int s = 0; s < BB_STEPS; s++) {
    const uint64_t j0 = w0 + (uint64_t)s * WAVE;
    if (j0 >= m) break;  // wave-uniform
    const bool valid = j0 + lane < m;
    const uint32_t d = (uint32_t)(r[s] >> (32 + shift)) & (BY_BRANCH_BINS - 1);
    const uint64_t mask = match_digit(d, valid);
    if (valid && !(mask & lt)) wc[d] += (uint32_t)__popcll(mask);
    wave_sync_lds();  // the next step's leaders read these sums
  }
}

__device__ __forceinline__ void zero_wave_counts(uint32_t (&s_wc)[BB_NW][BY_BRANCH_BINS]) {
#pragma unroll
  for (int w = 0; w < BB_NW; w++) s_wc[w][threadIdx.x] = 0;
}

template <bool FIRST>
__global__ __launch_bounds__(BB_NT) void k_bb_hist(const uint64_t* __restrict__ src,
                                                   const uint64_t* __restrict__ count, uint64_t cap,
                                                   uint32_t mmask, uint32_t shift, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t s_wc[BB_NW][BY_BRANCH_BINS];
  const uint64_t m = live_records(count, cap);
  const uint64_t mt = by_branch_tiles(m);
  const uint32_t wv = threadIdx.x / WAVE;
  for (uint64_t t = blockIdx.x; t < mt; t += gridDim.x) {
    zero_wave_counts(s_wc);
    __syncthreads();
    const uint64_t w0 = t * BY_BRANCH_TILE + (uint64_t)wv * BB_WSPAN;
    uint64_t r[BB_STEPS];
    load_wave_span<FIRST>(src, w0, m, mmask, r);
    wave_digit_counts(r, w0, m, shift, s_wc[wv]);
    __syncthreads();
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < BB_NW; w++) c += s_wc[w][threadIdx.x];
    cnt[(uint64_t)threadIdx.x * mt + t] = c;
    __syncthreads();  // the next tile zeroes the counts
  }
}

// the first level of a pass's scan: the 256 * tiles(m) digit counts scanned within chunks of
// BY_BRANCH_SCAN_CHUNK, a workgroup per chunk in a grid-stride loop, and the chunks' totals
__global__ __launch_bounds__(BB_SCAN_NT) void k_bb_scan_local(const uint32_t* __restrict__ cnt,
                                                              uint32_t* __restrict__ off,
                                                              const uint64_t* __restrict__ count, uint64_t cap,
                                                              uint32_t* __restrict__ ctot) {
  __shared__ uint32_t s_w[BB_SCAN_PER * (BB_SCAN_NT / WAVE) + 1];
  const uint64_t n = by_branch_tiles(live_records(count, cap)) * BY_BRANCH_BINS;
  const uint64_t nch = by_branch_scan_chunks(n);
  for (uint64_t c = blockIdx.x; c < nch; c += gridDim.x) {
    const uint64_t base = c * BY_BRANCH_SCAN_CHUNK;
    uint32_t x[BB_SCAN_PER];
#pragma unroll
    for (int k = 0; k < BB_SCAN_PER; k++) {
      const uint64_t i = base + (uint64_t)k * BB_SCAN_NT + threadIdx.x;
      x[k] = i < n ? cnt[i] : 0u;
    }
    uint32_t tot;
    block_excl_scan_kmajor<BB_SCAN_NT, BB_SCAN_PER>(x, s_w, &tot);
#pragma unroll
    for (int k = 0; k < BB_SCAN_PER; k++) {
      const uint64_t i = base + (uint64_t)k * BB_SCAN_NT + threadIdx.x;
      if (i < n) off[i] = x[k];
    }
    if (threadIdx.x == 0) ctot[c] = tot;
  }
}

// exclusive scan of n counts into 32-bit offsets (their total is at most m < 2^32), by one
// workgroup, 8,192 per step. RUNS: the n = tiles(m) head counts of the run table, and the call's
// two scalar results; else the second level of a pass's scan, over its chunk totals.
template <bool RUNS>
__global__ __launch_bounds__(BB_SCAN_NT) void k_bb_scan(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ off,
                                                        const uint64_t* __restrict__ count, uint64_t cap,
                                                        uint64_t* __restrict__ num_branches,
                                                        uint64_t* __restrict__ branch_off, uint64_t branch_cap) {
  __shared__ uint32_t s_w[BB_SCAN_PER * (BB_SCAN_NT / WAVE) + 1];
  const uint64_t m = live_records(count, cap);
  const uint64_t n = RUNS ? by_branch_tiles(m) : by_branch_scan_chunks(by_branch_tiles(m) * BY_BRANCH_BINS);
  uint32_t carry = 0;
  for (uint64_t base = 0; base < n; base += (uint64_t)BB_SCAN_NT * BB_SCAN_PER) {
    uint32_t x[BB_SCAN_PER];
#pragma unroll
    for (int k = 0; k < BB_SCAN_PER; k++) {
      const uint64_t i = base + (uint64_t)k * BB_SCAN_NT + threadIdx.x;
      x[k] = i < n ? cnt[i] : 0u;
    }
    uint32_t tot;
    block_excl_scan_kmajor<BB_SCAN_NT, BB_SCAN_PER>(x, s_w, &tot);
#pragma unroll
    for (int k = 0; k < BB_SCAN_PER; k++) {
      const uint64_t i = base + (uint64_t)k * BB_SCAN_NT + threadIdx.x;
      if (i < n) off[i] = carry + x[k];
    }
    carry += tot;
  }
  if constexpr (RUNS) {
    if (threadIdx.x == 0) {
      *num_branches = carry;
      if (branch_off) branch_off[carry < branch_cap ? carry : branch_cap] = m;
    }
  }
}

// KEYS (LAST only): the caller wants order_key
template <bool FIRST, bool LAST, bool KEYS>
__global__ __launch_bounds__(BB_NT) void k_bb_scatter(const uint64_t* __restrict__ src,
                                                      const uint64_t* __restrict__ count, uint64_t cap,
                                                      uint32_t mmask, uint32_t shift,
                                                      const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ coff, uint64_t* __restrict__ dst,
                                                      uint32_t* __restrict__ order, uint32_t* __restrict__ skey,
                                                      const uint64_t* __restrict__ cand_key,
                                                      uint64_t* __restrict__ order_key) {
  __shared__ uint32_t s_wc[BB_NW][BY_BRANCH_BINS];
  const uint64_t m = live_records(count, cap);
  const uint64_t mt = by_branch_tiles(m);
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wv = threadIdx.x / WAVE;
  const uint64_t lt = (1ull << lane) - 1;
  for (uint64_t t = blockIdx.x; t < mt; t += gridDim.x) {
    zero_wave_counts(s_wc);
    __syncthreads();
    const uint64_t w0 = t * BY_BRANCH_TILE + (uint64_t)wv * BB_WSPAN;
    uint64_t r[BB_STEPS];
    load_wave_span<FIRST>(src, w0, m, mmask, r);
    wave_digit_counts(r, w0, m, shift, s_wc[wv]);
    __syncthreads();
    {  // the waves' counts of digit threadIdx.x to the waves' first positions of it
      const uint64_t i = (uint64_t)threadIdx.x * mt + t;
      uint32_t base = off[i] + coff[i / BY_BRANCH_SCAN_CHUNK];
#pragma unroll
      for (int w = 0; w < BB_NW; w++) {
        const uint32_t c = s_wc[w][threadIdx.x];
        s_wc[w][threadIdx.x] = base;
        base += c;
      }
    }
    __syncthreads();
    uint32_t* const cur = s_wc[wv];  // the wave's cursors: the next position of every digit
#pragma unroll
    for (int s = 0; s < BB_STEPS; s++) {
      const uint64_t j0 = w0 + (uint64_t)s * WAVE;
      if (j0 >= m) break;  // wave-uniform
      const bool valid = j0 + lane < m;
      const uint32_t d = (uint32_t)(r[s] >> (32 + shift)) & (BY_BRANCH_BINS - 1);
      const uint64_t mask = match_digit(d, valid);
      const uint32_t rank = (uint32_t)__popcll(mask & lt);
      const uint32_t pos = valid ? cur[d] + rank : 0u;
      wave_sync_lds();  // every lane has read its cursor
      if (valid && rank == 0) cur[d] = pos + (uint32_t)__popcll(mask);
      wave_sync_lds();
      // pos < m and j < m hold by construction; the tests keep every store and the gather in bounds
      if (valid && pos < m) {
        if constexpr (LAST) {
          const uint32_t j = (uint32_t)r[s];
          order[pos] = j;
          skey[pos] = (uint32_t)(r[s] >> 32);
          if constexpr (KEYS) order_key[pos] = j < m ? cand_key[j] : 0ull;
        } else {
          dst[pos] = r[s];
        }
      }
    }
    __syncthreads();  // the next tile zeroes the counts
  }
}

// position j heads a run: the first record, or a sort key other than the one before it
__device__ __forceinline__ bool run_head(const uint32_t* __restrict__ skey, uint64_t j, uint64_t m) {
  return j < m && (j == 0 || skey[j] != skey[j - 1]);
}

__global__ __launch_bounds__(BB_NT) void k_bb_heads(const uint32_t* __restrict__ skey,
                                                    const uint64_t* __restrict__ count, uint64_t cap,
                                                    uint32_t* __restrict__ tcnt) {
  __shared__ uint32_t s_c[BB_NW];
  const uint64_t m = live_records(count, cap);
  const uint64_t mt = by_branch_tiles(m);
  for (uint64_t t = blockIdx.x; t < mt; t += gridDim.x) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < BB_PER; k++)
      c += run_head(skey, t * BY_BRANCH_TILE + (uint64_t)k * BB_NT + threadIdx.x, m);
    const uint32_t s = block_sum<BB_NT>(c, s_c);
    if (threadIdx.x == 0) tcnt[t] = s;
  }
}

__global__ __launch_bounds__(BB_NT) void k_bb_emit(const uint32_t* __restrict__ skey,
                                                   const uint64_t* __restrict__ cand,
                                                   const uint32_t* __restrict__ order,
                                                   const uint64_t* __restrict__ count, uint64_t cap,
                                                   const uint32_t* __restrict__ toff, uint64_t* __restrict__ branch,
                                                   uint64_t* __restrict__ branch_off, uint64_t branch_cap) {
  __shared__ uint32_t s_w[BB_PER * BB_NW + 1];
  const uint64_t m = live_records(count, cap);
  const uint64_t mt = by_branch_tiles(m);
  for (uint64_t t = blockIdx.x; t < mt; t += gridDim.x) {
    const uint64_t base = toff[t];
    if (base >= branch_cap) continue;  // uniform over the workgroup: the table is full
    uint32_t x[BB_PER], heads = 0;
#pragma unroll
    for (int k = 0; k < BB_PER; k++) {
      x[k] = run_head(skey, t * BY_BRANCH_TILE + (uint64_t)k * BB_NT + threadIdx.x, m);
      heads |= x[k] << k;
    }
    uint32_t tot;
    block_excl_scan_kmajor<BB_NT, BB_PER>(x, s_w, &tot);  // position order: k-major, thread-minor
#pragma unroll
    for (int k = 0; k < BB_PER; k++) {
      const uint64_t j = t * BY_BRANCH_TILE + (uint64_t)k * BB_NT + threadIdx.x;
      const uint64_t u = base + x[k];
      if (((heads >> k) & 1u) && u < branch_cap) {
        const uint32_t o = order[j];
        branch[u] = o < m ? cand[o] : 0ull;  // o < m by construction: the gather stays in bounds
        branch_off[u] = j;
      }
    }
  }
}

// diagnostics (rf_amd_diag_fanout_max_blocks): a cap on the grids below, so that a call over a
// few tiles runs every grid-stride loop more than once per workgroup; 0 = none
std::atomic<uint32_t> g_by_branch_max_blocks{0};

}  // namespace

extern "C" void rf_by_branch_set_max_blocks(uint32_t blocks) {
  g_by_branch_max_blocks.store(blocks, std::memory_order_relaxed);
}

extern "C" int rf_launch_found_by_branch(void* stream, const uint64_t* cand, const uint64_t* cand_key,
                                         const uint64_t* count, uint64_t cap, uint32_t num_members, uint32_t* order,
                                         uint64_t* order_key, uint64_t* branch, uint64_t* branch_off,
                                         uint64_t branch_cap, uint64_t* num_branches, void* scratch) {
  const ByBranchScratch lay = by_branch_scratch(cap);
  uint8_t* const sb = static_cast<uint8_t*>(scratch);
  uint64_t* const buf[2] = {reinterpret_cast<uint64_t*>(sb + lay.o_buf_a),
                            reinterpret_cast<uint64_t*>(sb + lay.o_buf_b)};
  uint32_t* const cnt = reinterpret_cast<uint32_t*>(sb + lay.o_cnt);
  uint32_t* const off = reinterpret_cast<uint32_t*>(sb + lay.o_off);
  uint32_t* const ctot = reinterpret_cast<uint32_t*>(sb + lay.o_chunk_tot);
  uint32_t* const coff = reinterpret_cast<uint32_t*>(sb + lay.o_chunk_off);
  const uint32_t passes = by_branch_passes(num_members);
  const uint32_t mb = by_branch_member_bits(num_members);
  const uint32_t mmask = (uint32_t)((1ull << mb) - 1);
  hipStream_t st = (hipStream_t)stream;
  uint64_t nblk = by_branch_tiles(cap);
  if (nblk > BB_MAX_GRID) nblk = BB_MAX_GRID;
  const uint32_t lim = g_by_branch_max_blocks.load(std::memory_order_relaxed);
  if (lim && nblk > lim) nblk = lim;
  if (nblk == 0) nblk = 1;  // cap == 0: the same launches, and every kernel finds m == 0
  uint64_t nscan = by_branch_scan_chunks(by_branch_tiles(cap) * BY_BRANCH_BINS);  // chunks of the first level
  if (nscan > nblk) nscan = nblk;
  if (nscan == 0) nscan = 1;
  const dim3 g((uint32_t)nblk), b(BB_NT), g1(1), b1(BB_SCAN_NT), gs((uint32_t)nscan);
  uint32_t* skey = nullptr;
  for (uint32_t p = 0; p < passes; p++) {
    const bool first = p == 0, last = p + 1 == passes;
    const uint64_t* src = first ? cand : buf[(p - 1) & 1];
    uint64_t* dst = buf[p & 1];
    const uint32_t shift = p * BY_BRANCH_DIGIT_BITS;
    if (first) hipLaunchKernelGGL(k_bb_hist<true>, g, b, 0, st, src, count, cap, mmask, shift, cnt);
    else hipLaunchKernelGGL(k_bb_hist<false>, g, b, 0, st, src, count, cap, mmask, shift, cnt);
    hipLaunchKernelGGL(k_bb_scan_local, gs, b1, 0, st, cnt, off, count, cap, ctot);
    hipLaunchKernelGGL(k_bb_scan<false>, g1, b1, 0, st, ctot, coff, count, cap, num_branches, branch_off, branch_cap);
    if (last) skey = reinterpret_cast<uint32_t*>(dst);
#define L(F, T, Q) hipLaunchKernelGGL((k_bb_scatter<F, T, Q>), g, b, 0, st, src, count, cap, mmask, shift, off, coff, dst, order, skey, cand_key, order_key)
    if (last) {
      if (first) { if (order_key) L(true, true, true); else L(true, true, false); }
      else { if (order_key) L(false, true, true); else L(false, true, false); }
    } else {
      if (first) L(true, false, false); else L(false, false, false);
    }
#undef L
  }
  hipLaunchKernelGGL(k_bb_heads, g, b, 0, st, skey, count, cap, cnt);
  hipLaunchKernelGGL(k_bb_scan<true>, g1, b1, 0, st, cnt, off, count, cap, num_branches, branch_off, branch_cap);
  hipLaunchKernelGGL(k_bb_emit, g, b, 0, st, skey, cand, order, count, cap, off, branch, branch_off, branch_cap);
  return launch_status();
}
