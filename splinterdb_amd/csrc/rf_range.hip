// rf_range.hip -- range maps: routing multi-get keys to their member lists on the device
// (rf_amd_range_map_route_keys / _route_var_keys, gfx950).
//
// A range map (rf_range_plan.h) is R ranges cut by R - 1 boundary keys in slice_lex_cmp order,
// each range with a list of member ids. A route call turns n device keys into the CSR that the
// ragged fan-out probe reads, in three stream-ordered launches without communication between
// workgroups, like the candidate compaction:
//   k_range_find<VAR, LDS>  one key per lane: its range r = the number of boundaries <= the key,
//                           to range[i]; the sum of the list lengths of a tile of RANGE_TILE keys
//                           to cnt[tile]
//   k_range_scan            one workgroup: exclusive scan of the tile sums into 64-bit offsets,
//                           the total to *total and to member_off[n]
//   k_range_emit            re-reads its tile's ranges, scans the list lengths in the workgroup,
//                           writes member_off[i], and expands the lists into member[] below
//                           pair_cap with coalesced stores
// Plain vector loads and stores only; every kernel walks its tiles in a grid-stride loop.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "rf_device.h"
#include "rf_range_plan.h"
#include "rf_launch.h"

using namespace rf;

namespace {

constexpr int RG_NT = 256;
constexpr int RG_PER = RANGE_TILE / RG_NT;  // keys per thread of a tile, k-major
constexpr int RG_NW = RG_NT / WAVE;
constexpr uint32_t RG_MAX_GRID = 4096;
constexpr uint32_t RG_LDS_PREFIXES = RANGE_LDS_RANGES - 1;
static_assert(RANGE_TILE % RG_NT == 0, "whole keys per thread");
static_assert((uint64_t)RANGE_TILE * RANGE_MAX_LIST < (1ull << 32), "a tile's pairs fit 32 bits");

// the first 8 bytes of a key in device memory, big-endian, zero-padded (range_prefix)
__device__ __forceinline__ uint64_t key_prefix(const uint8_t* k, uint64_t len) {
  if (len >= 8) {
    uint64_t w;
    __builtin_memcpy(&w, k, 8);  // one load at any alignment, inside the key
    return __builtin_bswap64(w);
  }
  uint64_t p = 0;
  for (uint32_t i = 0; i < 8; i++) p = (p << 8) | (i < len ? (uint64_t)k[i] : 0ull);
  return p;
}

// slice_lex_cmp(boundary, key) <= 0 for a boundary whose prefix equals the key's: unsigned bytes
// over the common length, then the shorter first. Where both hold 8 bytes or more the equal
// prefixes are 8 equal bytes, and the compare starts behind them.
__device__ __forceinline__ bool bound_le_key(const uint8_t* b, uint64_t bl, const uint8_t* k, uint64_t kl) {
  const uint64_t m = bl < kl ? bl : kl;
  uint64_t i = m >= 8 ? 8 : 0;
  for (; i + 8 <= m; i += 8) {
    uint64_t x, y;
    __builtin_memcpy(&x, b + i, 8);
    __builtin_memcpy(&y, k + i, 8);
    if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y);
  }
  for (; i < m; i++) {
    const uint32_t x = b[i], y = k[i];
    if (x != y) return x < y;
  }
  return bl <= kl;
}

// the number of boundaries <= the key: the upper bound of the key's prefix among the nb
// prefixes `pre` (LDS or global); only if a boundary shares the prefix, the lower bound too and
// a search of that run by full compares
template <typename P>
__device__ __forceinline__ uint32_t find_range(P pre, uint32_t nb, const uint64_t* __restrict__ boff,
                                               const uint8_t* __restrict__ bytes, const uint8_t* k, uint64_t len) {
  const uint64_t kp = key_prefix(k, len);
  uint32_t lo = 0, hi = nb;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pre[mid] <= kp) lo = mid + 1;
    else hi = mid;
  }
  if (hi == 0 || pre[hi - 1] != kp) return hi;
  uint32_t a = 0, b = hi - 1;  // pre[hi - 1] == kp: the run starts at or before hi - 1
  while (a < b) {
    const uint32_t mid = a + (b - a) / 2;
    if (pre[mid] < kp) a = mid + 1;
    else b = mid;
  }
  b = hi;
  while (a < b) {
    const uint32_t mid = a + (b - a) / 2;
    const uint64_t o = boff[mid];
    if (bound_le_key(bytes + o, boff[mid + 1] - o, k, len)) a = mid + 1;
    else b = mid;
  }
  return a;
}

// keys form: key i = keys[i * key_len, + key_len); var form: keys[offs[i], offs[i + 1])
template <bool VAR, bool LDS>
__global__ __launch_bounds__(RG_NT) void k_range_find(const uint8_t* __restrict__ keys,
                                                      const uint64_t* __restrict__ offs, uint32_t key_len,
                                                      uint64_t n, uint64_t ntiles,
                                                      const uint64_t* __restrict__ prefix, uint32_t nb,
                                                      const uint64_t* __restrict__ boff,
                                                      const uint8_t* __restrict__ bytes,
                                                      const uint64_t* __restrict__ loff,
                                                      uint32_t* __restrict__ range, uint32_t* __restrict__ cnt) {
  __shared__ uint64_t s_pre[LDS ? RG_LDS_PREFIXES : 1];
  __shared__ uint32_t s_c[RG_NW];
  if constexpr (LDS) {
    for (uint32_t j = threadIdx.x; j < nb; j += RG_NT) s_pre[j] = prefix[j];
    __syncthreads();
  }
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t t0 = t * RANGE_TILE;
    uint32_t c = 0;
#pragma unroll
    for (int q = 0; q < RG_PER; q++) {
      const uint64_t i = t0 + (uint64_t)q * RG_NT + threadIdx.x;
      if (i < n) {
        uint64_t o0, len;
        if constexpr (VAR) {
          o0 = offs[i];
          len = offs[i + 1] - o0;
        } else {
          o0 = i * key_len;
          len = key_len;
        }
        uint32_t r;
        if constexpr (LDS) r = find_range((const uint64_t*)s_pre, nb, boff, bytes, keys + o0, len);
        else r = find_range(prefix, nb, boff, bytes, keys + o0, len);
        range[i] = r;
        c += (uint32_t)(loff[r + 1] - loff[r]);
      }
    }
    const uint32_t s = block_sum<RG_NT>(c, s_c);
    if (threadIdx.x == 0) cnt[t] = s;
  }
}

// exclusive scan of the tile sums (chunks of 1,024: a chunk's total fits 2^36) into 64-bit
// offsets; *total = member_off[n] = the number of pairs (ntiles == 0: 0, and n is 0)
__global__ __launch_bounds__(1024) void k_range_scan(const uint32_t* __restrict__ cnt, uint64_t ntiles,
                                                     uint64_t* __restrict__ off, uint64_t* __restrict__ total,
                                                     uint64_t* __restrict__ member_off_n) {
  __shared__ uint64_t s_w[1024 / WAVE];
  __shared__ uint64_t s_tot;
  const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  uint64_t carry = 0;
  for (uint64_t base = 0; base < ntiles; base += 1024) {
    const uint64_t i = base + threadIdx.x;
    const uint64_t x = i < ntiles ? cnt[i] : 0u;
    uint64_t inc = x;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const uint64_t y = __shfl_up(inc, d, WAVE);
      if ((int)lane >= d) inc += y;
    }
    if (lane == WAVE - 1) s_w[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t s = 0;
      for (int j = 0; j < 1024 / WAVE; j++) {
        const uint64_t v = s_w[j];
        s_w[j] = s;
        s += v;
      }
      s_tot = s;
    }
    __syncthreads();
    if (i < ntiles) off[i] = carry + s_w[w] + inc - x;
    carry += s_tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *total = carry;
    *member_off_n = carry;
  }
}

// The expansion is the ragged probe's walk turned round: for each of its RG_PER rows of 64
// consecutive keys a wave parks the keys' pair offsets (relative to the row's first pair) and
// list starts in LDS and walks the row's pairs 64 per step -- lane p finds its key as the last k
// with off[k] <= p, so that empty lists own no pair, reads the id from the key's list and stores
// member[first + p], coalesced. The entries of the keys past n hold the row's pair count, so the
// search never names them.
__global__ __launch_bounds__(RG_NT) void k_range_emit(const uint32_t* __restrict__ range, uint64_t n,
                                                      uint64_t ntiles, const uint64_t* __restrict__ toff,
                                                      const uint64_t* __restrict__ loff,
                                                      const uint32_t* __restrict__ list,
                                                      uint64_t* __restrict__ member_off,
                                                      uint32_t* __restrict__ member, uint64_t pair_cap) {
  __shared__ uint32_t s_w[RG_PER * RG_NW + 1];
  __shared__ uint32_t s_off[RG_NW][WAVE + 1];
  __shared__ uint64_t s_src[RG_NW][WAVE];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wv = threadIdx.x / WAVE;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t t0 = t * RANGE_TILE;
    uint32_t x[RG_PER], len[RG_PER];
    uint64_t src[RG_PER];
#pragma unroll
    for (int q = 0; q < RG_PER; q++) {
      const uint64_t i = t0 + (uint64_t)q * RG_NT + threadIdx.x;
      src[q] = 0;
      len[q] = 0;
      if (i < n) {
        const uint32_t r = range[i];
        src[q] = loff[r];
        len[q] = (uint32_t)(loff[r + 1] - src[q]);
      }
      x[q] = len[q];
    }
    uint32_t tot;
    block_excl_scan_kmajor<RG_NT, RG_PER>(x, s_w, &tot);  // key order: k-major, thread-minor
    const uint64_t base = toff[t];
#pragma unroll
    for (int q = 0; q < RG_PER; q++) {
      const uint64_t i = t0 + (uint64_t)q * RG_NT + threadIdx.x;
      if (i < n) member_off[i] = base + x[q];
    }
    if (tot == 0 || base >= pair_cap) continue;  // uniform over the workgroup
#pragma unroll
    for (int q = 0; q < RG_PER; q++) {
      // the row: keys t0 + q * RG_NT + wv * WAVE + [0, 64)
      const uint32_t first = __builtin_amdgcn_readfirstlane(x[q]);
      const uint32_t np = __builtin_amdgcn_readlane(x[q] + len[q], WAVE - 1) - first;
      const bool live = t0 + (uint64_t)q * RG_NT + threadIdx.x < n;
      s_off[wv][lane] = live ? x[q] - first : np;
      s_src[wv][lane] = src[q];
      wave_sync_lds();
      const uint64_t pfirst = base + first;
      for (uint32_t p0 = 0; p0 < np; p0 += WAVE) {
        const uint32_t p = p0 + lane;
        const uint32_t k = wave_owner_of(s_off[wv], p);
        if (p < np && pfirst + p < pair_cap) member[pfirst + p] = list[s_src[wv][k] + (p - s_off[wv][k])];
      }
      wave_sync_lds();  // the next row's offsets overwrite this one's
    }
  }
}

// ---- maps made from segments (rf_range_seg_plan.h) -------------------------------------------
// rf_amd_range_map_update_segments: the scatter stores the new ids and lengths of the named
// segments, then the flatten rewrites loff[0..R] and list from the segments in three launches
// without communication between workgroups, the shape of a route call:
//   k_range_seg_len    one range per lane: its length = the sum of its path's segment lengths;
//                      the sum of a tile of RANGE_TILE ranges to tcnt[tile]
//   k_range_scan       as above, over the tile sums; the total to loff[R]
//   k_range_seg_emit   scans its tile's lengths in the workgroup, writes loff[r], then walks each
//                      range's path and copies the segments' ids: a thread per short range, a
//                      wave per long one, 64 ids at a time
// All in stream order: a route call queued before the update reads the old table, one queued
// after it the new. The flat table keeps its addresses and layout.

// One launch of an update: wave w takes pieces w, w + RG_NW, ...; the lanes copy the piece's ids
// from the kernel's arguments into the segment's slots, and lane 0 stores the new length where
// the piece is a list's last. The host sends no segment twice in one launch, none >=
// num_segments and no list longer than its capacity; the guards keep a broken argument block
// from writing outside the segment all the same.
__global__ __launch_bounds__(RG_NT) void k_range_seg_scatter(RangeSegUpdate a) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t np = a.npieces < RANGE_SEG_WORDS / RANGE_SEG_PIECE_WORDS ? a.npieces
                                                                          : RANGE_SEG_WORDS / RANGE_SEG_PIECE_WORDS;
  for (uint32_t k = threadIdx.x / WAVE; k < np; k += RG_NW) {
    const uint32_t* w = a.w + RANGE_SEG_PIECE_WORDS * k;
    const uint32_t seg = w[0], dst = w[1], src = w[2], n = w[3], len = w[4];
    if (seg >= a.num_segments) continue;
    const uint32_t cap = a.scap[seg];
    uint32_t* out = a.slots + a.sbase[seg];
    for (uint32_t i = lane; i < n; i += WAVE)
      if ((uint64_t)dst + i < cap && src + i < RANGE_SEG_WORDS) out[dst + i] = a.w[src + i];
    if (lane == 0 && len != RANGE_SEG_NO_LEN) a.slen[seg] = len < cap ? len : cap;
  }
}

// the current length of range r's list
__device__ __forceinline__ uint32_t seg_range_len(const RangeSegDev& d, uint64_t r) {
  uint32_t n = 0;
  for (uint64_t p = d.poff[r], e = d.poff[r + 1]; p < e; p++) n += d.slen[d.path[p]];
  return n;
}

__global__ __launch_bounds__(RG_NT) void k_range_seg_len(RangeSegDev d, uint64_t ntiles) {
  __shared__ uint32_t s_c[RG_NW];
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t t0 = t * RANGE_TILE;
    uint32_t c = 0;
#pragma unroll
    for (int q = 0; q < RG_PER; q++) {
      const uint64_t r = t0 + (uint64_t)q * RG_NT + threadIdx.x;
      if (r < d.num_ranges) c += seg_range_len(d, r);
    }
    const uint32_t s = block_sum<RG_NT>(c, s_c);
    if (threadIdx.x == 0) d.tcnt[t] = s;
  }
}

// A range of at most RANGE_SEG_THREAD_IDS ids is copied by its own thread, so that a tile of
// short lists -- the trunk's shape -- is expanded by all its threads at once; a longer one by a
// wave, 64 ids at a time. s_roff: each range's first id relative to the tile's, and the tile's
// count behind them.
__global__ __launch_bounds__(RG_NT) void k_range_seg_emit(RangeSegDev d, uint64_t ntiles) {
  __shared__ uint32_t s_w[RG_PER * RG_NW + 1];
  __shared__ uint32_t s_roff[RANGE_TILE + 1];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t wv = threadIdx.x / WAVE;
  const uint64_t R = d.num_ranges;
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t t0 = t * RANGE_TILE;
    uint32_t x[RG_PER], len[RG_PER];
#pragma unroll
    for (int q = 0; q < RG_PER; q++) {
      const uint64_t r = t0 + (uint64_t)q * RG_NT + threadIdx.x;
      x[q] = len[q] = r < R ? seg_range_len(d, r) : 0u;
    }
    uint32_t tot;
    block_excl_scan_kmajor<RG_NT, RG_PER>(x, s_w, &tot);  // range order: k-major, thread-minor
    const uint64_t base = d.toff[t];
#pragma unroll
    for (int q = 0; q < RG_PER; q++) {
      const uint32_t j = (uint32_t)q * RG_NT + threadIdx.x;
      s_roff[j] = x[q];
      if (t0 + j < R) d.loff[t0 + j] = base + x[q];
    }
    if (threadIdx.x == 0) s_roff[RANGE_TILE] = tot;
#pragma unroll
    for (int q = 0; q < RG_PER; q++) {
      if (len[q] == 0 || len[q] > RANGE_SEG_THREAD_IDS) continue;  // len > 0: the range is below R
      const uint64_t r = t0 + (uint64_t)q * RG_NT + threadIdx.x;
      uint64_t at = base + x[q];
      for (uint64_t p = d.poff[r], e = d.poff[r + 1]; p < e; p++) {
        const uint32_t s = d.path[p], n = d.slen[s];
        const uint32_t* src = d.slots + d.sbase[s];
        for (uint32_t i = 0; i < n; i++)
          if (at + i < d.list_cap) d.list[at + i] = src[i];
        at += n;
      }
    }
    __syncthreads();
    const uint32_t nr = R - t0 < RANGE_TILE ? (uint32_t)(R - t0) : RANGE_TILE;
    for (uint32_t j = wv; j < nr; j += RG_NW) {
      if (s_roff[j + 1] - s_roff[j] <= RANGE_SEG_THREAD_IDS) continue;  // uniform over the wave
      uint64_t at = base + s_roff[j];
      for (uint64_t p = d.poff[t0 + j], e = d.poff[t0 + j + 1]; p < e; p++) {
        const uint32_t s = d.path[p], n = d.slen[s];
        const uint32_t* src = d.slots + d.sbase[s];
        for (uint32_t i = lane; i < n; i += WAVE)
          if (at + i < d.list_cap) d.list[at + i] = src[i];
        at += n;
      }
    }
    __syncthreads();  // the next tile's offsets overwrite this one's
  }
}

// ---- maps that follow node splits (rf_range_split_plan.h) --------------------------------------
// rf_amd_range_map_split / _set_paths: one launch per argument block. The structural sections
// are kept twice; a launch reads the live copy and stores into the other one, so no thread
// stores where another one of the launch loads, whatever the order of the workgroups. The first
// launch of an edit copies what the edit keeps, each element placed by index arithmetic on the
// host's splice points; every launch stores the new elements it carries in its arguments. The
// flatten above follows, reading the copy just written.
constexpr uint32_t RG_SPLICE_MAX_GRID = 1024;

__global__ __launch_bounds__(RG_NT) void k_range_splice(RangeSpliceArgs a) {
  range_splice_store(a, (uint64_t)blockIdx.x * RG_NT + threadIdx.x, (uint64_t)gridDim.x * RG_NT);
}

// diagnostics (rf_amd_diag_fanout_max_blocks): a cap on the grids below, so that a route call
// over a few tiles runs every grid-stride loop more than once per workgroup; 0 = none
std::atomic<uint32_t> g_range_max_blocks{0};

}  // namespace

extern "C" void rf_range_set_max_blocks(uint32_t blocks) {
  g_range_max_blocks.store(blocks, std::memory_order_relaxed);
}

// k_range_scan on its own: the key-aware compaction (rf_per_key.hip) scans its tile sums with it
extern "C" void rf_launch_range_scan(void* stream, const uint32_t* cnt, uint64_t ntiles, uint64_t* off,
                                     uint64_t* total, uint64_t* total_too) {
  hipLaunchKernelGGL(k_range_scan, dim3(1), dim3(1024), 0, (hipStream_t)stream, cnt, ntiles, off, total, total_too);
}

extern "C" int rf_launch_range_seg_scatter(void* stream, const rf::RangeSegUpdate* a) {
  if (a->npieces == 0) return 0;
  if (a->npieces > RANGE_SEG_WORDS / RANGE_SEG_PIECE_WORDS) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_range_seg_scatter, dim3(1), dim3(RG_NT), 0, (hipStream_t)stream, *a);
  return launch_status();
}

extern "C" int rf_launch_range_splice(void* stream, const rf::RangeSpliceArgs* a) {
  // a launch that copies nothing stores at most its RANGE_SPLICE_WORDS words (bytes: four a word)
  const uint64_t elems = a->bulk ? range_splice_bulk_elems(a->e) : 4ull * RANGE_SPLICE_WORDS;
  uint64_t nblk = (elems + RG_NT - 1) / RG_NT;
  if (nblk > RG_SPLICE_MAX_GRID) nblk = RG_SPLICE_MAX_GRID;
  const uint32_t cap = g_range_max_blocks.load(std::memory_order_relaxed);
  if (cap && nblk > cap) nblk = cap;
  hipLaunchKernelGGL(k_range_splice, dim3((uint32_t)nblk), dim3(RG_NT), 0, (hipStream_t)stream, *a);
  return launch_status();
}

extern "C" int rf_launch_range_seg_flatten(void* stream, const rf::RangeSegDev* d) {
  const uint64_t ntiles = range_route_tiles(d->num_ranges);
  hipStream_t st = (hipStream_t)stream;
  uint64_t nblk = ntiles < RG_MAX_GRID ? ntiles : RG_MAX_GRID;
  const uint32_t cap = g_range_max_blocks.load(std::memory_order_relaxed);
  if (cap && nblk > cap) nblk = cap;
  const dim3 g((uint32_t)nblk), b(RG_NT);
  hipLaunchKernelGGL(k_range_seg_len, g, b, 0, st, *d, ntiles);
  rf_launch_range_scan(st, d->tcnt, ntiles, d->toff, d->toff + ntiles, d->loff + d->num_ranges);
  hipLaunchKernelGGL(k_range_seg_emit, g, b, 0, st, *d, ntiles);
  return launch_status();
}

extern "C" int rf_launch_range_route(void* stream, int var, const uint8_t* keys, const uint64_t* offs,
                                     uint32_t key_len, uint64_t n, const rf::RangeDev* m, uint32_t* range,
                                     uint64_t* member_off, uint32_t* member, uint64_t pair_cap, uint64_t* total,
                                     void* scratch) {
  const uint64_t ntiles = range_route_tiles(n);
  uint64_t* toff = static_cast<uint64_t*>(scratch);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(toff + ntiles);
  hipStream_t st = (hipStream_t)stream;
  uint64_t nblk = ntiles < RG_MAX_GRID ? ntiles : RG_MAX_GRID;
  const uint32_t cap = g_range_max_blocks.load(std::memory_order_relaxed);
  if (cap && nblk > cap) nblk = cap;
  const dim3 g((uint32_t)nblk), b(RG_NT);
  const uint32_t nb = m->num_ranges - 1;
  if (ntiles) {
#define L(V, S) hipLaunchKernelGGL((k_range_find<V, S>), g, b, 0, st, keys, offs, key_len, n, ntiles, m->prefix, nb, m->boff, m->bytes, m->loff, range, cnt)
    const bool lds = nb <= RG_LDS_PREFIXES;
    if (var) { if (lds) L(true, true); else L(true, false); }
    else { if (lds) L(false, true); else L(false, false); }
#undef L
  }
  rf_launch_range_scan(st, cnt, ntiles, toff, total, member_off + n);
  if (ntiles)
    hipLaunchKernelGGL(k_range_emit, g, b, 0, st, range, n, ntiles, toff, m->loff, m->list, member_off, member,
                       pair_cap);
  return launch_status();
}
