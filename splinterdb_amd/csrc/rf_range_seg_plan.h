// rf_range_seg_plan.h -- host-only planning of a range map made from segments
// (rf_amd_range_map_create_segments, rf_amd_range_map_update_segments): the validation of the
// caller's table, the image, the host flatten, and the cut of an update into launches and pieces.
// Plain C++ like rf_range_plan.h: no HIP calls, no engine types -- tests/c/range_seg_check.cpp
// checks it without a GPU. The plan functions return 0 or the RF_AMD_E* code with the message in
// *err; a refused call has written nothing.
//
// A segment is what one (node, pivot) of the trunk contributes to a lookup path: the member ids
// of the pivot's live inflight bundles, then its pivot bundle. Segment s has a fixed capacity
// cap[s] and a current list of len[s] <= cap[s] ids in its own slots. Range r has a path, a
// sequence of segment ids from the root down, and its list is the concatenation of the current
// lists of its path's segments. A segment of the root is in many paths and stored once.
//
// The route kernels read a flat table, so the image keeps one: loff[0..R] and list, with room
// for every path's capacities, rewritten from the segments after every update (the flatten:
// k_range_seg_len, k_range_scan, k_range_seg_emit; range_seg_flatten_host is its mirror). The
// flat table stays at the same addresses, so a route call never knows the difference.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "rf_range_plan.h"

namespace rf {

// The image of a segmented map: the flat map's sections (rf_range_plan.h) with `list` sized for
// the sum over ranges of their paths' capacities, and behind `bytes`, each on an 8-byte boundary:
//   poff     R + 1 uint64   path offsets, poff[0] = 0
//   sbase    S uint64       the first slot of each segment in `slots`
//   toff     T + 1 uint64   the flatten's tile offsets, T = ceil(R / RANGE_TILE), and the total
//   tcnt     T uint32       the flatten's tile sums
//   path     poff[R] uint32 segment ids
//   scap     S uint32       capacities
//   slen     S uint32       current lengths
//   slots    sum of cap uint32
struct RangeSegPlan : RangePlan {
  uint32_t num_segments = 0;
  uint64_t list_cap = 0;  // ids `list` has room for
  uint64_t o_poff = 0, o_sbase = 0, o_toff = 0, o_tcnt = 0, o_path = 0, o_scap = 0, o_slen = 0, o_slots = 0;
};

// the segment sections by address (device, or the plan's own image on the host): what the
// scatter and the flatten read and write
struct RangeSegDev {
  uint32_t num_ranges, num_segments;
  uint64_t list_cap;
  const uint64_t *poff, *sbase;
  const uint32_t *path, *scap;
  uint32_t *slen, *slots;
  uint64_t* loff;
  uint32_t* list;
  uint64_t* toff;
  uint32_t* tcnt;
};

inline RangeSegDev range_seg_dev(const RangeSegPlan& p, uint8_t* base) {
  RangeSegDev d;
  d.num_ranges = p.num_ranges;
  d.num_segments = p.num_segments;
  d.list_cap = p.list_cap;
  d.poff = reinterpret_cast<const uint64_t*>(base + p.o_poff);
  d.sbase = reinterpret_cast<const uint64_t*>(base + p.o_sbase);
  d.path = reinterpret_cast<const uint32_t*>(base + p.o_path);
  d.scap = reinterpret_cast<const uint32_t*>(base + p.o_scap);
  d.slen = reinterpret_cast<uint32_t*>(base + p.o_slen);
  d.slots = reinterpret_cast<uint32_t*>(base + p.o_slots);
  d.loff = reinterpret_cast<uint64_t*>(base + p.o_loff);
  d.list = reinterpret_cast<uint32_t*>(base + p.o_list);
  d.toff = reinterpret_cast<uint64_t*>(base + p.o_toff);
  d.tcnt = reinterpret_cast<uint32_t*>(base + p.o_tcnt);
  return d;
}

// The flatten on the host, step for step the three launches: the tile sums of the ranges'
// lengths, their exclusive scan (the total to loff[R]), then per tile the scan of the lengths
// into loff and each range's path expanded into list. Nothing at or past list[list_cap) is
// written, whatever the lengths say.
inline void range_seg_flatten_host(const RangeSegDev& d) {
  const uint64_t R = d.num_ranges, tiles = range_route_tiles(R);
  auto len_of = [&](uint64_t r) {
    uint32_t n = 0;
    for (uint64_t p = d.poff[r]; p < d.poff[r + 1]; p++) n += d.slen[d.path[p]];
    return n;
  };
  for (uint64_t t = 0; t < tiles; t++) {
    uint32_t c = 0;
    for (uint64_t r = t * RANGE_TILE; r < R && r < (t + 1) * RANGE_TILE; r++) c += len_of(r);
    d.tcnt[t] = c;
  }
  uint64_t carry = 0;
  for (uint64_t t = 0; t < tiles; t++) {
    d.toff[t] = carry;
    carry += d.tcnt[t];
  }
  d.toff[tiles] = carry;
  d.loff[R] = carry;
  for (uint64_t t = 0; t < tiles; t++) {
    uint64_t at = d.toff[t];
    for (uint64_t r = t * RANGE_TILE; r < R && r < (t + 1) * RANGE_TILE; r++) {
      d.loff[r] = at;
      for (uint64_t p = d.poff[r]; p < d.poff[r + 1]; p++) {
        const uint32_t s = d.path[p], n = d.slen[s];
        const uint32_t* src = d.slots + d.sbase[s];
        for (uint32_t i = 0; i < n; i++)
          if (at + i < d.list_cap) d.list[at + i] = src[i];
        at += n;
      }
    }
  }
}

// bound arrays as rf_amd_range_map_create takes them; range r's path is path[path_off[r] ..
// path_off[r + 1]); segment s has room for seg_cap[s] ids and starts as seg_ids[seg_off[s] ..
// seg_off[s + 1]). max_list is the largest sum of a path's capacities: the bound on any list the
// map can ever hold, and at most RANGE_MAX_LIST.
inline int plan_range_map_segments(uint32_t num_ranges, const uint8_t* bound_bytes, const uint64_t* bound_off,
                                   const uint32_t* path, const uint64_t* path_off, uint32_t num_segments,
                                   const uint32_t* seg_cap, const uint32_t* seg_ids, const uint64_t* seg_off,
                                   RangeSegPlan* plan, std::string* err) {
  auto refuse = [&](const char* m) {
    if (err) *err = m;
    return RF_AMD_EINVAL;
  };
  if (!plan) return refuse("null plan");
  const uint32_t R = num_ranges, S = num_segments;
  if (R == 0) return refuse("num_ranges == 0");
  if (!path_off) return refuse("null path offsets");
  if (const char* m = range_bounds_refusal(R, bound_bytes, bound_off)) return refuse(m);
  const uint64_t nbytes = R > 1 ? bound_off[R - 1] - bound_off[0] : 0;
  for (uint32_t r = 0; r < R; r++)
    if (path_off[r + 1] < path_off[r]) return refuse("path offsets decrease");
  const uint64_t npath = path_off[R] - path_off[0];
  if (npath && !path) return refuse("null paths");
  if (S && (!seg_cap || !seg_off)) return refuse("null segment capacities / offsets");
  uint64_t nslots = 0;
  for (uint32_t s = 0; s < S; s++) {
    if (seg_off[s + 1] < seg_off[s]) return refuse("segment offsets decrease");
    if (seg_off[s + 1] - seg_off[s] > seg_cap[s]) return refuse("an initial list longer than its capacity");
    nslots += seg_cap[s];
  }
  if (S && seg_off[S] - seg_off[0] && !seg_ids) return refuse("null segment ids");
  uint64_t list_cap = 0;
  uint32_t max_list = 0;
  for (uint32_t r = 0; r < R; r++) {
    uint64_t room = 0;
    for (uint64_t p = path_off[r]; p < path_off[r + 1]; p++) {
      if (path[p] >= S) return refuse("a path entry >= num_segments");
      room += seg_cap[path[p]];
      if (room > RANGE_MAX_LIST) return refuse("a path whose capacities sum to more than 65,535 ids");
    }
    if (room > max_list) max_list = (uint32_t)room;
    list_cap += room;
  }
  // nothing above has written anything
  const uint64_t tiles = range_route_tiles(R);
  RangeSegPlan p;
  p.num_ranges = R;
  p.max_list = max_list;
  p.num_segments = S;
  p.list_cap = list_cap;
  p.o_prefix = 0;
  p.o_boff = p.o_prefix + 8ull * (R - 1);
  p.o_loff = p.o_boff + 8ull * R;
  p.o_list = p.o_loff + 8ull * (R + 1);
  p.o_bytes = (p.o_list + 4 * list_cap + 7) & ~7ull;
  p.o_poff = (p.o_bytes + nbytes + 8 + 7) & ~7ull;
  p.o_sbase = p.o_poff + 8ull * (R + 1);
  p.o_toff = p.o_sbase + 8ull * S;
  p.o_tcnt = p.o_toff + 8 * (tiles + 1);
  p.o_path = p.o_tcnt + 4 * tiles;
  p.o_scap = p.o_path + 4 * npath;
  p.o_slen = p.o_scap + 4ull * S;
  p.o_slots = p.o_slen + 4ull * S;
  p.image.assign(p.o_slots + 4 * nslots + 8, 0);
  uint8_t* base = p.image.data();
  uint64_t* prefix = reinterpret_cast<uint64_t*>(base + p.o_prefix);
  uint64_t* boff = reinterpret_cast<uint64_t*>(base + p.o_boff);
  for (uint32_t j = 0; j < R; j++) boff[j] = R > 1 ? bound_off[j] - bound_off[0] : 0;
  for (uint32_t j = 0; j + 1 < R; j++)
    prefix[j] = range_prefix(bound_bytes + bound_off[j], bound_off[j + 1] - bound_off[j]);
  if (nbytes) memcpy(base + p.o_bytes, bound_bytes + bound_off[0], nbytes);
  uint64_t* poff = reinterpret_cast<uint64_t*>(base + p.o_poff);
  uint64_t* sbase = reinterpret_cast<uint64_t*>(base + p.o_sbase);
  uint32_t* scap = reinterpret_cast<uint32_t*>(base + p.o_scap);
  const RangeSegDev d = range_seg_dev(p, base);
  for (uint32_t r = 0; r <= R; r++) poff[r] = path_off[r] - path_off[0];
  if (npath) memcpy(base + p.o_path, path + path_off[0], 4 * npath);
  uint64_t at = 0;
  for (uint32_t s = 0; s < S; s++) {
    const uint64_t n = seg_off[s + 1] - seg_off[s];
    sbase[s] = at;
    scap[s] = seg_cap[s];
    d.slen[s] = (uint32_t)n;
    if (n) memcpy(d.slots + at, seg_ids + seg_off[s], 4 * n);
    at += seg_cap[s];
  }
  range_seg_flatten_host(d);
  *plan = std::move(p);
  return 0;
}

// ---- updates ------------------------------------------------------------------------------------
// The new ids and lengths of an update travel in the scatter kernel's arguments, as a filter
// set's member updates do (SetUpdate, rf_plan.h): no staging buffer, nothing whose lifetime the
// host would have to track. A launch carries RANGE_SEG_WORDS 32-bit words: npieces pieces of
// RANGE_SEG_PIECE_WORDS words each -- {segment, first slot written, first id word, ids, length} --
// and behind them the pieces' ids. A piece is a whole list or, where a list does not fit what is
// left of a launch, a part of it; `length` is RANGE_SEG_NO_LEN on every piece but a list's last,
// which stores the segment's new length. No segment has two pieces in one launch.
constexpr uint32_t RANGE_SEG_WORDS = 1000;
constexpr uint32_t RANGE_SEG_PIECE_WORDS = 5;
constexpr uint32_t RANGE_SEG_LAUNCH_IDS = RANGE_SEG_WORDS - RANGE_SEG_PIECE_WORDS;  // one piece's most
constexpr uint32_t RANGE_SEG_NO_LEN = 0xFFFFFFFFu;
// the flatten's expansion: the longest list a single thread copies; a longer one takes a wave
constexpr uint32_t RANGE_SEG_THREAD_IDS = 32;
struct RangeSegUpdate {
  uint32_t* slots;
  uint32_t* slen;
  const uint64_t* sbase;
  const uint32_t* scap;
  uint32_t num_segments;
  uint32_t npieces;
  uint32_t w[RANGE_SEG_WORDS];
};
static_assert(sizeof(RangeSegUpdate) == 40 + 4 * RANGE_SEG_WORDS && sizeof(RangeSegUpdate) <= 4096,
              "one launch's pieces and ids fit HIP's 4,096 bytes of kernel arguments");

// what the host keeps of a segmented map for its updates: the capacities, and the scratch of the
// deduplication (mark[s] == gen: an entry of s seen in this call)
struct RangeSegState {
  std::vector<uint32_t> cap, mark;
  uint32_t gen = 0;
  void init(const uint32_t* seg_cap, uint32_t S) {
    cap.assign(seg_cap, seg_cap + S);
    mark.assign(S, 0u);
    gen = 0;
  }
};

// a piece of the plan: ids h_ids[src .. src + n) to slots [dst, dst + n) of segment seg
struct RangeSegPiece {
  uint32_t seg, dst, n, len;
  uint64_t src;
};
// order: the positions, in the call's arrays, of the entries kept; launch l takes
// pieces[cuts[l] .. cuts[l + 1]); a call without entries has no launch
struct RangeSegUpdatePlan {
  std::vector<uint32_t> order;
  std::vector<RangeSegPiece> pieces;
  std::vector<uint32_t> cuts;
  uint32_t launches() const { return cuts.empty() ? 0u : (uint32_t)cuts.size() - 1; }
};

// the call: segment seg_id[i]'s list becomes ids[ids_off[i] .. ids_off[i + 1]). Of a repeated id
// only the last entry is kept; the kept entries go out in the call's order.
inline int plan_range_seg_update(RangeSegState* s, uint32_t count, const uint32_t* seg_id, const uint32_t* ids,
                                 const uint64_t* ids_off, RangeSegUpdatePlan* plan, std::string* err) {
  auto refuse = [&](const char* m) {
    if (err) *err = m;
    return RF_AMD_EINVAL;
  };
  if (!s || !plan) return refuse("null segment state");
  if (count && (!seg_id || !ids_off)) return refuse("null segment arrays");
  for (uint32_t i = 0; i < count; i++) {
    if (seg_id[i] >= s->cap.size()) return refuse("segment id >= num_segments");
    if (ids_off[i + 1] < ids_off[i]) return refuse("id offsets decrease");
    if (ids_off[i + 1] - ids_off[i] > s->cap[seg_id[i]]) return refuse("a list longer than its segment's capacity");
  }
  if (count && ids_off[count] - ids_off[0] && !ids) return refuse("null ids");
  // nothing above has written anything; nothing below fails
  plan->order.clear();
  plan->pieces.clear();
  plan->cuts.clear();
  if (count == 0) return 0;
  if (++s->gen == 0) {  // the counter wrapped: stale marks could match again
    s->mark.assign(s->mark.size(), 0u);
    s->gen = 1;
  }
  std::vector<uint32_t>& order = plan->order;
  std::vector<uint32_t>& cuts = plan->cuts;
  order.resize(count);
  uint32_t kept = 0;
  for (uint32_t i = count; i-- > 0;) {  // backwards: the first entry met of an id is its last
    if (s->mark[seg_id[i]] == s->gen) continue;
    s->mark[seg_id[i]] = s->gen;
    order[count - ++kept] = i;
  }
  order.erase(order.begin(), order.begin() + (count - kept));
  cuts.push_back(0);
  uint32_t used = 0;  // words of the open launch
  for (uint32_t i : order) {
    const uint32_t n = (uint32_t)(ids_off[i + 1] - ids_off[i]);
    uint32_t done = 0;
    do {
      if (used + RANGE_SEG_PIECE_WORDS + (n > done ? 1u : 0u) > RANGE_SEG_WORDS) {  // no room for a piece
        cuts.push_back((uint32_t)plan->pieces.size());
        used = 0;
      }
      const uint32_t room = RANGE_SEG_WORDS - used - RANGE_SEG_PIECE_WORDS;
      const uint32_t take = n - done < room ? n - done : room;
      RangeSegPiece pc;
      pc.seg = seg_id[i];
      pc.dst = done;
      pc.n = take;
      pc.src = ids_off[i] + done;
      done += take;
      pc.len = done == n ? n : RANGE_SEG_NO_LEN;
      plan->pieces.push_back(pc);
      used += RANGE_SEG_PIECE_WORDS + take;
      if (done < n) {  // the launch is full: the rest of the list goes into the next
        cuts.push_back((uint32_t)plan->pieces.size());
        used = 0;
      }
    } while (done < n);
  }
  if (cuts.back() != plan->pieces.size()) cuts.push_back((uint32_t)plan->pieces.size());
  return 0;
}

// the arguments of launch l: the pieces, then their ids copied from the caller's array
inline void range_seg_fill_launch(const RangeSegUpdatePlan& plan, uint32_t l, const uint32_t* ids,
                                  RangeSegUpdate* a) {
  const uint32_t first = plan.cuts[l], np = plan.cuts[l + 1] - first;
  a->npieces = np;
  uint32_t at = RANGE_SEG_PIECE_WORDS * np;
  for (uint32_t k = 0; k < np; k++) {
    const RangeSegPiece& pc = plan.pieces[first + k];
    uint32_t* w = a->w + RANGE_SEG_PIECE_WORDS * k;
    w[0] = pc.seg;
    w[1] = pc.dst;
    w[2] = at;
    w[3] = pc.n;
    w[4] = pc.len;
    if (pc.n) memcpy(a->w + at, ids + pc.src, 4ull * pc.n);
    at += pc.n;
  }
}

// the scatter kernel on the host: what one launch stores, with the kernel's guards
inline void range_seg_scatter_host(const RangeSegUpdate& a) {
  for (uint32_t k = 0; k < a.npieces; k++) {
    const uint32_t* w = a.w + RANGE_SEG_PIECE_WORDS * k;
    const uint32_t seg = w[0], dst = w[1], src = w[2], n = w[3], len = w[4];
    if (seg >= a.num_segments) continue;
    const uint32_t cap = a.scap[seg];
    uint32_t* out = a.slots + a.sbase[seg];
    for (uint32_t i = 0; i < n; i++)
      if ((uint64_t)dst + i < cap && src + i < RANGE_SEG_WORDS) out[dst + i] = a.w[src + i];
    if (len != RANGE_SEG_NO_LEN) a.slen[seg] = len < cap ? len : cap;
  }
}

}  // namespace rf
