// rf_range_split_plan.h -- host-only planning of a range map that follows node splits
// (rf_amd_range_map_create_segments_room, rf_amd_range_map_split, rf_amd_range_map_set_paths):
// the image with room to grow, the host state a roomy map keeps, the validation of an edit, its
// cut into launches of argument words, and the host mirror of the splice kernel. Plain C++ like
// rf_range_seg_plan.h: no HIP calls, no engine types -- tests/c/range_split_check.cpp checks it
// without a GPU. The plan functions return 0 or the RF_AMD_E* code with the message in *err; a
// refused call has written nothing.
//
// A leaf split (leaf_split, src/trunk.c:4789; leaf_split_select_pivots and leaf_split_init,
// :4710-4736) puts m - 1 new boundary keys strictly inside one range and gives each of the m new
// ranges a path of its own: the parent replaces the child's pivot by one pivot per new leaf
// (flush_to_one_child, :5258-5340). An index split (index_split, :4977) moves no boundary and
// replaces the paths of a contiguous run of ranges. Both are one splice: ranges [r0, r0 + k_old)
// become k_new ranges, with k_new - k_old new boundaries at boundary index r0 and k_new new paths.
//
// The splice inserts into prefix, boff, bytes, poff and path and shifts their tails. The source
// and the destination of a tail overlap and nothing orders the workgroups of a launch, so the
// image keeps these five structural sections twice: the splice reads the live copy and writes
// every element of the other one -- each from index arithmetic on the host-computed splice
// points, no scan -- and the host then gives the route launches and the flatten the other copy.
// The copy that earlier route calls read stays intact until the next structural call on the same
// stream. loff, list, the segments' sections and the flatten's scratch stay single: the flatten
// (rf_range_seg_plan.h) rewrites the flat table after every edit, as after an update.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "rf_range_seg_plan.h"

namespace rf {

// The image of a roomy map: the sections of RangeSegPlan, each sized by `room` instead of by the
// initial table, and the structural ones twice. The inherited offsets are those of copy 0, which
// create fills; o2_* are copy 1's, which the first edit writes. toff and tcnt are sized by
// room.ranges, list by room.list_ids, and max_list is room.max_list.
struct RangeRoomPlan : RangeSegPlan {
  rf_amd_range_room room{};
  uint64_t o2_prefix = 0, o2_boff = 0, o2_bytes = 0, o2_poff = 0, o2_path = 0;
  uint64_t bound_bytes = 0, path_entries = 0, list_ids = 0;  // the used part of room's fields
};

// the five structural sections of one copy, by address
struct RangeStructDev {
  uint64_t *prefix, *boff, *poff;
  uint8_t* bytes;
  uint32_t* path;
};

inline RangeStructDev range_struct_dev(const RangeRoomPlan& p, uint8_t* base, uint32_t copy) {
  RangeStructDev d;
  d.prefix = reinterpret_cast<uint64_t*>(base + (copy ? p.o2_prefix : p.o_prefix));
  d.boff = reinterpret_cast<uint64_t*>(base + (copy ? p.o2_boff : p.o_boff));
  d.poff = reinterpret_cast<uint64_t*>(base + (copy ? p.o2_poff : p.o_poff));
  d.bytes = base + (copy ? p.o2_bytes : p.o_bytes);
  d.path = reinterpret_cast<uint32_t*>(base + (copy ? p.o2_path : p.o_path));
  return d;
}

// create with room: everything plan_range_map_segments refuses, then a room smaller than the
// initial table in any field and room.max_list > RANGE_MAX_LIST, all EINVAL
inline int plan_range_map_segments_room(uint32_t num_ranges, const uint8_t* bound_bytes, const uint64_t* bound_off,
                                        const uint32_t* path, const uint64_t* path_off, uint32_t num_segments,
                                        const uint32_t* seg_cap, const uint32_t* seg_ids, const uint64_t* seg_off,
                                        const rf_amd_range_room* room, RangeRoomPlan* plan, std::string* err) {
  auto refuse = [&](const char* m) {
    if (err) *err = m;
    return RF_AMD_EINVAL;
  };
  if (!plan) return refuse("null plan");
  if (!room) return refuse("null room");
  RangeSegPlan c;  // the table as the roomless create lays it out: validated, flattened
  if (int rc = plan_range_map_segments(num_ranges, bound_bytes, bound_off, path, path_off, num_segments, seg_cap,
                                       seg_ids, seg_off, &c, err))
    return rc;
  const uint64_t R = num_ranges, S = num_segments;
  const uint64_t nbytes = R > 1 ? bound_off[R - 1] - bound_off[0] : 0, npath = path_off[R] - path_off[0];
  if (room->max_list > RANGE_MAX_LIST) return refuse("room.max_list over 65,535 ids");
  if (room->ranges < R) return refuse("room.ranges below the initial ranges");
  if (room->bound_bytes < nbytes) return refuse("room.bound_bytes below the initial boundary bytes");
  if (room->path_entries < npath) return refuse("room.path_entries below the initial path entries");
  if (room->list_ids < c.list_cap) return refuse("room.list_ids below the initial paths' capacities");
  if (room->max_list < c.max_list) return refuse("room.max_list below the initial largest path capacity");
  // nothing above has written anything
  const uint64_t Rm = room->ranges, tiles = range_route_tiles(Rm);
  uint64_t nslots = 0;
  for (uint64_t s = 0; s < S; s++) nslots += seg_cap[s];
  RangeRoomPlan p;
  p.room = *room;
  p.num_ranges = num_ranges;
  p.max_list = room->max_list;
  p.num_segments = num_segments;
  p.list_cap = room->list_ids;
  p.bound_bytes = nbytes;
  p.path_entries = npath;
  p.list_ids = c.list_cap;
  const uint64_t bytes_room = (room->bound_bytes + 8 + 7) & ~7ull;
  const uint64_t path_room = (4 * room->path_entries + 7) & ~7ull;
  p.o_prefix = 0;
  p.o_boff = p.o_prefix + 8 * (Rm - 1);
  p.o2_prefix = p.o_boff + 8 * Rm;
  p.o2_boff = p.o2_prefix + 8 * (Rm - 1);
  p.o_loff = p.o2_boff + 8 * Rm;
  p.o_poff = p.o_loff + 8 * (Rm + 1);
  p.o2_poff = p.o_poff + 8 * (Rm + 1);
  p.o_sbase = p.o2_poff + 8 * (Rm + 1);
  p.o_toff = p.o_sbase + 8 * S;
  p.o_bytes = p.o_toff + 8 * (tiles + 1);
  p.o2_bytes = p.o_bytes + bytes_room;
  p.o_path = p.o2_bytes + bytes_room;
  p.o2_path = p.o_path + path_room;
  p.o_list = p.o2_path + path_room;
  p.o_tcnt = (p.o_list + 4 * room->list_ids + 7) & ~7ull;
  p.o_scap = p.o_tcnt + 4 * tiles;
  p.o_slen = p.o_scap + 4 * S;
  p.o_slots = p.o_slen + 4 * S;
  p.image.assign(p.o_slots + 4 * nslots + 8, 0);
  uint8_t* to = p.image.data();
  const uint8_t* from = c.image.data();
  memcpy(to + p.o_prefix, from + c.o_prefix, 8 * (R - 1));
  memcpy(to + p.o_boff, from + c.o_boff, 8 * R);
  memcpy(to + p.o_loff, from + c.o_loff, 8 * (R + 1));
  memcpy(to + p.o_poff, from + c.o_poff, 8 * (R + 1));
  memcpy(to + p.o_sbase, from + c.o_sbase, 8 * S);
  memcpy(to + p.o_bytes, from + c.o_bytes, nbytes);
  memcpy(to + p.o_path, from + c.o_path, 4 * npath);
  memcpy(to + p.o_list, from + c.o_list, 4 * c.list_cap);
  memcpy(to + p.o_scap, from + c.o_scap, 4 * S);
  memcpy(to + p.o_slen, from + c.o_slen, 4 * S);
  memcpy(to + p.o_slots, from + c.o_slots, 4 * nslots);
  *plan = std::move(p);
  return 0;
}

// ---- the host state of a roomy map -----------------------------------------------------------------
// What the validation and the splice points of an edit need: the boundaries' offsets and bytes
// (the order check compares a new boundary with its neighbours), the paths' offsets and capacity
// sums, the used part of each room field, and which structural copy is live.
struct RangeSplitState {
  rf_amd_range_room room{};
  std::vector<uint64_t> boff;   // R: boff[j] = the first byte of boundary j, boff[R - 1] = the bytes in use
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> poff;   // R + 1
  std::vector<uint32_t> pcap;   // R: the sum of each path's capacities
  uint64_t list_ids = 0;        // the sum of pcap
  uint32_t live = 0;            // the structural copy the route launches and the flatten are given
  uint32_t num_ranges() const { return (uint32_t)pcap.size(); }
  uint64_t bound_bytes() const { return boff.back(); }
  uint64_t path_entries() const { return poff.back(); }
  // from the arrays of a create that plan_range_map_segments_room has accepted
  void init(const rf_amd_range_room& rm, uint32_t R, const uint8_t* bound_bytes, const uint64_t* bound_off,
            const uint32_t* path, const uint64_t* path_off, const uint32_t* seg_cap) {
    room = rm;
    boff.assign(R, 0);
    for (uint32_t j = 0; j < R && R > 1; j++) boff[j] = bound_off[j] - bound_off[0];
    bytes.clear();
    if (boff.back()) bytes.assign(bound_bytes + bound_off[0], bound_bytes + bound_off[0] + boff.back());
    poff.assign(R + 1, 0);
    pcap.assign(R, 0);
    list_ids = 0;
    for (uint32_t r = 0; r < R; r++) {
      poff[r + 1] = path_off[r + 1] - path_off[0];
      for (uint64_t p = path_off[r]; p < path_off[r + 1]; p++) pcap[r] += seg_cap[path[p]];
      list_ids += pcap[r];
    }
    live = 0;
  }
};

// ---- an edit ---------------------------------------------------------------------------------------
// Ranges [r0, r0 + k_old) become k_new ranges: a split has k_old == 1 and k_new == pieces, a
// set_paths k_old == k_new == count. The k_new - k_old new boundaries take the boundary indexes
// from r0 and their nbb bytes go in at byte_at; the new ranges' pe_new path entries replace the
// pe_old old ones at path_at. The *_new fields are the sizes after the edit.
struct RangeSplice {
  uint32_t r0, k_old, k_new, r_new;
  uint64_t byte_at, nbb, bytes_new;
  uint64_t path_at, pe_old, pe_new, path_new;
};

// One launch of an edit. Its new elements travel in w, four kinds in this order, each a run of
// consecutive items: new boundaries [b0, b0 + bn) at w[bw], four words each -- the 8-byte prefix
// (range_prefix, computed on the host), then the boundary's first byte relative to byte_at; the
// new boundary bytes [y0, y0 + yn) packed at w[yw]; the new ranges [p0, p0 + pn) at w[pw], two
// words each, a path's first entry relative to path_at; the new path entries [q0, q0 + qn) at
// w[qw]. The first launch of an edit (bulk != 0) also copies what the edit keeps.
constexpr uint32_t RANGE_SPLICE_WORDS = 944;
constexpr uint32_t RANGE_SPLICE_BOUND_WORDS = 4, RANGE_SPLICE_RANGE_WORDS = 2;
struct RangeSpliceArgs {
  RangeStructDev src, dst;
  RangeSplice e;
  uint32_t bulk, pad;
  uint32_t b0, bn, bw, y0, yn, yw, p0, pn, pw, q0, qn, qw;
  uint32_t w[RANGE_SPLICE_WORDS];
};
static_assert(sizeof(RangeSpliceArgs) == 80 + 72 + 8 + 48 + 4 * RANGE_SPLICE_WORDS && sizeof(RangeSpliceArgs) <= 4096,
              "one launch's splice points and new elements fit HIP's 4,096 bytes of kernel arguments");

struct RangeSpliceCut {
  uint32_t b0, bn, y0, yn, p0, pn, q0, qn;
};
// the edit, the cut of its new elements into launches (at least one: the bulk copy), and where
// the caller's arrays start
struct RangeSplicePlan {
  RangeSplice e{};
  uint64_t bound0 = 0, path0 = 0;  // bound_off[0] and path_off[0] of the call
  std::vector<RangeSpliceCut> cuts;
  uint32_t launches() const { return (uint32_t)cuts.size(); }
};

// the words the new elements of an edit take; an edit of at most RANGE_SPLICE_WORDS is one launch
inline uint64_t range_splice_words(uint64_t nbound, uint64_t nbytes, uint64_t nranges, uint64_t nentries) {
  return RANGE_SPLICE_BOUND_WORDS * nbound + (nbytes + 3) / 4 + RANGE_SPLICE_RANGE_WORDS * nranges + nentries;
}

inline void range_splice_cut(const RangeSplice& e, std::vector<RangeSpliceCut>* cuts) {
  cuts->clear();
  const uint64_t total[4] = {(uint64_t)e.k_new - e.k_old, e.nbb, e.k_new, e.pe_new};
  const uint32_t words[4] = {RANGE_SPLICE_BOUND_WORDS, 0, RANGE_SPLICE_RANGE_WORDS, 1};  // 0: four bytes a word
  uint64_t done[4] = {0, 0, 0, 0};
  do {
    uint32_t first[4], take[4] = {0, 0, 0, 0}, used = 0;
    for (int k = 0; k < 4; k++) {
      first[k] = (uint32_t)done[k];
      const uint64_t left = total[k] - done[k], room = RANGE_SPLICE_WORDS - used;
      const uint64_t fit = words[k] ? room / words[k] : 4 * room;
      take[k] = (uint32_t)(left < fit ? left : fit);
      used += words[k] ? words[k] * take[k] : (take[k] + 3) / 4;
      done[k] += take[k];
      if (done[k] < total[k]) break;  // the launch is full: the later kinds wait for the next
    }
    cuts->push_back({first[0], take[0], first[1], take[1], first[2], take[2], first[3], take[3]});
  } while (done[0] < total[0] || done[1] < total[1] || done[2] < total[2] || done[3] < total[3]);
}

// The shared validation and planning of split and set_paths. bound_off: k_new - k_old + 1 offsets
// (unused with no new boundary); path_off: k_new + 1 offsets. On success the state is the map's
// after the edit and `live` names the copy the launches write.
inline int plan_range_splice(RangeSplitState* s, const RangeSegState& seg, uint64_t r0, uint64_t k_old, uint64_t k_new,
                             const uint8_t* bound_bytes, const uint64_t* bound_off, const uint32_t* path,
                             const uint64_t* path_off, RangeSplicePlan* plan, std::string* err) {
  auto refuse = [&](int rc, const char* m) {
    if (err) *err = m;
    return rc;
  };
  if (!s || !plan) return refuse(RF_AMD_EINVAL, "null split state");
  const uint64_t R = s->num_ranges();
  if (k_new == 0) return refuse(RF_AMD_EINVAL, k_old ? "pieces == 0" : "count == 0");
  if (r0 >= R || k_old > R - r0) return refuse(RF_AMD_EINVAL, "a range >= num_ranges");
  const uint64_t nbn = k_new - k_old;  // k_new >= k_old: a split's 1, or equal
  if (nbn >= (1ull << 32)) return refuse(RF_AMD_EINVAL, "too many pieces");
  if (!path_off) return refuse(RF_AMD_EINVAL, "null path offsets");
  if (nbn && !bound_off) return refuse(RF_AMD_EINVAL, "null boundary offsets");
  for (uint64_t j = 0; j < nbn; j++)
    if (bound_off[j + 1] < bound_off[j]) return refuse(RF_AMD_EINVAL, "boundary offsets decrease");
  const uint64_t nbb = nbn ? bound_off[nbn] - bound_off[0] : 0;
  if (nbb && !bound_bytes) return refuse(RF_AMD_EINVAL, "null boundary bytes");
  // strictly above the lower boundary of the range, strictly ascending, strictly below the upper
  const uint8_t* prev = r0 ? s->bytes.data() + s->boff[r0 - 1] : nullptr;
  uint64_t prev_len = r0 ? s->boff[r0] - s->boff[r0 - 1] : 0;
  for (uint64_t j = 0; j < nbn; j++) {
    const uint64_t len = bound_off[j + 1] - bound_off[j];
    const uint8_t* b = len ? bound_bytes + bound_off[j] : nullptr;
    if ((r0 || j) && range_key_le(b, len, prev, prev_len))
      return refuse(RF_AMD_EINVAL, j ? "new boundaries not strictly ascending"
                                     : "a new boundary not above its range's lower boundary");
    prev = b;
    prev_len = len;
  }
  if (nbn && r0 + 1 < R &&
      range_key_le(s->bytes.data() + s->boff[r0], s->boff[r0 + 1] - s->boff[r0], prev, prev_len))
    return refuse(RF_AMD_EINVAL, "a new boundary not below its range's upper boundary");
  for (uint64_t i = 0; i < k_new; i++)
    if (path_off[i + 1] < path_off[i]) return refuse(RF_AMD_EINVAL, "path offsets decrease");
  const uint64_t pe_new = path_off[k_new] - path_off[0];
  if (pe_new && !path) return refuse(RF_AMD_EINVAL, "null paths");
  uint64_t cap_new = 0;
  for (uint64_t i = 0; i < k_new; i++) {
    uint64_t c = 0;
    for (uint64_t p = path_off[i]; p < path_off[i + 1]; p++) {
      if (path[p] >= seg.cap.size()) return refuse(RF_AMD_EINVAL, "a path entry >= num_segments");
      c += seg.cap[path[p]];
      if (c > s->room.max_list) return refuse(RF_AMD_EINVAL, "a path whose capacities sum above room.max_list");
    }
    cap_new += c;
  }
  uint64_t cap_old = 0;
  for (uint64_t r = r0; r < r0 + k_old; r++) cap_old += s->pcap[r];
  const uint64_t path_at = s->poff[r0], pe_old = s->poff[r0 + k_old] - path_at;
  RangeSplice e;
  e.r0 = (uint32_t)r0;
  e.k_old = (uint32_t)k_old;
  e.k_new = (uint32_t)k_new;
  e.byte_at = s->boff[r0];
  e.nbb = nbb;
  e.bytes_new = s->bound_bytes() + nbb;
  e.path_at = path_at;
  e.pe_old = pe_old;
  e.pe_new = pe_new;
  e.path_new = s->path_entries() - pe_old + pe_new;
  const uint64_t list_new = s->list_ids - cap_old + cap_new;
  if (R + nbn > s->room.ranges) return refuse(RF_AMD_ENOSPC, "more ranges than room.ranges");
  if (e.bytes_new > s->room.bound_bytes) return refuse(RF_AMD_ENOSPC, "more boundary bytes than room.bound_bytes");
  if (e.path_new > s->room.path_entries) return refuse(RF_AMD_ENOSPC, "more path entries than room.path_entries");
  if (list_new > s->room.list_ids) return refuse(RF_AMD_ENOSPC, "more list ids than room.list_ids");
  e.r_new = (uint32_t)(R + nbn);
  // nothing above has written anything; nothing below fails
  plan->e = e;
  plan->bound0 = nbn ? bound_off[0] : 0;
  plan->path0 = path_off[0];
  range_splice_cut(e, &plan->cuts);
  if (nbn) {
    std::vector<uint64_t> at(nbn);
    for (uint64_t j = 0; j < nbn; j++) at[j] = e.byte_at + (bound_off[j] - bound_off[0]);
    s->boff.insert(s->boff.begin() + r0, at.begin(), at.end());
    for (uint64_t j = r0 + nbn; j < s->boff.size(); j++) s->boff[j] += nbb;
    if (nbb)
      s->bytes.insert(s->bytes.begin() + e.byte_at, bound_bytes + bound_off[0], bound_bytes + bound_off[0] + nbb);
  }
  std::vector<uint64_t> starts(k_new);
  std::vector<uint32_t> caps(k_new, 0u);
  for (uint64_t i = 0; i < k_new; i++) {
    starts[i] = path_at + (path_off[i] - path_off[0]);
    for (uint64_t p = path_off[i]; p < path_off[i + 1]; p++) caps[i] += seg.cap[path[p]];
  }
  s->poff.erase(s->poff.begin() + r0, s->poff.begin() + r0 + k_old);
  s->poff.insert(s->poff.begin() + r0, starts.begin(), starts.end());
  for (uint64_t r = r0 + k_new; r < s->poff.size(); r++) s->poff[r] += pe_new - pe_old;
  s->pcap.erase(s->pcap.begin() + r0, s->pcap.begin() + r0 + k_old);
  s->pcap.insert(s->pcap.begin() + r0, caps.begin(), caps.end());
  s->list_ids = list_new;
  s->live ^= 1u;
  return 0;
}

// range `range` becomes `pieces` ranges: bound_off holds `pieces` offsets (pieces - 1 boundaries)
inline int plan_range_split(RangeSplitState* s, const RangeSegState& seg, uint32_t range, uint32_t pieces,
                            const uint8_t* bound_bytes, const uint64_t* bound_off, const uint32_t* path,
                            const uint64_t* path_off, RangeSplicePlan* plan, std::string* err) {
  if (pieces == 0) {
    if (err) *err = "pieces == 0";
    return RF_AMD_EINVAL;
  }
  return plan_range_splice(s, seg, range, 1, pieces, bound_bytes, bound_off, path, path_off, plan, err);
}

// the paths of ranges [first, first + count) are replaced; count == 0 is the caller's to skip
inline int plan_range_set_paths(RangeSplitState* s, const RangeSegState& seg, uint32_t first, uint32_t count,
                                const uint32_t* path, const uint64_t* path_off, RangeSplicePlan* plan,
                                std::string* err) {
  if (s && (first > s->num_ranges() || count > s->num_ranges() - first)) {
    if (err) *err = "first + count > num_ranges";
    return RF_AMD_EINVAL;
  }
  return plan_range_splice(s, seg, first, count, count, nullptr, nullptr, path, path_off, plan, err);
}

// the arguments of launch l but for the sections' addresses: the new elements copied from the
// caller's arrays
inline void range_splice_fill_launch(const RangeSplicePlan& plan, uint32_t l, const uint8_t* bound_bytes,
                                     const uint64_t* bound_off, const uint32_t* path, const uint64_t* path_off,
                                     RangeSpliceArgs* a) {
  const RangeSpliceCut& c = plan.cuts[l];
  a->e = plan.e;
  a->bulk = l == 0;
  a->pad = 0;
  uint32_t at = 0;
  a->b0 = c.b0, a->bn = c.bn, a->bw = at;
  for (uint32_t i = 0; i < c.bn; i++, at += RANGE_SPLICE_BOUND_WORDS) {
    const uint64_t o = bound_off[c.b0 + i], len = bound_off[c.b0 + i + 1] - o;
    const uint64_t pre = len ? range_prefix(bound_bytes + o, len) : 0, rel = o - plan.bound0;
    a->w[at] = (uint32_t)pre, a->w[at + 1] = (uint32_t)(pre >> 32);
    a->w[at + 2] = (uint32_t)rel, a->w[at + 3] = (uint32_t)(rel >> 32);
  }
  a->y0 = c.y0, a->yn = c.yn, a->yw = at;
  if (c.yn) {
    a->w[at + (c.yn - 1) / 4] = 0;  // the last word's spare bytes
    memcpy(a->w + at, bound_bytes + plan.bound0 + c.y0, c.yn);
  }
  at += (c.yn + 3) / 4;
  a->p0 = c.p0, a->pn = c.pn, a->pw = at;
  for (uint32_t i = 0; i < c.pn; i++, at += RANGE_SPLICE_RANGE_WORDS) {
    const uint64_t rel = path_off[c.p0 + i] - plan.path0;
    a->w[at] = (uint32_t)rel, a->w[at + 1] = (uint32_t)(rel >> 32);
  }
  a->q0 = c.q0, a->qn = c.qn, a->qw = at;
  if (c.qn) memcpy(a->w + at, path + plan.path0 + c.q0, 4ull * c.qn);
}

// ---- the splice, element by element: the kernel's body and its host mirror --------------------------
// Thread `tid` of `nth` stores its share of one launch. Every destination element is written by
// exactly one thread of one launch of the edit, from the source copy or from the arguments; the
// guards keep a broken argument block inside the sizes the edit names.
#if defined(__HIPCC__)
#define RF_SPLICE_FN __host__ __device__ inline
#else
#define RF_SPLICE_FN inline
#endif
RF_SPLICE_FN void range_splice_store(const RangeSpliceArgs& a, uint64_t tid, uint64_t nth) {
  const RangeSplice& e = a.e;
  const uint64_t r0 = e.r0, nbn = e.k_new - e.k_old, nb_new = e.r_new - 1;
  if (a.bulk) {
    for (uint64_t j = tid; j < nb_new; j += nth) {
      if (j < r0) a.dst.prefix[j] = a.src.prefix[j];
      else if (j >= r0 + nbn) a.dst.prefix[j] = a.src.prefix[j - nbn];
    }
    for (uint64_t j = tid; j < e.r_new; j += nth) {
      if (j < r0) a.dst.boff[j] = a.src.boff[j];
      else if (j >= r0 + nbn) a.dst.boff[j] = a.src.boff[j - nbn] + e.nbb;
    }
    for (uint64_t b = tid; b < e.bytes_new; b += nth) {
      if (b < e.byte_at) a.dst.bytes[b] = a.src.bytes[b];
      else if (b >= e.byte_at + e.nbb) a.dst.bytes[b] = a.src.bytes[b - e.nbb];
    }
    for (uint64_t r = tid; r <= e.r_new; r += nth) {
      if (r < r0) a.dst.poff[r] = a.src.poff[r];
      else if (r >= r0 + e.k_new) a.dst.poff[r] = a.src.poff[r - nbn] - e.pe_old + e.pe_new;
    }
    for (uint64_t p = tid; p < e.path_new; p += nth) {
      if (p < e.path_at) a.dst.path[p] = a.src.path[p];
      else if (p >= e.path_at + e.pe_new) a.dst.path[p] = a.src.path[p - e.pe_new + e.pe_old];
    }
  }
  for (uint64_t i = tid; i < a.bn; i += nth) {
    const uint64_t j = a.b0 + i, w = a.bw + RANGE_SPLICE_BOUND_WORDS * i;
    if (j >= nbn || w + RANGE_SPLICE_BOUND_WORDS > RANGE_SPLICE_WORDS) continue;
    a.dst.prefix[r0 + j] = a.w[w] | (uint64_t)a.w[w + 1] << 32;
    a.dst.boff[r0 + j] = e.byte_at + (a.w[w + 2] | (uint64_t)a.w[w + 3] << 32);
  }
  const uint8_t* yb = reinterpret_cast<const uint8_t*>(a.w + (a.yw < RANGE_SPLICE_WORDS ? a.yw : 0));
  for (uint64_t i = tid; i < a.yn; i += nth) {
    const uint64_t b = a.y0 + i;
    if (b >= e.nbb || 4ull * a.yw + i >= 4ull * RANGE_SPLICE_WORDS) continue;
    a.dst.bytes[e.byte_at + b] = yb[i];
  }
  for (uint64_t i = tid; i < a.pn; i += nth) {
    const uint64_t r = a.p0 + i, w = a.pw + RANGE_SPLICE_RANGE_WORDS * i;
    if (r >= e.k_new || w + RANGE_SPLICE_RANGE_WORDS > RANGE_SPLICE_WORDS) continue;
    a.dst.poff[r0 + r] = e.path_at + (a.w[w] | (uint64_t)a.w[w + 1] << 32);
  }
  for (uint64_t i = tid; i < a.qn; i += nth) {
    const uint64_t p = a.q0 + i, w = a.qw + i;
    if (p >= e.pe_new || w >= RANGE_SPLICE_WORDS) continue;
    a.dst.path[e.path_at + p] = a.w[w];
  }
}

// one launch on the host
inline void range_splice_host(const RangeSpliceArgs& a) { range_splice_store(a, 0, 1); }

// the elements of the longest section an edit's first launch copies: what sizes its grid
inline uint64_t range_splice_bulk_elems(const RangeSplice& e) {
  uint64_t n = (uint64_t)e.r_new + 1;
  if (e.bytes_new > n) n = e.bytes_new;
  if (e.path_new > n) n = e.path_new;
  return n;
}

}  // namespace rf
