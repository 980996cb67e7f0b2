// rf_batch_plan.h -- host-only planning of a batch: everything rf_engine.cpp decides about a
// batch before it allocates (per-filter geometry of src/routing_filter.c:357-389, coarse
// buckets, K4 bins, entry regions, page caps, probe lines, the K5 workgroup map, tile cuts of
// chained batches, which old filters are read in place), and the probe-side plan of an
// imported batch. Plain C++: no HIP calls, no environment, no allocation on the device, no
// engine types -- tests/c/plan_check.cpp checks it without a GPU. A planner returns 0 or the
// RF_AMD_E* code, with the message in *err.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/rf_amd.h"
#include "rf_plan.h"

namespace rf {

// rf_amd_max_fingerprints (src/routing_filter.h:120-127: two extents of index slots)
inline uint64_t max_fingerprints(const rf_amd_config& cfg) {
  const uint64_t addrs_per_extent = (uint64_t)cfg.page_size * cfg.pages_per_extent / 8;
  return 2ull * addrs_per_extent * (1ull << cfg.log_index_size) - 1;
}

inline uint32_t vsize_of(uint32_t value) { return value == 0 ? 0 : 32 - __builtin_clz(value); }

// log_num_buckets and num_indices of a filter of nfp > 0 fingerprints
// (src/routing_filter.c:374-379)
inline uint32_t log_buckets_of(uint64_t nfp, uint32_t lis) {
  const uint32_t lnb = 63 - __builtin_clzll(nfp);
  return lnb < lis ? lis : lnb;
}
inline uint32_t num_indices_of(uint64_t nfp, uint32_t lis) { return 1u << (log_buckets_of(nfp, lis) - lis); }

// Probe-line group size (k_plines): the largest G = 2^g <= min(IS, 64) whose 64-byte line
// (128 encoding bits for n + G, 384 remainder bits for n * rvs) holds mean + sigma sd + 2
// entries, n ~ Poisson(lam*G) with lam = fingerprints per bucket (< 2 by the choice of
// log_num_buckets). Larger G = smaller line table but more overflowed lines (those probes
// walk the image). sigma: PlanKnobs::line_sigma (lam is an upper bound; table size measured
// not to matter for the probe, overflow rate does).
// Returns g + 1, or 0 = no lines (rvs > 32: probes walk the image).
inline uint32_t line_log_group(uint32_t lis, uint32_t rvs, double lam, double sigma) {
  if (rvs > 32) return 0;
  for (int g = (int)(lis < 6 ? lis : 6); g >= 0; g--) {
    const double G = (double)(1u << g), mean = lam * G;
    const double cap = rvs ? std::min(128.0 - G, 384.0 / rvs) : 128.0 - G;
    if (mean + sigma * sqrt(mean) + 2.0 <= cap) return (uint32_t)g + 1;
  }
  return 0;
}

// Dense lines (rf_plan.h: LINE_DENSE) for a filter whose lines are now L_now per index: the
// smallest L < L_now whose groups of G = ceil(IS / L) <= 64 buckets hold mean + sigma sd + 2
// entries in the line's cap = U - G, n ~ Poisson(lam G) as above. An over-full dense line costs
// only its tail buckets the image walk, not the whole line, so sigma is a knob of its own
// (PlanKnobs::dense_sigma). L <= 256 keeps K6's and the probes' divisions by reciprocal exact.
// Returns G, or 0 = no dense geometry beats the current one.
inline uint32_t line_dense_group(uint32_t lis, uint32_t rvs, double lam, double sigma, uint32_t L_now) {
  if (rvs > 32) return 0;
  const uint32_t IS = 1u << lis;
  for (uint32_t L = 1; L < L_now && L <= 256; L++) {
    const uint32_t G = (IS + L - 1) / L;
    if (G > 64) continue;
    const double mean = lam * G, cap = (double)(line_unary_bits(G, rvs) - G);
    if (mean + sigma * sqrt(mean) + 2.0 <= cap) return G;
  }
  return 0;
}
// a filter's line table against the L2 of the XCD that probes it: only a larger table has
// anything to gain from denser lines (measured: DESIGN.md section 5)
constexpr uint64_t LINE_DENSE_MIN_TABLE = 4ull << 20;

// K6 cuts a filter's probe lines from its LDS page images when the per-page group table
// fits: each block needs IS/G + 1 entries. Returns 0: never (k_plines cuts every line),
// 1: always (even a page of the smallest blocks fits), 2: page by page -- K6 flags a page
// whose blocks do not fit and k_plines cuts those pages' lines.
inline int lines_in_assembly(uint32_t lis, uint32_t lg_line, uint32_t page_size) {
  const uint32_t IS = 1u << lis, L = lines_per_index(lis, lg_line);
  const uint32_t min_block = 2 + (IS - 1) / 8 + 4 + 3;
  const uint32_t maxb = page_size / min_block + 1;
  if (maxb > ASM_MAXB || L + 1 > ASM_GT) return 0;
  return (uint64_t)maxb * (L + 1) <= ASM_GT ? 1 : 2;
}

// the environment switches of planning (rf_engine.cpp reads them at every create / import)
struct PlanKnobs {
  bool wide64 = false;           // incremental builds keep 64-bit entries
  bool old_decode = false;       // old filters are always decoded from their images
  bool old_resplit_off = false;  // ... also when only their geometry changed
  uint32_t layout_seg = LAYOUT_SEG_MAX;  // indices per K5 workgroup: a power of two in
                                         // [LAYOUT_SEG_MIN, LAYOUT_SEG_MAX], or 0 = never split
  double line_sigma = 3.5;       // line_log_group
  int lines_dense = -1;          // dense lines: 0 never, 1 every filter with a dense geometry,
                                 // -1 those whose table outgrows LINE_DENSE_MIN_TABLE
  double dense_sigma = 2.5;      // line_dense_group
};

// the filter an incremental add starts from: filter `plan` of a batch of this process
struct OldFilter {
  bool present = false;             // the caller named an old batch for this filter
  const FilterPlan* plan = nullptr; // its plan there (nullptr: no such filter in that batch)
  uint32_t fingerprint_size = 0, log_index_size = 0;  // that batch's routing config
  bool has_entries = false;  // built by this engine, its sorted entries still held
  bool wide = false;         // itself an incremental build (entries in d_sorted)
  bool built = false;
  bool same_device = false;
};

// what to plan: num_filters filters of num_new[f] new fingerprints with value[f] (nullptr: 0),
// or -- num_runs != nullptr -- of num_runs[f] runs each (run_len / run_value, filter-major;
// num_new / value are not read), each on top of olds[f] (olds == nullptr: all fresh)
struct BatchInput {
  const rf_amd_config* cfg = nullptr;
  uint32_t num_filters = 0;
  const uint32_t* num_new = nullptr;
  const uint16_t* value = nullptr;
  const uint32_t* num_runs = nullptr;
  const uint32_t* run_len = nullptr;
  const uint16_t* run_value = nullptr;
  const OldFilter* olds = nullptr;
};

// per-filter prefix arrays (F + 1 each) of the batch's per-element maps: tiles, old tiles,
// coarse buckets, pages, indices, decoded old indices. The maps themselves (element ->
// filter, tile -> first key) are filled on the device (k_seg_fill), so creating a batch
// uploads O(filters) bytes, not O(indices + pages)
enum { PRE_TILE, PRE_OTILE, PRE_CB, PRE_PG, PRE_IDX, PRE_OIDX, NUM_PRE };

struct BatchPlan {
  uint32_t F = 0;
  std::vector<FilterPlan> plans;  // scalar fields only: the engine fills in the old_* pointers
  std::vector<uint32_t> pre;      // NUM_PRE x (F + 1)
  uint32_t* pre_of(int k) { return pre.data() + (size_t)k * (F + 1); }
  const uint32_t* pre_of(int k) const { return pre.data() + (size_t)k * (F + 1); }
  bool wide = false;        // incremental add: some filter has an old filter
  bool flag32 = false;      // wide build with 32-bit flagged entries (every fp_size + vs <= 31)
  bool chained = false;     // several runs of new inputs per filter
  uint64_t old_total = 0;   // flag32: decoded old entries reserved (sum of old num_fingerprints)
  uint32_t num_tiles = 0, num_old_tiles = 0, num_old_idx = 0;
  uint64_t E = 0, keys_total = 0;  // entry slots, new inputs
  uint32_t CB = 0, I = 0, PS = 0, PF = 0;  // coarse buckets, indices, page slots, page_first words
  uint64_t NL = 0;             // probe lines (64 B each)
  bool plines_needed = false;  // some filter's lines come from k_plines
  uint32_t line_lmax = 0;      // max probe lines per index
  bool lines_dense = false;    // some filter has dense lines (LINE_DENSE)
  // K5 over several workgroups per filter (layout_groups): indices per workgroup, workgroup ->
  // filter << 6 | segment (~0: none), the grid of k_layout_seg (0: no filter is split),
  // whether any filter keeps one workgroup
  uint32_t lay_seg = 0, lay_grid = 0;
  bool lay_whole = true;
  std::vector<uint32_t> lay_wg;
  bool k4_bitmap = false;  // K4 runs k_cb_bitmap, not k_cb_sort (k4_bitmap_batch)
  bool k4_pack = false;    // ... and packs index-block bodies for K6 to place (k4_pack_batch)
  // tile maps of a chained batch: tiles are cut at run boundaries and carry their run's value
  // and end (both relative to the filter's first input, like tile_start)
  std::vector<uint32_t> tile_filter, tile_start, tile_value, tile_end;
  std::vector<uint4> pplans;  // packed probe plan per filter (LaunchArgs::pplans)
};

inline int plan_fail(std::string* err, int rc, const std::string& msg) {
  if (err) *err = msg;
  return rc;
}

inline int check_config(const rf_amd_config* cfg, std::string* err) {
  if (!cfg) return plan_fail(err, RF_AMD_EINVAL, "null config");
  if (cfg->page_size != MAX_PAGE || cfg->pages_per_extent != 32)
    return plan_fail(err, RF_AMD_EINVAL, "engine supports 4 KiB pages in 32-page extents");
  if (cfg->fingerprint_size == 0 || cfg->fingerprint_size > 32 || cfg->log_index_size > MAX_LIS ||
      cfg->log_index_size < 3)
    return plan_fail(err, RF_AMD_EINVAL, "unsupported fingerprint_size / log_index_size");
  return 0;
}

// Probe side of a filter whose num_fp, lnb, vs, num_indices and idx_base are set: remainder
// widths, the probe-line group (dense where the knobs and the table's size say so), and the
// filter's place in the batch's line table (*line_total: lines of the filters before it,
// advanced by its own; *line_lmax raised to its lines per index; *any_dense set by a dense
// filter). The one place that derives them, for built and imported batches alike.
// fresh: a filter built in one add or imported -- what the dense format was measured on; the
// rounds of an incremental chain keep the current format unless the knob forces it.
inline void probe_geometry(FilterPlan& p, const rf_amd_config& cfg, const PlanKnobs& knobs, bool fresh,
                           uint64_t* line_total, uint32_t* line_lmax, bool* any_dense) {
  const uint32_t lis = cfg.log_index_size;
  const double lam = (double)p.num_fp / (double)(1ull << p.lnb);
  p.rem = cfg.fingerprint_size - p.lnb;
  p.rvs = p.rem + p.vs;
  p.lg_line = line_log_group(lis, p.rvs, lam, knobs.line_sigma);
  if (p.lg_line && knobs.lines_dense != 0) {
    const uint32_t L = lines_per_index(lis, p.lg_line);
    if (knobs.lines_dense > 0 || (fresh && (uint64_t)p.num_indices * L * 64 > LINE_DENSE_MIN_TABLE))
      if (const uint32_t G = line_dense_group(lis, p.rvs, lam, knobs.dense_sigma, L)) p.lg_line = LINE_DENSE | (G - 1);
  }
  p.line_base = (uint32_t)*line_total;
  if (p.lg_line) {
    const uint32_t L = lines_per_index(lis, p.lg_line);
    if (line_is_dense(p.lg_line)) *any_dense = true;
    *line_total += (uint64_t)p.num_indices * L;
    *line_lmax = std::max(*line_lmax, L);
  }
}

// vs | rem << 8 | rvs << 16 | lg_line << 24: pplans[f].x, ProbeGroup::x
inline uint32_t pplan_word(const FilterPlan& p) { return p.vs | (p.rem << 8) | (p.rvs << 16) | (p.lg_line << 24); }
inline uint4 pack_pplan(const FilterPlan& p) { return make_uint4(pplan_word(p), p.line_base, p.idx_base, 0); }

// Argument checks of a chained batch's run arrays; run_first[f] = first run of filter f,
// run_total[f] = its new inputs.
inline int check_runs(const BatchInput& in, std::vector<uint32_t>* run_first, std::vector<uint32_t>* run_total,
                      std::string* err) {
  const rf_amd_config& cfg = *in.cfg;
  run_first->assign(in.num_filters + 1, 0u);
  run_total->assign(in.num_filters, 0u);
  for (uint32_t f = 0; f < in.num_filters; f++) {
    if (in.num_runs[f] == 0) return plan_fail(err, RF_AMD_EINVAL, "a filter without runs");
    const uint32_t r0 = (*run_first)[f], r1 = r0 + in.num_runs[f];
    (*run_first)[f + 1] = r1;
    uint64_t tot = 0;
    for (uint32_t r = r0; r < r1; r++) {
      if (in.run_len[r] == 0) return plan_fail(err, RF_AMD_EINVAL, "zero-length run");
      if (r > r0 && in.run_value[r] <= in.run_value[r - 1])
        return plan_fail(err, RF_AMD_EINVAL, "run values of a filter must be strictly increasing");
      tot += in.run_len[r];
    }
    if (tot > max_fingerprints(cfg))
      return plan_fail(err, RF_AMD_EINVAL, "num_fingerprints over routing_filter_max_fingerprints (reference: UB)");
    if (cfg.fingerprint_size + vsize_of(in.run_value[r1 - 1]) > 32)
      return plan_fail(err, RF_AMD_EINVAL, "fp_size + value_size > 32");
    const OldFilter* o = in.olds && in.olds[f].present ? &in.olds[f] : nullptr;
    if (o && o->plan && vsize_of(in.run_value[r0]) < o->plan->vs)
      return plan_fail(err, RF_AMD_EINVAL, "first run's value narrower than the old filter's value_size");
    (*run_total)[f] = (uint32_t)tot;
  }
  return 0;
}

// Geometry of one filter: num_new new fingerprints of value v on top of the old filter `op`
// (nullptr: a fresh filter). Fills every scalar field of *p that does not depend on the other
// filters of the batch (the *_base / *_first fields are the caller's running sums, the probe
// lines probe_geometry's, old_direct the batch's decision).
inline int filter_geometry(const rf_amd_config& cfg, uint32_t num_new, uint32_t v, const FilterPlan* op,
                           FilterPlan* out, std::string* err) {
  FilterPlan& p = *out;
  const uint32_t lis = cfg.log_index_size, fps = cfg.fingerprint_size, IS = 1u << lis;
  p.num_new = num_new;
  p.old_region = op ? op->num_fp : 0;
  const uint64_t nfp = (uint64_t)p.num_new + p.old_region;
  if (nfp > max_fingerprints(cfg))  // checked before the u32 descriptor field can wrap
    return plan_fail(err, RF_AMD_EINVAL, "num_fingerprints over routing_filter_max_fingerprints (reference: UB)");
  p.num_fp = (uint32_t)nfp;
  if (p.num_fp == 0) return plan_fail(err, RF_AMD_EINVAL, "routing_filter_add with zero fingerprints (reference: UB)");
  const uint32_t lnb = log_buckets_of(nfp, lis);
  p.vs = vsize_of(v);
  if (lnb > fps || (1u << (lnb - lis)) > MAX_INDICES || fps + p.vs > 32 || (op && p.vs < op->vs))
    return plan_fail(err, RF_AMD_EINVAL, "filter geometry out of range (over routing_filter_max_fingerprints, "
                                         "fp_size + value_size > 32, or value narrower than old filter)");
  p.lnb = lnb;
  p.value = v;
  p.num_indices = 1u << (lnb - lis);
  int cb = (int)lnb - (int)CB_LOG_MEAN;
  if (cb < 0) cb = 0;
  if (cb > (int)(lnb - lis)) cb = (int)(lnb - lis);
  // load factor ~1 (nfp just over a power of two: C3/C4's 2^20 keys) leaves coarse buckets
  // of 2^12 buckets half full (~4K of SORT_CAP entries), and K4's cost is mostly per
  // workgroup: use coarse buckets of 2^13 buckets (~8K entries, still >= 9 sd under
  // SORT_CAP) with K4 bins of two buckets each (at most MAX_BINS bins, MAX_IPC indices)
  p.binsh = 0;
  if (cb >= 1 && lnb - cb == CB_LOG_MEAN && lis + 9 >= CB_LOG_MEAN + 1 /* ipc <= MAX_IPC */ &&
      nfp * 1000 <= (1026ull << lnb)) {
    cb -= 1;
    p.binsh = 1;
  }
  p.cbits = (uint32_t)cb;
  p.bbits = lnb - p.cbits;
  // page bound: sum of block sizes <= NI*(12 + IS/8) + E*(1+rvs)/8; next-fit <= 2x + 1
  const uint32_t rvs = fps - lnb + p.vs;
  const uint64_t bound = (uint64_t)p.num_indices * (12 + IS / 8) + (nfp * (1 + rvs) + 7) / 8;
  const uint64_t cap = 2 * ((bound + cfg.page_size - 1) / cfg.page_size) + 2;
  p.page_cap = (uint32_t)std::min<uint64_t>(cap, p.num_indices);
  if (op) {
    p.old_num_indices = op->num_indices;
    p.old_vs = op->vs;
    p.old_rvs = op->rvs;
    p.npo = p.num_indices / op->num_indices;
  }
  return 0;
}

// K5 workgroups: the G segments of a split filter go to one XCD (workgroup w runs on XCD
// w % 8), consecutive there, so segment q - 1 is workgroup w - 8: dispatched before its waiter
inline void assign_layout(BatchPlan& b) {
  uint32_t pos[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  b.lay_wg.clear();
  b.lay_whole = false;
  for (uint32_t f = 0; f < b.F; f++) {
    const uint32_t G = layout_groups(b.plans[f], b.lay_seg);
    if (G == 1) {
      b.lay_whole = true;
      continue;
    }
    const uint32_t x = (uint32_t)(std::min_element(pos, pos + 8) - pos);
    const uint32_t w0 = x + 8 * pos[x];
    const size_t need = w0 + 8 * (size_t)(G - 1) + 1;
    if (b.lay_wg.size() < need) b.lay_wg.resize(need, ~0u);
    for (uint32_t q = 0; q < G; q++) b.lay_wg[w0 + 8 * q] = f << 6 | q;
    pos[x] += G;
  }
  b.lay_grid = (uint32_t)b.lay_wg.size();
}

// K4 by bitmap (k_cb_bitmap). The entries of one coarse bucket of a fresh build differ only in
// their low bbits + rvs bits (the bits above are the bucket's number), so sorting and
// deduplicating them is building a set of 2^(bbits + rvs) bits. A filter qualifies when that
// set fits K4_BITMAP_MAX_BITS, an index owns whole 32-bit words of it (lis + rvs >= 5), and
// the num_unique quirk cannot bite (an index's first entry is compared with UINT32_MAX >>
// value_size, which a fingerprint equals only if fp_size + vs == 32).
inline bool k4_bitmap_filter(const FilterPlan& p, const rf_amd_config& cfg) {
  return p.bbits + p.rvs <= K4_BITMAP_MAX_BITS && cfg.log_index_size + p.rvs >= 5 &&
         cfg.fingerprint_size + p.vs < 32;
}
// The batch takes the bitmap kernel only when every filter qualifies and the build is fresh and
// single-run: old entries (wide, flag32) are never deduplicated, and the runs of a chained batch
// carry different values.
inline bool k4_bitmap_batch(const BatchPlan& b, const rf_amd_config& cfg) {
  if (b.wide || b.flag32 || b.chained || b.plans.empty()) return false;
  for (const FilterPlan& p : b.plans)
    if (!k4_bitmap_filter(p, cfg)) return false;
  return true;
}

// Packed builds (rf_plan.h: IDX_PACKED): a bitmap batch whose K4 can build every index block's
// body from its bit set, so that no sorted entries are written and K6 only places the bodies.
// Bound on the dwords one coarse bucket's bodies take, each starting on a dword. A block of c
// entries has (c + IS - 1) / 8 + 4 encoding bytes and at most c rvs / 8 + 4 remainder bytes
// (k_layout's block_size less the 2-byte count), and up to 3 bytes of padding: over the ipc
// indices of a bucket of `kept` entries that is at most
//   (kept (1 + rvs) + ipc (IS - 1)) / 8 + 11 ipc   bytes,
// which grows with kept <= min(SORT_CAP, 2^(bbits + rvs)).
inline uint32_t k4_pack_bound_dwords(const FilterPlan& p, uint32_t lis) {
  const uint64_t ipc = 1ull << (p.bbits - lis), IS = 1ull << lis;
  const uint64_t kept = std::min<uint64_t>(SORT_CAP, 1ull << (p.bbits + p.rvs));
  return (uint32_t)(((kept * (1 + p.rvs) + ipc * (IS - 1)) / 8 + 11 * ipc) / 4);
}
// A filter packs when a bucket of the filter lies inside one word of the bit set (rvs <= 5) and a
// K4 thread's four words inside one index (lis + rvs >= 7), a coarse bucket's bodies and their
// starts fit the LDS they are staged in (and with it the bucket's region of `part`), and K6
// holds every block of a page in its tables: lines_asm says so, and a filter without lines is
// held to the same bound. (Pages of more blocks are assembled from sorted entries only.)
inline bool k4_pack_filter(const FilterPlan& p, const rf_amd_config& cfg) {
  const uint32_t lis = cfg.log_index_size;
  if (p.rvs > 5 || lis + p.rvs < 7 || p.bbits < lis || (1u << (p.bbits - lis)) > K4_PACK_MAX_IPC) return false;
  if (k4_pack_bound_dwords(p, lis) > K4_PACK_STAGE_DW) return false;
  const uint32_t min_block = 2 + ((1u << lis) - 1) / 8 + 4 + 3;  // (lines_in_assembly)
  return p.lines_asm || (!p.lg_line && cfg.page_size / min_block + 1 <= ASM_MAXB);
}
inline bool k4_pack_batch(const BatchPlan& b, const rf_amd_config& cfg) {
  if (!b.k4_bitmap) return false;
  for (const FilterPlan& p : b.plans)
    if (!k4_pack_filter(p, cfg)) return false;
  return true;
}

// Old filters of an incremental batch: read in place from their batch's sorted entries when
// the geometry allows (32-bit pipeline; the old batch built here, not imported), else decoded
// from the image -- only those join the batch's old-index list and old32
inline void plan_old_filters(BatchPlan& b, const BatchInput& in, const PlanKnobs& knobs) {
  const uint32_t lis = in.cfg->log_index_size, fps = in.cfg->fingerprint_size;
  const bool direct_ok = b.flag32 && !knobs.old_decode;
  uint32_t* po = b.pre_of(PRE_OIDX);  // decoded old indices per filter
  for (uint32_t f = 0; f < b.F; f++) {
    po[f + 1] = po[f];
    if (!in.olds || !in.olds[f].present) continue;
    const OldFilter& o = in.olds[f];
    const FilterPlan* op = o.plan;
    FilterPlan& p = b.plans[f];
    // in place also across a geometry change (lnb grew: rounds 2, 3 and 5 of the compaction
    // chain), as long as each new coarse bucket lies inside one old one (cbits did not shrink)
    // (old_resplit_off: decode those, for A/B)
    const bool same_cfg = direct_ok && o.has_entries && o.fingerprint_size == fps && o.log_index_size == lis;
    const bool same_geo = op->lnb == p.lnb && op->cbits == p.cbits;
    const bool resplit = p.cbits >= op->cbits && p.lnb >= op->lnb && !knobs.old_resplit_off;
    if (same_cfg && (same_geo || resplit)) {
      p.old_direct = 1;
      p.old_cbits = op->cbits;
      p.old_bbits = op->bbits;
      continue;
    }
    p.old_idx_base = b.num_old_idx;
    p.old_first = b.old_total;
    b.old_total += p.old_region;
    b.num_old_idx += op->num_indices;
    po[f + 1] += p.old_num_indices;
  }
}

// tile maps of a chained batch (see BatchPlan)
inline void cut_tiles(BatchPlan& b, const BatchInput& in, const std::vector<uint32_t>& run_first) {
  for (std::vector<uint32_t>* v : {&b.tile_filter, &b.tile_start, &b.tile_value, &b.tile_end}) v->reserve(b.num_tiles);
  for (uint32_t f = 0; f < b.F; f++) {
    uint32_t first = 0;
    for (uint32_t r = run_first[f]; r < run_first[f + 1]; r++) {
      const uint32_t end = first + in.run_len[r];
      for (uint32_t s0 = first; s0 < end; s0 += TILE_KEYS) {
        b.tile_filter.push_back(f);
        b.tile_start.push_back(s0);
        b.tile_value.push_back(in.run_value[r]);
        b.tile_end.push_back(std::min(end, s0 + (uint32_t)TILE_KEYS));
      }
      first = end;
    }
  }
}

// The plan of a batch to build (rf_amd_batch_create, rf_amd_batch_create_runs).
inline int plan_batch(const BatchInput& in0, const PlanKnobs& knobs, BatchPlan* out, std::string* err) {
  BatchInput in = in0;
  if (in.num_runs && in.run_len && in.run_value) {
    // one run per filter: exactly the plain batch (runs and filters then share their index)
    bool single = true;
    for (uint32_t f = 0; f < in.num_filters && single; f++) single = in.num_runs[f] == 1;
    if (single) {
      for (uint32_t f = 0; f < in.num_filters; f++)
        if (in.run_len[f] == 0) return plan_fail(err, RF_AMD_EINVAL, "zero-length run");
      in.num_new = in.run_len;
      in.value = in.run_value;
      in.num_runs = nullptr;
    }
  }
  if (int rc = check_config(in.cfg, err)) return rc;
  if (in.num_filters == 0 || !(in.num_runs ? (in.run_len && in.run_value) : in.num_new != nullptr))
    return plan_fail(err, RF_AMD_EINVAL, "empty batch");
  const rf_amd_config& cfg = *in.cfg;
  const uint32_t F = in.num_filters;
  std::vector<uint32_t> run_first, run_total;  // chained: first run, inputs per filter
  if (in.num_runs) {
    if (int rc = check_runs(in, &run_first, &run_total, err)) return rc;
    in.num_new = run_total.data();
  }
  BatchPlan& b = *out;
  b = BatchPlan();
  b.F = F;
  b.chained = in.num_runs != nullptr;
  b.plans.resize(F);
  b.pre.assign((size_t)NUM_PRE * (F + 1), 0u);
  const uint32_t lis = cfg.log_index_size;
  for (uint32_t f = 0; f < F; f++) {
    FilterPlan& p = b.plans[f];
    memset(&p, 0, sizeof(p));
    const FilterPlan* op = nullptr;
    if (in.olds && in.olds[f].present) {
      const OldFilter& o = in.olds[f];
      if (!o.plan || !o.built || !o.same_device) return plan_fail(err, RF_AMD_EINVAL, "bad old filter reference");
      op = o.plan;
      b.wide = true;
    }
    const uint32_t v = b.chained ? in.run_value[run_first[f + 1] - 1] : in.value ? in.value[f] : 0;
    if (int rc = filter_geometry(cfg, in.num_new[f], v, op, &p, err)) return rc;
    p.e_first = b.E;
    p.key_first = b.keys_total;
    p.cb_base = b.CB;
    p.idx_base = b.I;
    p.page_base = b.PS;
    p.pf_base = b.PF;
    probe_geometry(p, cfg, knobs, !op && !b.chained, &b.NL, &b.line_lmax, &b.lines_dense);
    const int la = p.lg_line ? lines_in_assembly(lis, p.lg_line, cfg.page_size) : 0;
    p.lines_asm = la != 0;
    p.lines_flag = la == 2;
    if (p.lg_line && la != 1) b.plines_needed = true;
    uint32_t ntiles = (p.num_new + TILE_KEYS - 1) / TILE_KEYS;
    if (b.chained) {
      // the last chain step's group width (num_unique quirk): from the filter that step starts
      // from -- the old filter plus every run but the last; tiles end at run boundaries
      const uint64_t prev_fp = (uint64_t)p.num_fp - in.run_len[run_first[f + 1] - 1];
      p.npo = prev_fp ? p.num_indices / num_indices_of(prev_fp, lis) : 1u;
      ntiles = 0;
      for (uint32_t r = run_first[f]; r < run_first[f + 1]; r++) ntiles += (in.run_len[r] + TILE_KEYS - 1) / TILE_KEYS;
    }
    auto pre = [&](int k, uint32_t count) { b.pre_of(k)[f + 1] = b.pre_of(k)[f] + count; };
    pre(PRE_TILE, ntiles);
    pre(PRE_OTILE, (p.old_region + TILE_KEYS - 1) / TILE_KEYS);
    pre(PRE_CB, 1u << p.cbits);
    pre(PRE_PG, p.page_cap);
    pre(PRE_IDX, p.num_indices);
    b.E += p.num_fp;
    b.keys_total += p.num_new;
    b.CB += 1u << p.cbits;
    b.I += p.num_indices;
    b.PS += p.page_cap;
    b.PF += p.page_cap + 1;
  }
  if (b.wide) {
    // 32-bit entries when (e << 1) | flag fits: fp_size + value_size <= 31 in every filter
    b.flag32 = !knobs.wide64;
    for (const auto& p : b.plans) b.flag32 = b.flag32 && cfg.fingerprint_size + p.vs <= 31;
  }
  if (!b.wide || b.flag32) {
    // fresh and 32-bit incremental builds: the fused kernel partitions the new keys straight
    // into SORT_CAP slots per coarse bucket (k_hash_scatter), so each filter's entry region is
    // its buckets' regions (>= its num_fingerprints: incremental builds' sorted entries, laid
    // out by the scan of new + old counts, fit in it too)
    b.E = 0;
    for (auto& p : b.plans) {
      p.e_first = b.E;
      b.E += (uint64_t)CB_REGION << p.cbits;
    }
  }
  if (b.wide) plan_old_filters(b, in, knobs);
  b.lay_seg = knobs.layout_seg;
  if (cfg.page_size > MAX_PAGE || F >= (1u << 26)) b.lay_seg = 0;
  assign_layout(b);
  b.k4_bitmap = k4_bitmap_batch(b, cfg);
  b.k4_pack = k4_pack_batch(b, cfg);
  b.num_tiles = b.pre_of(PRE_TILE)[F];
  b.num_old_tiles = b.pre_of(PRE_OTILE)[F];
  if (b.NL > 0xffffffffull) return plan_fail(err, RF_AMD_EINVAL, "batch too large (probe lines > 2^32)");
  b.pplans.resize(F);
  for (uint32_t f = 0; f < F; f++) b.pplans[f] = pack_pplan(b.plans[f]);
  if (b.chained) cut_tiles(b, in, run_first);
  return 0;
}

// The probe-side plan of images imported as a built, probe-only batch (rf_amd_batch_import):
// filter f's pages are the num_pages[f] pages after those of the filters before it, its
// probe lines always come from k_plines.
inline int plan_import(const rf_amd_config* cfgp, uint32_t F, const rf_amd_filter_info* infos,
                       const PlanKnobs& knobs, BatchPlan* out, std::string* err) {
  if (int rc = check_config(cfgp, err)) return rc;
  if (F == 0 || !infos) return plan_fail(err, RF_AMD_EINVAL, "bad image");
  const rf_amd_config& cfg = *cfgp;
  const uint32_t lis = cfg.log_index_size;
  BatchPlan& b = *out;
  b = BatchPlan();
  b.F = F;
  b.plans.resize(F);
  b.pplans.resize(F);
  uint64_t pages_total = 0, idx_total = 0;
  for (uint32_t f = 0; f < F; f++) {
    const rf_amd_filter_info& in = infos[f];
    FilterPlan& p = b.plans[f];
    memset(&p, 0, sizeof(p));
    const uint32_t lnb = in.num_fingerprints ? log_buckets_of(in.num_fingerprints, lis) : lis;
    if (in.num_fingerprints == 0 || lnb > cfg.fingerprint_size || (1u << (lnb - lis)) > MAX_INDICES ||
        in.num_indices != (1u << (lnb - lis)) || in.value_size > 32 - cfg.fingerprint_size || in.error ||
        in.num_pages == 0)
      return plan_fail(err, RF_AMD_EINVAL, "image geometry out of range (filter " + std::to_string(f) + ")");
    p.num_fp = in.num_fingerprints;
    p.lnb = lnb;
    p.vs = in.value_size;
    p.num_indices = in.num_indices;
    p.page_cap = in.num_pages;
    p.page_base = (uint32_t)pages_total;
    p.idx_base = (uint32_t)idx_total;
    probe_geometry(p, cfg, knobs, true, &b.NL, &b.line_lmax, &b.lines_dense);
    if (p.lg_line) b.plines_needed = true;
    b.pplans[f] = pack_pplan(p);
    pages_total += in.num_pages;
    idx_total += p.num_indices;
  }
  if (b.NL >= (1ull << 32) || pages_total >= (1ull << 32)) return plan_fail(err, RF_AMD_EINVAL, "import too large");
  b.PS = (uint32_t)pages_total;
  b.I = (uint32_t)idx_total;
  return 0;
}

}  // namespace rf
