// plan_check -- the batch planner (splinterdb_amd/csrc/rf_batch_plan.h) checked on the host:
// the invariants the kernels rely on, on the smallest inputs that reach each branch. Built
// and run by tests/test_batch_plan.py; needs no device. Prints "ref <lis> <n> <lnb>
// <num_indices> <vs>" lines for that test to compare with the CPU oracle, then "plan_check: OK".
// Each argument fp:lis:n:value:sigma adds a "line <fp> <lis> <n> <value> <sigma> <lg_line> <lnb>
// <rem> <vs> <rvs>" row: the probe geometry the planner gives a fresh filter of n fingerprints
// under PlanKnobs::line_sigma = sigma (tests/test_probe_geometry_cases.py).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "rf_batch_plan.h"

using namespace rf;

static int g_failed = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      g_failed++;                                             \
    }                                                         \
  } while (0)

static rf_amd_config config(uint32_t fp = 26, uint32_t lis = 8) { return rf_amd_config{fp, lis, 42, 4096, 32}; }

// a plain batch: n[f] new fingerprints of value v[f] on top of olds[f]
static int plan(const rf_amd_config& cfg, const std::vector<uint32_t>& n, const std::vector<uint16_t>& v,
                const std::vector<OldFilter>& olds, const PlanKnobs& k, BatchPlan* out, std::string* err = nullptr) {
  BatchInput in;
  in.cfg = &cfg;
  in.num_filters = (uint32_t)n.size();
  in.num_new = n.data();
  in.value = v.empty() ? nullptr : v.data();
  in.olds = olds.empty() ? nullptr : olds.data();
  return plan_batch(in, k, out, err);
}
static int plan1(const rf_amd_config& cfg, uint32_t n, uint16_t v, BatchPlan* out, const OldFilter* old = nullptr,
                 const PlanKnobs& k = PlanKnobs()) {
  return plan(cfg, {n}, {v}, old ? std::vector<OldFilter>{*old} : std::vector<OldFilter>{}, k, out);
}
// a batch of runs: runs[f] = {(len, value), ...}
typedef std::vector<std::pair<uint32_t, uint16_t>> Runs;
static int plan_runs(const rf_amd_config& cfg, const std::vector<Runs>& runs, BatchPlan* out, std::string* err = nullptr) {
  std::vector<uint32_t> nr, len;
  std::vector<uint16_t> val;
  for (const Runs& r : runs) {
    nr.push_back((uint32_t)r.size());
    for (const auto& x : r) {
      len.push_back(x.first);
      val.push_back(x.second);
    }
  }
  BatchInput in;
  in.cfg = &cfg;
  in.num_filters = (uint32_t)runs.size();
  in.num_runs = nr.data();
  in.run_len = len.data();
  in.run_value = val.data();
  return plan_batch(in, PlanKnobs(), out, err);
}

// the descriptor of filter 0 of a built batch `b` of config `cfg`, as the engine would make it
static OldFilter old_of(const BatchPlan& b, const rf_amd_config& cfg) {
  OldFilter o;
  o.present = true;
  o.plan = &b.plans[0];
  o.fingerprint_size = cfg.fingerprint_size;
  o.log_index_size = cfg.log_index_size;
  o.has_entries = true;
  o.wide = b.wide;
  o.built = true;
  o.same_device = true;
  return o;
}

template <typename T>
static bool same_vec(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}
static bool same_plan(const BatchPlan& a, const BatchPlan& b) {
  return a.F == b.F && same_vec(a.plans, b.plans) && same_vec(a.pre, b.pre) && a.wide == b.wide &&
         a.flag32 == b.flag32 && a.chained == b.chained && a.old_total == b.old_total &&
         a.num_tiles == b.num_tiles && a.num_old_tiles == b.num_old_tiles && a.num_old_idx == b.num_old_idx &&
         a.E == b.E && a.keys_total == b.keys_total && a.CB == b.CB && a.I == b.I && a.PS == b.PS &&
         a.PF == b.PF && a.NL == b.NL && a.plines_needed == b.plines_needed && a.line_lmax == b.line_lmax &&
         a.lay_seg == b.lay_seg && a.lay_grid == b.lay_grid && a.lay_whole == b.lay_whole &&
         same_vec(a.lay_wg, b.lay_wg) && same_vec(a.tile_filter, b.tile_filter) &&
         same_vec(a.tile_start, b.tile_start) && same_vec(a.tile_value, b.tile_value) &&
         same_vec(a.tile_end, b.tile_end) && same_vec(a.pplans, b.pplans);
}

static void check_fresh_geometry() {
  const rf_amd_config cfg = config();
  const uint64_t maxfp = max_fingerprints(cfg);
  for (uint64_t n : {(uint64_t)1, (uint64_t)4095, (uint64_t)4096, (uint64_t)8192, maxfp}) {
    BatchPlan b;
    CHECK(plan1(cfg, (uint32_t)n, 0, &b) == 0);
    if (b.plans.empty()) continue;
    const FilterPlan& p = b.plans[0];
    const uint32_t lis = cfg.log_index_size;
    CHECK(p.num_fp == n);
    CHECK(p.cbits + p.bbits == p.lnb);
    CHECK(p.num_indices == 1u << (p.lnb - lis) && p.num_indices <= MAX_INDICES);
    CHECK(p.bbits >= p.binsh && (1u << (p.bbits - p.binsh)) <= MAX_BINS);
    CHECK(p.bbits >= lis && (1u << (p.bbits - lis)) <= MAX_IPC);
    CHECK((1u << p.cbits) <= MAX_CB);
    CHECK(p.page_cap <= p.num_indices);
    CHECK(((uint64_t)CB_REGION << p.cbits) >= p.num_fp);
  }
  BatchPlan b;
  // max + 1 = 2^23 still fits the u32 argument: rejected by the planner, not by the cast
  CHECK(plan1(cfg, (uint32_t)(maxfp + 1), 0, &b) == RF_AMD_EINVAL);
}

static void check_binsh() {
  BatchPlan b;
  CHECK(plan1(config(26, 8), 1u << 20, 0, &b) == 0);
  CHECK(b.plans[0].binsh == 1 && b.plans[0].cbits == b.plans[0].lnb - 13);
  CHECK(plan1(config(26, 8), (uint32_t)((1ull << 20) * 103 / 100), 0, &b) == 0);
  CHECK(b.plans[0].binsh == 0 && b.plans[0].cbits == b.plans[0].lnb - 12);
  // log_index_size 3 never takes the wide coarse buckets (2^(13-3) indices > MAX_IPC). Its
  // routing_filter_max_fingerprints is 2^18 - 1, so 1 << 20 cannot be planned there at all;
  // 1 << 17 is the largest power of two that can, and log_index_size 4 takes them at that size
  CHECK(plan1(config(26, 3), 1u << 20, 0, &b) == RF_AMD_EINVAL);
  CHECK(plan1(config(26, 3), 1u << 17, 0, &b) == 0);
  CHECK(b.plans[0].binsh == 0 && b.plans[0].cbits == b.plans[0].lnb - 12);
  CHECK(plan1(config(26, 4), 1u << 17, 0, &b) == 0);
  CHECK(b.plans[0].binsh == 1);
}

static void check_value_width() {
  BatchPlan b, old;
  CHECK(plan1(config(26), 100, 63, &b) == 0);
  CHECK(b.plans[0].vs == 6 && b.plans[0].value == 63);
  CHECK(plan1(config(26), 100, 64, &b) == RF_AMD_EINVAL);
  CHECK(plan1(config(32), 100, 1, &b) == RF_AMD_EINVAL);
  CHECK(plan1(config(32), 100, 0, &b) == 0);
  CHECK(plan1(config(26), 100, 4, &old) == 0);  // vs 3
  const OldFilter o = old_of(old, config(26));
  CHECK(plan1(config(26), 100, 1, &b, &o) == RF_AMD_EINVAL);
  CHECK(plan1(config(26), 100, 4, &b, &o) == 0);
}

static const std::vector<uint32_t> THREE = {1u << 18, 40000, 1};

static void check_bases() {
  const rf_amd_config cfg = config(22, 4);
  BatchPlan b;
  CHECK(plan(cfg, THREE, {}, {}, PlanKnobs(), &b) == 0);
  uint64_t e = 0, key = 0, lines = 0;
  uint32_t cb = 0, idx = 0, page = 0, pf = 0;
  for (uint32_t f = 0; f < b.F; f++) {
    const FilterPlan& p = b.plans[f];
    CHECK(p.num_new == THREE[f] && p.num_fp == THREE[f]);
    CHECK(p.e_first == e && p.key_first == key && p.cb_base == cb && p.idx_base == idx);
    CHECK(p.page_base == page && p.pf_base == pf && p.line_base == lines);
    e += (uint64_t)CB_REGION << p.cbits;  // fresh batches: the fused build's regions
    key += p.num_new;
    cb += 1u << p.cbits;
    idx += p.num_indices;
    page += p.page_cap;
    pf += p.page_cap + 1;
    if (p.lg_line) lines += (uint64_t)p.num_indices << (cfg.log_index_size - (p.lg_line - 1));
    CHECK(b.pplans[f].x == pplan_word(p) && b.pplans[f].y == p.line_base && b.pplans[f].z == p.idx_base &&
          b.pplans[f].w == 0);
  }
  CHECK(b.E == e && b.keys_total == key && b.CB == cb && b.I == idx && b.PS == page && b.PF == pf && b.NL == lines);
  CHECK(b.pre.size() == (size_t)NUM_PRE * (b.F + 1));
  CHECK(b.pre_of(PRE_TILE)[b.F] == b.num_tiles && b.num_tiles == 16 + 3 + 1);
  CHECK(b.pre_of(PRE_OTILE)[b.F] == b.num_old_tiles && b.num_old_tiles == 0);
  CHECK(b.pre_of(PRE_CB)[b.F] == b.CB);
  CHECK(b.pre_of(PRE_PG)[b.F] == b.PS);
  CHECK(b.pre_of(PRE_IDX)[b.F] == b.I);
  CHECK(b.pre_of(PRE_OIDX)[b.F] == b.num_old_idx && b.num_old_idx == 0);
  for (int k = 0; k < NUM_PRE; k++) CHECK(b.pre_of(k)[0] == 0);
  CHECK(!b.wide && !b.flag32 && !b.chained);
}

// the K5 map of plan b: every split filter's segments once, segment q at w0 + 8 q (its
// predecessor is workgroup w - 8 of the same filter), nothing else
static void check_layout_map(const BatchPlan& b) {
  CHECK(b.lay_grid == b.lay_wg.size());
  std::vector<uint32_t> w0(b.F, ~0u), seen(b.F, 0);
  bool whole = false;
  size_t used = 0;
  for (uint32_t f = 0; f < b.F; f++) {
    const uint32_t G = layout_groups(b.plans[f], b.lay_seg);
    if (G == 1) {
      whole = true;
      continue;
    }
    CHECK(G == b.plans[f].num_indices / b.lay_seg && G <= LAYOUT_MAX_GROUPS);
    for (uint32_t w = 0; w < b.lay_wg.size(); w++)
      if (b.lay_wg[w] == (f << 6)) w0[f] = w;
    CHECK(w0[f] != ~0u);
    for (uint32_t q = 0; q < G && w0[f] != ~0u; q++) {
      const size_t w = w0[f] + 8 * (size_t)q;
      CHECK(w < b.lay_wg.size() && b.lay_wg[w] == (f << 6 | q));
    }
    used += G;
  }
  for (uint32_t x : b.lay_wg) {
    if (x == ~0u) continue;
    CHECK((x >> 6) < b.F && (x & 63) < layout_groups(b.plans[x >> 6], b.lay_seg));
    if ((x >> 6) < b.F) seen[x >> 6]++;
  }
  size_t words = 0;
  for (uint32_t f = 0; f < b.F; f++) {
    const uint32_t G = layout_groups(b.plans[f], b.lay_seg);
    CHECK(seen[f] == (G == 1 ? 0 : G));  // each exactly once, filters of one workgroup not at all
    words += seen[f];
  }
  CHECK(words == used);
  CHECK(b.lay_whole == whole);
}

static void check_layout() {
  const rf_amd_config cfg = config(22, 4);
  for (uint32_t seg : {4096u, 256u, 0u}) {
    PlanKnobs k;
    k.layout_seg = seg;
    BatchPlan b;
    CHECK(plan(cfg, THREE, {}, {}, k, &b) == 0);
    CHECK(b.lay_seg == seg);
    check_layout_map(b);
    const uint32_t g0 = layout_groups(b.plans[0], seg), g1 = layout_groups(b.plans[1], seg);
    if (seg == 4096) CHECK(g0 == 4 && g1 == 1 && b.lay_grid > 0 && b.lay_whole);
    if (seg == 256) CHECK(g0 == 64 && g1 == 8 && b.lay_whole);  // the third filter has one index
    if (seg == 0) CHECK(b.lay_grid == 0 && b.lay_whole);
  }
  // two split filters and nothing else: no filter is laid out whole
  BatchPlan b;
  CHECK(plan(cfg, {1u << 18, 1u << 18}, {}, {}, PlanKnobs(), &b) == 0);
  check_layout_map(b);
  CHECK(!b.lay_whole && b.lay_grid > 0);
  // npo > seg: the put-back groups would straddle segments, so the filter is not split
  BatchPlan old;
  CHECK(plan1(cfg, 1, 0, &old) == 0);
  const OldFilter o = old_of(old, cfg);
  CHECK(plan1(cfg, 1u << 18, 0, &b, &o) == 0);
  CHECK(b.plans[0].num_indices == 16384 && b.plans[0].npo == 16384);
  CHECK(layout_groups(b.plans[0], b.lay_seg) == 1 && b.lay_grid == 0 && b.lay_whole);
}

static void check_chained() {
  const rf_amd_config cfg = config();
  const uint32_t T = TILE_KEYS;
  BatchPlan b;
  CHECK(plan_runs(cfg, {{{5, 0}, {T, 1}, {T + 1, 2}}}, &b) == 0);
  CHECK(b.chained && b.num_tiles == 4 && b.pre_of(PRE_TILE)[1] == 4);
  const uint32_t start[4] = {0, 5, 5 + T, 5 + 2 * T}, end[4] = {5, 5 + T, 5 + 2 * T, 5 + 2 * T + 1};
  const uint32_t run_end[4] = {5, 5 + T, 5 + 2 * T + 1, 5 + 2 * T + 1}, value[4] = {0, 1, 2, 2};
  CHECK(b.tile_filter.size() == 4 && b.tile_start.size() == 4 && b.tile_value.size() == 4 && b.tile_end.size() == 4);
  for (uint32_t t = 0; t < 4 && b.tile_end.size() == 4; t++) {
    CHECK(b.tile_filter[t] == 0 && b.tile_start[t] == start[t] && b.tile_end[t] == end[t]);
    CHECK(b.tile_end[t] == std::min(run_end[t], b.tile_start[t] + T));
    CHECK(b.tile_value[t] == value[t]);
  }
  const FilterPlan& p = b.plans[0];
  CHECK(p.num_new == 2 * T + 6 && p.num_fp == p.num_new && p.value == 2 && p.vs == 2 && b.keys_total == p.num_new);
  // the last step starts from the 5 + T fingerprints before the last run
  CHECK(p.npo == p.num_indices / num_indices_of(5 + T, cfg.log_index_size) && p.npo == 2);
  CHECK(plan_runs(cfg, {{{5, 1}, {5, 1}}}, &b) == RF_AMD_EINVAL);
  CHECK(plan_runs(cfg, {{{5, 2}, {5, 1}}}, &b) == RF_AMD_EINVAL);
  CHECK(plan_runs(cfg, {{{5, 0}, {0, 1}}}, &b) == RF_AMD_EINVAL);
  CHECK(plan_runs(cfg, {{{0, 0}}}, &b) == RF_AMD_EINVAL);
  CHECK(plan_runs(cfg, {{}, {{5, 0}, {5, 1}}}, &b) == RF_AMD_EINVAL);  // a filter without runs
  // one run per filter: the plain batch, byte for byte
  BatchPlan r, q;
  CHECK(plan_runs(config(22, 4), {{{THREE[0], 3}}, {{THREE[1], 0}}, {{THREE[2], 7}}}, &r) == 0);
  CHECK(plan(config(22, 4), THREE, {3, 0, 7}, {}, PlanKnobs(), &q) == 0);
  CHECK(same_plan(r, q) && !r.chained && r.tile_filter.empty());
}

static void check_old_filters() {
  const rf_amd_config cfg = config();
  BatchPlan old, b;
  CHECK(plan1(cfg, 5000, 1, &old) == 0);
  const FilterPlan& op = old.plans[0];
  const OldFilter o = old_of(old, cfg);
  auto decoded = [&](const BatchPlan& p) {  // the old filter joins old32 and the old-index list
    return p.plans[0].old_direct == 0 && p.plans[0].old_first == 0 && p.plans[0].old_idx_base == 0 &&
           p.old_total == op.num_fp && p.num_old_idx == op.num_indices && p.pre_of(PRE_OIDX)[1] == p.num_old_idx;
  };
  CHECK(plan1(cfg, 100, 1, &b, &o) == 0);
  CHECK(b.wide && b.flag32 && b.plans[0].old_direct == 1 && b.old_total == 0 && b.num_old_idx == 0);
  CHECK(b.plans[0].old_cbits == op.cbits && b.plans[0].old_bbits == op.bbits && b.pre_of(PRE_OIDX)[1] == 0);
  CHECK(b.plans[0].old_region == 5000 && b.plans[0].num_fp == 5100 && b.plans[0].npo == 1);
  CHECK(b.num_old_tiles == 1 && b.pre_of(PRE_OTILE)[1] == 1);
  CHECK(b.plans[0].old_pages == nullptr && b.plans[0].old_slots == nullptr && b.plans[0].old_entries == nullptr &&
        b.plans[0].old_idx_start == nullptr && b.plans[0].old_idx_cnt == nullptr &&
        b.plans[0].old_out == nullptr);  // the engine's to fill in
  // the planner does not (and cannot) tell a rejected old filter from a healthy one: its error
  // bits are on the device, perhaps still to be written; the kernels test them (old_error)
  CHECK(old_error(b.plans[0]) == 0);
  PlanKnobs k;
  k.old_decode = true;
  CHECK(plan1(cfg, 100, 1, &b, &o, k) == 0);
  CHECK(b.flag32 && decoded(b));
  OldFilter imported = o;
  imported.has_entries = false;
  CHECK(plan1(cfg, 100, 1, &b, &imported) == 0);
  CHECK(b.flag32 && decoded(b));
  CHECK(plan1(cfg, 100, 63, &b, &o) == 0);  // fp + vs == 32: 64-bit entries
  CHECK(b.wide && !b.flag32 && decoded(b) && b.E == 5100);
  k = PlanKnobs();
  k.wide64 = true;
  CHECK(plan1(cfg, 100, 1, &b, &o, k) == 0);
  CHECK(!b.flag32 && decoded(b));
  // fewer coarse buckets than the old filter: with one config cbits never shrinks as a filter
  // grows, so the descriptor is made to say so
  FilterPlan finer = op;
  finer.cbits += 1;
  finer.bbits -= 1;
  OldFilter of = o;
  of.plan = &finer;
  CHECK(plan1(cfg, 100, 1, &b, &of) == 0);
  CHECK(b.plans[0].cbits < finer.cbits && decoded(b));
  // lnb grew (5000 -> 10000 fingerprints): in place by re-splitting, unless switched off
  CHECK(plan1(cfg, 5000, 1, &b, &o) == 0);
  CHECK(b.plans[0].lnb == op.lnb + 1 && b.plans[0].cbits >= op.cbits && b.plans[0].old_direct == 1);
  k = PlanKnobs();
  k.old_resplit_off = true;
  CHECK(plan1(cfg, 5000, 1, &b, &o, k) == 0);
  CHECK(b.plans[0].lnb == op.lnb + 1 && decoded(b));
  CHECK(plan1(cfg, 100, 1, &b, &o, k) == 0);  // same geometry: still in place
  CHECK(b.plans[0].old_direct == 1);
  // a batch of another routing config offers its image only
  OldFilter other = o;
  other.log_index_size = 9;
  CHECK(plan1(cfg, 100, 1, &b, &other) == 0);
  CHECK(decoded(b));
  OldFilter bad = o;
  bad.built = false;
  std::string err;
  CHECK(plan(cfg, {100}, {1}, {bad}, PlanKnobs(), &b, &err) == RF_AMD_EINVAL && err == "bad old filter reference");
  bad = o;
  bad.same_device = false;
  CHECK(plan1(cfg, 100, 1, &b, &bad) == RF_AMD_EINVAL);
  bad = o;
  bad.plan = nullptr;  // no such filter in the old batch
  CHECK(plan1(cfg, 100, 1, &b, &bad) == RF_AMD_EINVAL);
  // two filters, the second decoded: its old indices start the batch's list
  CHECK(plan(cfg, {100, 100}, {1, 1}, {o, imported}, PlanKnobs(), &b) == 0);
  CHECK(b.plans[0].old_direct == 1 && b.plans[1].old_direct == 0 && b.plans[1].old_idx_base == 0 &&
        b.plans[1].old_first == 0 && b.old_total == op.num_fp && b.num_old_idx == op.num_indices);
  CHECK(b.pre_of(PRE_OIDX)[1] == 0 && b.pre_of(PRE_OIDX)[2] == b.num_old_idx);
}

static void check_import() {
  const rf_amd_config cfg = config();
  BatchPlan b, im;
  CHECK(plan(cfg, {70000, 300}, {5, 0}, {}, PlanKnobs(), &b) == 0);
  std::vector<rf_amd_filter_info> infos;
  for (const FilterPlan& p : b.plans) infos.push_back(rf_amd_filter_info{p.num_fp, p.num_fp, p.vs, p.num_indices, 3, 0});
  CHECK(plan_import(&cfg, 2, infos.data(), PlanKnobs(), &im, nullptr) == 0);
  CHECK(im.F == 2 && im.I == b.I && im.PS == 6 && im.NL == b.NL && im.line_lmax == b.line_lmax);
  for (uint32_t f = 0; f < 2 && im.F == 2; f++) {
    const FilterPlan &p = b.plans[f], &q = im.plans[f];
    CHECK(q.vs == p.vs && q.rem == p.rem && q.rvs == p.rvs && q.lg_line == p.lg_line && q.lnb == p.lnb);
    CHECK(q.line_base == p.line_base && q.idx_base == p.idx_base && q.page_base == 3 * f && q.page_cap == 3);
    CHECK(im.pplans[f].x == b.pplans[f].x && im.pplans[f].y == b.pplans[f].y && im.pplans[f].z == b.pplans[f].z);
    CHECK(q.lines_asm == 0);  // an import's lines always come from k_plines
  }
  CHECK(im.plines_needed == (im.NL != 0) && im.NL != 0);
  std::string err;
  auto rejected = [&](rf_amd_filter_info bad) {
    std::vector<rf_amd_filter_info> v = infos;
    v[1] = bad;
    return plan_import(&cfg, 2, v.data(), PlanKnobs(), &im, &err) == RF_AMD_EINVAL &&
           err == "image geometry out of range (filter 1)";
  };
  rf_amd_filter_info bad = infos[1];
  bad.num_indices *= 2;
  CHECK(rejected(bad));
  bad = infos[1];
  bad.value_size = 32 - cfg.fingerprint_size + 1;
  CHECK(rejected(bad));
  bad.value_size = 32 - cfg.fingerprint_size;
  CHECK(!rejected(bad));
  bad = infos[1];
  bad.num_pages = 0;
  CHECK(rejected(bad));
  bad = infos[1];
  bad.error = RF_AMD_ERR_PAGE_CAP;
  CHECK(rejected(bad));
  bad = infos[1];
  bad.num_fingerprints = 0;
  CHECK(rejected(bad));
  CHECK(plan_import(&cfg, 0, infos.data(), PlanKnobs(), &im, &err) == RF_AMD_EINVAL);
}

static void check_line_sigma() {
  // a wider margin never gives a larger group
  for (uint32_t rvs : {0u, 6u, 14u, 20u, 32u, 33u})
    for (double lam : {0.5, 1.0, 1.99}) {
      const uint32_t a = line_log_group(8, rvs, lam, 3.5), b = line_log_group(8, rvs, lam, 8.0);
      CHECK(b <= a && a <= 7);
      CHECK((rvs > 32) == (a == 0));
    }
  PlanKnobs k;
  k.line_sigma = 8.0;
  BatchPlan a, b;
  CHECK(plan1(config(), 70000, 5, &a) == 0 && plan1(config(), 70000, 5, &b, nullptr, k) == 0);
  CHECK(b.plans[0].lg_line <= a.plans[0].lg_line && b.NL >= a.NL);
}

// one "line" row per argument fp:lis:n:value:sigma (sigma is echoed as given)
static void print_line_rows(int argc, char** argv) {
  for (int i = 1; i < argc; i++) {
    unsigned fp, lis, n, value;
    char sigma[64];
    if (sscanf(argv[i], "%u:%u:%u:%u:%63s", &fp, &lis, &n, &value, sigma) != 5) {
      printf("bad argument %s\n", argv[i]);
      g_failed++;
      continue;
    }
    PlanKnobs k;
    k.line_sigma = atof(sigma);
    BatchPlan b;
    CHECK(plan1(config(fp, lis), n, (uint16_t)value, &b, nullptr, k) == 0);
    if (b.plans.empty()) continue;
    const FilterPlan& p = b.plans[0];
    printf("line %u %u %u %u %s %u %u %u %u %u\n", fp, lis, n, value, sigma, p.lg_line, p.lnb, p.rem, p.vs, p.rvs);
  }
}

int main(int argc, char** argv) {
  check_fresh_geometry();
  check_binsh();
  check_value_width();
  check_bases();
  check_layout();
  check_chained();
  check_old_filters();
  check_import();
  check_line_sigma();
  for (uint32_t lis : {4u, 8u})
    for (uint32_t n : {1u, 300u, 5000u, 70000u}) {
      BatchPlan b;
      CHECK(plan1(config(26, lis), n, 0, &b) == 0);
      printf("ref %u %u %u %u %u\n", lis, n, b.plans[0].lnb, b.plans[0].num_indices, b.plans[0].vs);
    }
  print_line_rows(argc, argv);
  if (g_failed) {
    printf("plan_check: %d checks FAILED\n", g_failed);
    return 1;
  }
  printf("plan_check: OK\n");
  return 0;
}
