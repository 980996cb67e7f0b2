// k4_pack_check -- which bitmap batches are built packed (k4_pack_batch in
// splinterdb_amd/csrc/rf_batch_plan.h: K4 writes index-block bodies, K6 places them), and the
// bound on a coarse bucket's staged bodies, checked on the host. Built and run by
// tests/test_k4_pack_plan.py; needs no device. Prints one "case <name> <packs> <rvs>" line per
// planned batch, one "sweep <plans> <packed>" line, then "k4_pack_check: OK".
#include <stdio.h>

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

static rf_amd_config config(uint32_t fp, uint32_t lis) { return rf_amd_config{fp, lis, 42, 4096, 32}; }

static int plan(const rf_amd_config& cfg, const std::vector<uint32_t>& n, const std::vector<uint16_t>& v,
                const std::vector<OldFilter>& olds, BatchPlan* out) {
  BatchInput in;
  in.cfg = &cfg;
  in.num_filters = (uint32_t)n.size();
  in.num_new = n.data();
  in.value = v.data();
  in.olds = olds.empty() ? nullptr : olds.data();
  return plan_batch(in, PlanKnobs(), out, nullptr);
}

static void report(const char* name, const BatchPlan& b) {
  printf("case %s %d %u\n", name, b.k4_pack ? 1 : 0, b.plans[0].rvs);
}

// dwords the bodies of one coarse bucket take when its `kept` entries fill the indices one after
// the other, `per` to an index (the last one partly), the rest empty
static uint32_t bodies(uint32_t kept, uint32_t per, uint32_t ipc, uint32_t IS, uint32_t rvs) {
  uint32_t dw = 0;
  for (uint32_t l = 0; l < ipc; l++) {
    const uint32_t c = kept < per ? kept : per;
    kept -= c;
    dw += pack_body_dwords(c, IS, rvs);
  }
  return dw;
}

// one filter that packs: everything K4's packed path relies on
static void check_packed_filter(const FilterPlan& p, const rf_amd_config& cfg) {
  const uint32_t lis = cfg.log_index_size, IS = 1u << lis, ipc = 1u << (p.bbits - lis);
  CHECK(p.rvs <= 5 && lis + p.rvs >= 7 && ipc <= K4_PACK_MAX_IPC && ipc * 4 <= (uint32_t)SORT_NT * 4);
  CHECK(p.bbits + p.rvs <= K4_BITMAP_MAX_BITS);
  CHECK(p.lines_asm || !p.lg_line);
  CHECK(cfg.page_size / (2 + (IS - 1) / 8 + 4 + 3) + 1 <= ASM_MAXB);
  const uint32_t bound = k4_pack_bound_dwords(p, lis);
  CHECK(bound <= K4_PACK_STAGE_DW && bound <= CB_REGION);
  // the bound against the bodies themselves: every entry the bucket can keep, spread evenly,
  // one to an index, and packed into as few indices as their capacity (2^(lis + rvs) distinct
  // keys) allows; and the same with fewer entries
  const uint32_t cap = 1u << (lis + p.rvs);
  const uint32_t kmax = (uint32_t)std::min<uint64_t>(SORT_CAP, 1ull << (p.bbits + p.rvs));
  for (uint32_t kept : {kmax, kmax - 1, kmax / 2 + 1, ipc, 1u, 0u}) {
    if (kept > kmax) continue;
    for (uint32_t per : {cap, (kept + ipc - 1) / ipc, 1u, 7u, 9u}) {
      if (per == 0 || per > cap || (uint64_t)per * ipc < kept) continue;
      CHECK(bodies(kept, per, ipc, IS, p.rvs) <= bound);
    }
  }
}

int main() {
  BatchPlan b;
  // C2 packs: rvs 4, 16 indices of 256 buckets per coarse bucket, lines cut by K6
  {
    const rf_amd_config cfg = config(26, 8);
    CHECK(plan(cfg, std::vector<uint32_t>(8, 8000000u), std::vector<uint16_t>(8, 0), {}, &b) == 0);
    const FilterPlan& p = b.plans[0];
    CHECK(p.rvs == 4 && p.bbits == 12 && p.lines_asm && b.k4_bitmap && b.k4_pack);
    for (const FilterPlan& q : b.plans) check_packed_filter(q, cfg);
    report("c2", b);
  }
  // C3 is no bitmap batch
  {
    const rf_amd_config cfg = config(26, 8);
    CHECK(plan(cfg, {1u << 20}, {0}, {}, &b) == 0);
    CHECK(!b.k4_bitmap && !b.k4_pack);
    report("c3", b);
  }
  // the shapes of tests/k4_pack_cases.py (the first five: those of test_gpu_k4_bitmap.py)
  {
    struct S { uint32_t fp, lis, n; uint16_t v; uint32_t rvs; bool bitmap, packs; const char* name; };
    const S shapes[] = {{18, 8, 20000, 0, 4, true, true, "s_20000"},
                        {18, 4, 40000, 1, 4, true, false, "s_40000_v1"},  // lis 4: K6 does not hold a page's blocks
                        {18, 8, 100000, 3, 4, true, true, "s_100000_v3"},
                        {18, 8, 100000, 0, 2, true, true, "s_100000"},
                        {18, 8, 300000, 0, 0, true, true, "s_300000"},
                        {18, 3, 70000, 0, 2, true, false, "lis3"},    // wsh 0: a thread's words span four indices
                        {16, 8, 1500, 0, 6, true, false, "rvs6"},     // a bucket's bits span two words
                        {16, 9, 6000, 0, 4, true, true, "lis9_count"}};
    for (const S& s : shapes) {
      const rf_amd_config cfg = config(s.fp, s.lis);
      CHECK(plan(cfg, {s.n}, {s.v}, {}, &b) == 0);
      const FilterPlan& p = b.plans[0];
      CHECK(p.rvs == s.rvs && b.k4_bitmap == s.bitmap && b.k4_pack == s.packs);
      if (b.k4_pack) check_packed_filter(p, cfg);
      report(s.name, b);
    }
    const rf_amd_config cfg3 = config(18, 3);
    CHECK(plan(cfg3, {70000}, {0}, {}, &b) == 0);
    CHECK(3 + b.plans[0].rvs - 5 < 2 && !b.plans[0].lines_asm);
  }
  // a filter that cannot pack beside ones that can: the whole batch keeps its sorted entries
  {
    const rf_amd_config cfg = config(16, 8);
    CHECK(plan(cfg, {20000u, 1500u}, {0, 0}, {}, &b) == 0);
    CHECK(b.k4_bitmap && k4_pack_filter(b.plans[0], cfg) && !k4_pack_filter(b.plans[1], cfg) && !b.k4_pack);
    report("mixed", b);
  }
  // incremental and chained batches: never
  {
    const rf_amd_config cfg = config(26, 8);
    BatchPlan old;
    CHECK(plan(cfg, {5000000u}, {0}, {}, &old) == 0);
    CHECK(old.k4_pack);
    OldFilter o;
    o.present = true;
    o.plan = &old.plans[0];
    o.fingerprint_size = cfg.fingerprint_size;
    o.log_index_size = cfg.log_index_size;
    o.has_entries = false;  // a packed batch keeps none
    o.built = o.same_device = true;
    CHECK(plan(cfg, {3000000u}, {0}, {o}, &b) == 0);
    CHECK(b.wide && !b.k4_pack && !b.plans[0].old_direct);  // and the old filter is decoded
    report("incremental", b);
    const uint32_t nr2[] = {2}, len2[] = {4000000u, 4000000u};
    const uint16_t val2[] = {0, 1};
    BatchInput in;
    in.cfg = &cfg;
    in.num_filters = 1;
    in.num_runs = nr2;
    in.run_len = len2;
    in.run_value = val2;
    CHECK(plan_batch(in, PlanKnobs(), &b, nullptr) == 0);
    CHECK(b.chained && !b.k4_pack);
    report("chained", b);
  }
  // sweep: every (fingerprint, log_index_size, n, value) the planner accepts
  {
    uint64_t plans = 0, packed = 0;
    const uint16_t values[] = {0, 1, 3, 31};
    for (uint32_t fp = 8; fp <= 32; fp++)
      for (uint32_t lis = 3; lis <= MAX_LIS; lis++)
        for (uint32_t lg = 0; lg <= 23; lg++)
          for (uint32_t n : {(1u << lg), (1u << lg) + 1, (3u << lg) / 2, (2u << lg) - 1})
            for (uint16_t v : values) {
              const rf_amd_config cfg = config(fp, lis);
              if (plan(cfg, {n}, {v}, {}, &b) != 0) continue;
              plans++;
              const FilterPlan& p = b.plans[0];
              CHECK(b.k4_pack == (b.k4_bitmap && k4_pack_filter(p, cfg)));
              if (!b.k4_pack) continue;
              packed++;
              check_packed_filter(p, cfg);
            }
    CHECK(plans > 1000 && packed > 100);
    printf("sweep %llu %llu\n", (unsigned long long)plans, (unsigned long long)packed);
  }
  if (g_failed) {
    printf("k4_pack_check: %d FAILED\n", g_failed);
    return 1;
  }
  printf("k4_pack_check: OK\n");
  return 0;
}
