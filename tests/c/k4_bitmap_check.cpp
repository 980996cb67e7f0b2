// k4_bitmap_check -- which batches take K4's bitmap kernel (k4_bitmap_batch in
// splinterdb_amd/csrc/rf_batch_plan.h), checked on the host. Built and run by
// tests/test_k4_bitmap_plan.py; needs no device. Prints one "case <name> <eligible> <key bits>"
// line per planned batch, then "k4_bitmap_check: OK".
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

// widest in-bucket key of the batch
static uint32_t key_bits(const BatchPlan& b) {
  uint32_t kw = 0;
  for (const FilterPlan& p : b.plans) kw = std::max(kw, p.bbits + p.rvs);
  return kw;
}
static void report(const char* name, const BatchPlan& b) {
  printf("case %s %d %u\n", name, b.k4_bitmap ? 1 : 0, key_bits(b));
}

int main() {
  BatchPlan b;
  // C2: 8 filters of 8,000,000 keys, fingerprint 26, log_index_size 8
  {
    const rf_amd_config cfg = config(26, 8);
    CHECK(plan(cfg, std::vector<uint32_t>(8, 8000000u), std::vector<uint16_t>(8, 0), {}, &b) == 0);
    const FilterPlan& p = b.plans[0];
    CHECK(p.lnb == 22 && p.rem == 4 && p.vs == 0 && p.cbits == 10 && p.bbits == 12);
    CHECK(p.bbits + p.rvs == 16 && b.k4_bitmap);
    for (const FilterPlan& q : b.plans) CHECK(k4_bitmap_filter(q, cfg));
    report("c2", b);
  }
  // C3: 2^20 keys -- 13 bucket bits (binsh 1) and 6 remainder bits
  {
    const rf_amd_config cfg = config(26, 8);
    CHECK(plan(cfg, {1u << 20}, {0}, {}, &b) == 0);
    CHECK(b.plans[0].bbits + b.plans[0].rvs == 19 && !b.k4_bitmap);
    report("c3", b);
  }
  // fingerprint 26 with value 63: fp_size + vs = 32 (and the key is wider anyway)
  {
    const rf_amd_config cfg = config(26, 8);
    CHECK(plan(cfg, {8000000u}, {63}, {}, &b) == 0);
    CHECK(b.plans[0].vs == 6 && !b.k4_bitmap);
    report("fp26_value63", b);
    // the clause on its own: a 16-bit key whose fingerprint could equal UINT32_MAX >> vs
    FilterPlan p = b.plans[0];
    p.bbits = 6;
    p.rvs = 10;
    CHECK(p.bbits + p.rvs == 16 && !k4_bitmap_filter(p, cfg));
    p.vs = 5;
    CHECK(k4_bitmap_filter(p, cfg));
  }
  // an index must own whole bitmap words: lis + rvs >= 5
  {
    const rf_amd_config cfg = config(18, 3);
    CHECK(plan(cfg, {(1u << 18) - 1}, {0}, {}, &b) == 0);  // lnb 17: rem 1, rvs 1
    CHECK(b.plans[0].rvs == 1 && b.plans[0].bbits + b.plans[0].rvs <= K4_BITMAP_MAX_BITS && !b.k4_bitmap);
    report("narrow_index", b);
  }
  // the shapes of tests/test_gpu_k4_bitmap.py (fingerprint 18): key widths 16, 16, 16, 14, 12
  {
    struct S { uint32_t lis, n; uint16_t v; uint32_t kw, vs, rvs; const char* name; };
    const S shapes[] = {{8, 20000, 0, 16, 0, 4, "s_20000"},  {4, 40000, 1, 16, 1, 4, "s_40000_v1"},
                        {8, 100000, 3, 16, 2, 4, "s_100000_v3"}, {8, 100000, 0, 14, 0, 2, "s_100000"},
                        {8, 300000, 0, 12, 0, 0, "s_300000"}};
    for (const S& s : shapes) {
      const rf_amd_config cfg = config(18, s.lis);
      CHECK(plan(cfg, {s.n}, {s.v}, {}, &b) == 0);
      const FilterPlan& p = b.plans[0];
      CHECK(p.bbits + p.rvs == s.kw && p.vs == s.vs && p.rvs == s.rvs && b.k4_bitmap);
      CHECK(p.binsh == 0 || s.n != 20000);  // 20,000 > 16,810: bins of one bucket, 4 coarse buckets
      if (s.n == 20000) CHECK(p.cbits == 2);
      report(s.name, b);
    }
  }
  // one ineligible filter among eligible ones: the whole batch takes the sort
  {
    const rf_amd_config cfg = config(26, 8);
    CHECK(plan(cfg, {8000000u, 1u << 20, 8000000u}, {0, 0, 0}, {}, &b) == 0);
    CHECK(k4_bitmap_filter(b.plans[0], cfg) && !k4_bitmap_filter(b.plans[1], cfg) &&
          k4_bitmap_filter(b.plans[2], cfg) && !b.k4_bitmap);
    report("mixed", b);
  }
  // incremental batches: never, whatever the geometry (32-bit flagged and 64-bit entries)
  {
    const rf_amd_config cfg = config(26, 8);
    BatchPlan old;
    CHECK(plan(cfg, {4000000u}, {0}, {}, &old) == 0);
    const OldFilter o = old_of(old, cfg);
    CHECK(plan(cfg, {4000000u}, {0}, {o}, &b) == 0);
    CHECK(b.wide && b.flag32 && b.plans[0].bbits + b.plans[0].rvs == 16 && k4_bitmap_filter(b.plans[0], cfg) &&
          !b.k4_bitmap);
    report("incremental32", b);
    // a fresh filter beside an incremental one: the batch is wide
    CHECK(plan(cfg, {4000000u, 8000000u}, {0, 0}, {o, OldFilter()}, &b) == 0);
    CHECK(b.wide && !b.k4_bitmap);
    report("incremental_mixed", b);
    const rf_amd_config cfg31 = config(31, 8);  // fp_size + vs = 32 with value 1: 64-bit entries
    BatchPlan old31;
    CHECK(plan(cfg31, {4000000u}, {0}, {}, &old31) == 0);
    const OldFilter o31 = old_of(old31, cfg31);
    CHECK(plan(cfg31, {4000000u}, {1}, {o31}, &b) == 0);
    CHECK(b.wide && !b.flag32 && !b.k4_bitmap);
    report("incremental64", b);
  }
  // chained batches: never; runs of length one per filter are the plain batch
  {
    const rf_amd_config cfg = config(26, 8);
    const uint32_t nr2[] = {2}, len2[] = {4000000u, 4000000u};
    const uint16_t val2[] = {0, 1};
    BatchInput in;
    in.cfg = &cfg;
    in.num_filters = 1;
    in.num_runs = nr2;
    in.run_len = len2;
    in.run_value = val2;
    CHECK(plan_batch(in, PlanKnobs(), &b, nullptr) == 0);
    CHECK(b.chained && !b.k4_bitmap);
    report("chained", b);
    const uint32_t nr1[] = {1}, len1[] = {8000000u};
    const uint16_t val1[] = {0};
    in.num_runs = nr1;
    in.run_len = len1;
    in.run_value = val1;
    CHECK(plan_batch(in, PlanKnobs(), &b, nullptr) == 0);
    CHECK(!b.chained && b.k4_bitmap);
    report("single_run", b);
  }
  if (g_failed) {
    printf("k4_bitmap_check: %d FAILED\n", g_failed);
    return 1;
  }
  printf("k4_bitmap_check: OK\n");
  return 0;
}
