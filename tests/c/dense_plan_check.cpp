// dense_plan_check -- which filters the planner (splinterdb_amd/csrc/rf_batch_plan.h) gives dense
// probe lines, checked on the host. Built and run by tests/test_probe_dense_cases.py; needs no
// device. With the knob unset only a fresh filter whose line table outgrows one XCD's L2 takes
// them: the C2 shape does, the C3 / C4 / C5 shapes, every round of the compaction chain and small
// filters keep the current format. Each argument fp:lis:n:value adds a "dense <fp> <lis> <n>
// <value> <lg_line forced> <lg_line default> <lines forced>" row for the test to compare with its
// numpy restatement. Ends with "dense_plan_check: OK".
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "rf_batch_plan.h"

using namespace rf;

static int g_failed = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      g_failed++;                                                  \
    }                                                              \
  } while (0)

static rf_amd_config config(uint32_t fp = 26, uint32_t lis = 8) { return rf_amd_config{fp, lis, 42, 4096, 32}; }

static PlanKnobs knobs(int dense) {
  PlanKnobs k;
  k.lines_dense = dense;
  return k;
}

static int plan1(const rf_amd_config& cfg, uint32_t n, uint16_t v, const PlanKnobs& k, BatchPlan* out,
                 const OldFilter* old = nullptr) {
  BatchInput in;
  in.cfg = &cfg;
  in.num_filters = 1;
  in.num_new = &n;
  in.value = &v;
  in.olds = old;
  return plan_batch(in, k, out, nullptr);
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

// the plan's line count is its filters' lines_per_index, whatever the format
static void check_lines(const BatchPlan& b, const rf_amd_config& cfg) {
  uint64_t lines = 0;
  for (const FilterPlan& p : b.plans) {
    CHECK(p.line_base == lines);
    CHECK(!line_is_dense(p.lg_line) || b.lines_dense);
    if (p.lg_line) lines += (uint64_t)p.num_indices * lines_per_index(cfg.log_index_size, p.lg_line);
    if (line_is_dense(p.lg_line)) {
      const uint32_t G = line_group(p.lg_line), U = line_unary_bits(G, p.rvs);
      CHECK(G >= 1 && G <= 64 && U <= LINE_UNARY_MAX && U >= G);
      CHECK((U - G) * (1 + p.rvs) <= 512 - G);  // the entries the unary region counts have their fields
      CHECK(lines_per_index(cfg.log_index_size, p.lg_line) <= 256);
    }
  }
  CHECK(b.NL == lines);
}

static void check_c2_goes_dense() {
  BatchPlan b, off, imp;
  CHECK(plan1(config(), 8000000, 0, knobs(-1), &b) == 0);
  const FilterPlan& p = b.plans[0];
  // lambda 1.907, rvs 4: seven lines of 37 buckets per index, 95 entries, 132 unary bits
  CHECK(p.lg_line == (LINE_DENSE | 36) && p.rvs == 4);
  CHECK(lines_per_index(8, p.lg_line) == 7 && line_unary_bits(37, 4) == 132);
  CHECK(b.NL == 16384ull * 7 && b.line_lmax == 7 && b.lines_dense);
  CHECK(b.pplans[0].x >> 24 == p.lg_line);
  check_lines(b, config());
  CHECK(plan1(config(), 8000000, 0, knobs(0), &off) == 0);
  CHECK(off.plans[0].lg_line == 6 && off.NL == 16384ull * 8 && !off.lines_dense);  // the current format: 32 buckets per line
  // an import of the same image derives the same geometry
  rf_amd_filter_info info;
  memset(&info, 0, sizeof(info));
  info.num_fingerprints = 8000000;
  info.num_indices = 16384;
  info.num_pages = 100;
  const rf_amd_config cfg = config();
  CHECK(plan_import(&cfg, 1, &info, knobs(-1), &imp, nullptr) == 0);
  CHECK(imp.plans[0].lg_line == p.lg_line && imp.NL == b.NL);
}

static void check_the_gate_keeps_the_rest() {
  const rf_amd_config cfg = config();
  BatchPlan b;
  // C3 and C4: 2^20 keys; C5: 2^21; and every filter of at most 300,000 keys
  for (uint32_t n : {1u << 20, 1u << 21, 300000u, 262144u, 140000u, 70000u, 5000u, 100u, 1u}) {
    CHECK(plan1(cfg, n, 0, knobs(-1), &b) == 0);
    CHECK(!line_is_dense(b.plans[0].lg_line));
    check_lines(b, cfg);
  }
  for (uint32_t lis : {3u, 4u, 6u, 9u, 11u})
    for (uint32_t fp : {12u, 20u, 26u, 32u}) {
      const rf_amd_config c = config(fp, lis);
      const uint32_t n = 300000;
      if (plan1(c, n, 0, knobs(-1), &b)) continue;  // out of range at this lis
      CHECK(!line_is_dense(b.plans[0].lg_line));
    }
  // the compaction chain: eight incremental rounds of 2^20 - 1 keys, values 0..7; the later
  // rounds' tables outgrow the L2, but an incremental round keeps the current format
  BatchPlan prev, seventh;
  for (uint32_t v = 0; v < 8; v++) {
    BatchPlan cur;
    const OldFilter o = v ? old_of(prev, cfg) : OldFilter();
    CHECK(plan1(cfg, (1u << 20) - 1, (uint16_t)v, knobs(-1), &cur, v ? &o : nullptr) == 0);
    CHECK(!line_is_dense(cur.plans[0].lg_line));
    if (v == 7) CHECK((uint64_t)cur.plans[0].num_indices * lines_per_index(8, cur.plans[0].lg_line) * 64 > LINE_DENSE_MIN_TABLE);
    check_lines(cur, cfg);
    if (v == 7) seventh = prev;
    prev = cur;
  }
  // forced on, the last round goes dense (the tests' incremental case)
  BatchPlan forced;
  const OldFilter o = old_of(seventh, cfg);
  CHECK(plan1(cfg, (1u << 20) - 1, 7, knobs(1), &forced, &o) == 0);
  CHECK(line_is_dense(forced.plans[0].lg_line));
  check_lines(forced, cfg);
}

int main(int argc, char** argv) {
  check_c2_goes_dense();
  check_the_gate_keeps_the_rest();
  for (int i = 1; i < argc; i++) {
    unsigned fp, lis, n, value;
    if (sscanf(argv[i], "%u:%u:%u:%u", &fp, &lis, &n, &value) != 4) return 2;
    BatchPlan f, d;
    const rf_amd_config cfg = config(fp, lis);
    CHECK(plan1(cfg, n, (uint16_t)value, knobs(1), &f) == 0);
    CHECK(plan1(cfg, n, (uint16_t)value, knobs(-1), &d) == 0);
    check_lines(f, cfg);
    printf("dense %u %u %u %u %u %u %llu\n", fp, lis, n, value, f.plans[0].lg_line, d.plans[0].lg_line,
           (unsigned long long)f.NL);
  }
  if (g_failed) {
    printf("dense_plan_check: %d checks FAILED\n", g_failed);
    return 1;
  }
  printf("dense_plan_check: OK\n");
  return 0;
}
