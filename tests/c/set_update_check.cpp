// set_update_check -- the planner of a filter set's member updates
// (splinterdb_amd/csrc/rf_set_plan.h) checked on the host: which entry of a repeated id wins,
// the cuts into launches, the member count, a refused call leaving everything as it was, and the
// seed rule of the keys forms as members come and go. Built (with the address and
// undefined-behaviour sanitizers) and run by tests/test_set_update_plan.py; needs no device.
// Prints "set_update_check: OK".
#include <stdio.h>

#include <set>
#include <string>
#include <vector>

#include "rf_set_plan.h"

using namespace rf;

static int g_failed = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      g_failed++;                                             \
    }                                                         \
  } while (0)

typedef std::vector<uint32_t> U32;

// entry i: id ids[i], seed seeds[i]; null[i] (empty: none) clears the slot
static int update(SetState* s, const U32& ids, const U32& seeds, const std::vector<uint8_t>& null,
                  SetUpdatePlan* plan, std::string* err = nullptr) {
  return plan_set_update(s, (uint32_t)ids.size(), ids.data(), null.empty() ? nullptr : null.data(), seeds.data(),
                         plan, err);
}

static bool same_state(const SetState& a, const SetState& b) {
  return a.capacity == b.capacity && a.num_members == b.num_members && a.seed == b.seed &&
         a.one_seed == b.one_seed && a.slot_seed == b.slot_seed && a.occupied == b.occupied;
}

static void check_dedup() {
  SetState s;
  s.init(8);
  SetUpdatePlan p;
  // the entries' seeds tell them apart: entry i carries seed 100 + i
  const U32 ids = {3, 5, 3, 3, 7, 5}, seeds = {100, 101, 102, 103, 104, 105};
  CHECK(update(&s, ids, seeds, {}, &p) == 0);
  CHECK((p.order == U32{3, 4, 5}));  // the last entry of 3, of 7, of 5, in the call's order
  CHECK((p.cuts == U32{0, 3}));
  CHECK(s.slot_seed[3] == 103 && s.slot_seed[7] == 104 && s.slot_seed[5] == 105);
  CHECK(s.occupied[3] && s.occupied[5] && s.occupied[7]);
  for (uint32_t g : {0u, 1u, 2u, 4u, 6u}) CHECK(!s.occupied[g]);
  CHECK(s.num_members == 8);
  CHECK(!s.one_seed && s.seed == 103);
  // a cleared slot wins over an earlier filter of the same id, and the other way round
  CHECK(update(&s, {3, 3, 5, 5}, {7, 0, 0, 9}, {0, 1, 1, 0}, &p) == 0);
  CHECK((p.order == U32{1, 3}));
  CHECK(!s.occupied[3] && s.occupied[5] && s.slot_seed[5] == 9);
}

static void check_cuts() {
  for (uint32_t count : {0u, 1u, 63u, 64u, 65u, 128u, 129u, 1000u}) {
    // with repeats: entry i names id (i * 7) % m, so ids recur once count > m
    for (uint32_t m : {2000u, 90u}) {
      SetState s;
      s.init(2000);
      SetUpdatePlan p;
      U32 ids(count), seeds(count, 42);
      for (uint32_t i = 0; i < count; i++) ids[i] = (i * 7) % m;
      CHECK(update(&s, ids, seeds, {}, &p) == 0);
      // the deduplicated list by the rule itself: entry i stays when no later entry names its id
      U32 want;
      for (uint32_t i = 0; i < count; i++) {
        bool later = false;
        for (uint32_t j = i + 1; j < count; j++) later |= ids[j] == ids[i];
        if (!later) want.push_back(i);
      }
      CHECK(p.order == want);
      const uint32_t kept = (uint32_t)want.size();
      CHECK(p.launches() == (kept + SET_UPD_PER_LAUNCH - 1) / SET_UPD_PER_LAUNCH);
      CHECK(!p.cuts.empty() && p.cuts.front() == 0 && p.cuts.back() == kept);
      U32 joined;
      for (uint32_t l = 0; l < p.launches(); l++) {
        CHECK(p.cuts[l] < p.cuts[l + 1]);
        CHECK(p.cuts[l + 1] - p.cuts[l] <= SET_UPD_PER_LAUNCH);
        std::set<uint32_t> in_launch;
        for (uint32_t k = p.cuts[l]; k < p.cuts[l + 1]; k++) {
          CHECK(in_launch.insert(ids[p.order[k]]).second);
          joined.push_back(p.order[k]);
        }
      }
      CHECK(joined == want);
      if (count == 0) CHECK(p.launches() == 0 && s.num_members == 0);
    }
  }
}

static void check_num_members() {
  SetState s;
  s.init(16);
  SetUpdatePlan p;
  CHECK(update(&s, {0, 1, 2, 3}, {42, 42, 42, 42}, {0, 0, 1, 0}, &p) == 0);
  CHECK(s.num_members == 4 && s.capacity == 16);
  CHECK(update(&s, {9}, {42}, {}, &p) == 0);
  CHECK(s.num_members == 10);
  CHECK(update(&s, {2}, {42}, {}, &p) == 0);
  CHECK(s.num_members == 10);
  CHECK(update(&s, {15}, {0}, {1}, &p) == 0);  // a cleared slot counts as named
  CHECK(s.num_members == 16);
  CHECK(update(&s, {}, {}, {}, &p) == 0);
  CHECK(s.num_members == 16 && p.launches() == 0);
}

static void check_refusal() {
  SetState s;
  s.init(16);
  SetUpdatePlan p;
  CHECK(update(&s, {0, 1, 5}, {42, 42, 43}, {}, &p) == 0);
  const SetState before = s;
  const SetUpdatePlan plan_before = p;
  std::string err;
  // the bad id last, so that every earlier entry has been looked at
  CHECK(update(&s, {2, 0, 16}, {42, 7, 42}, {0, 1, 0}, &p, &err) == RF_AMD_EINVAL);
  CHECK(!err.empty());
  CHECK(same_state(s, before));
  CHECK(p.order == plan_before.order && p.cuts == plan_before.cuts);
  CHECK(update(&s, {0xFFFFFFFFu}, {42}, {}, &p) == RF_AMD_EINVAL);
  CHECK(same_state(s, before));
  CHECK(plan_set_update(&s, 2, nullptr, nullptr, nullptr, &p, &err) == RF_AMD_EINVAL);
  CHECK(same_state(s, before));
  // and the set still takes a legal call
  CHECK(update(&s, {15}, {42}, {}, &p) == 0);
  CHECK(s.num_members == 16 && s.occupied[15]);
}

static void check_seed_state() {
  SetState s;
  s.init(8);
  SetUpdatePlan p;
  CHECK(s.one_seed && s.seed == 0);  // no member: the keys forms are legal and find nothing
  CHECK(update(&s, {2}, {42}, {}, &p) == 0);  // the first member
  CHECK(s.one_seed && s.seed == 42);
  CHECK(update(&s, {5}, {42}, {}, &p) == 0);  // a second with the same seed
  CHECK(s.one_seed && s.seed == 42);
  CHECK(update(&s, {3}, {43}, {}, &p) == 0);  // a different seed
  CHECK(!s.one_seed);
  CHECK(update(&s, {3}, {42}, {}, &p) == 0);  // the different one replaced
  CHECK(s.one_seed && s.seed == 42);
  CHECK(update(&s, {3}, {43}, {}, &p) == 0);
  CHECK(!s.one_seed);
  CHECK(update(&s, {3}, {0}, {1}, &p) == 0);  // ... or cleared
  CHECK(s.one_seed && s.seed == 42);
  CHECK(update(&s, {2, 5}, {43, 43}, {}, &p) == 0);  // every member moves to another seed
  CHECK(s.one_seed && s.seed == 43);
  CHECK(update(&s, {2, 5}, {0, 0}, {1, 1}, &p) == 0);  // every member cleared
  CHECK(s.one_seed && s.seed == 0);
  for (uint32_t g = 0; g < 8; g++) CHECK(!s.occupied[g]);
  CHECK(s.num_members == 6);  // a set does not shrink
}

int main() {
  check_dedup();
  check_cuts();
  check_num_members();
  check_refusal();
  check_seed_state();
  if (g_failed) {
    printf("set_update_check: %d checks FAILED\n", g_failed);
    return 1;
  }
  printf("set_update_check: OK\n");
  return 0;
}
