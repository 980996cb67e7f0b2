// set_kind_check -- member kinds in the planner of a filter set's member updates
// (splinterdb_amd/csrc/rf_set_plan.h) checked on the host: a slot holds a filter, NULL or an
// unfiltered member (RF_AMD_MEMBER_UNFILTERED, src/trunk.c:6020-6022); the last entry of a
// repeated id wins across kinds; unfiltered slots have no seed and take no part in the seed rule
// of the keys forms; they count for num_members; a refused call leaves the kinds as they were.
// Built (with the address and undefined-behaviour sanitizers) and run by
// tests/test_set_kind_plan.py; needs no device. Prints "set_kind_check: OK".
#include <stdio.h>

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
typedef std::vector<uint8_t> U8;
static const uint8_t F = SET_FILTER, N = SET_NULL, U = SET_UNFILTERED;

static int update(SetState* s, const U32& ids, const U32& seeds, const U8& kinds, SetUpdatePlan* plan,
                  std::string* err = nullptr) {
  return plan_set_update(s, (uint32_t)ids.size(), ids.data(), kinds.empty() ? nullptr : kinds.data(), seeds.data(),
                         plan, err);
}

static void check_kinds() {
  CHECK(F == 0 && N == 1 && U == 2);  // the values of the array that was is_null
  SetState s;
  s.init(8);
  SetUpdatePlan p;
  for (uint32_t g = 0; g < 8; g++) CHECK(s.kind[g] == N);  // a slot never set is a NULL member
  CHECK(update(&s, {0, 1, 2, 3}, {42, 9, 9, 42}, {F, U, N, F}, &p) == 0);
  CHECK((s.kind == U8{F, U, N, F, N, N, N, N}));
  CHECK(s.occupied[0] && !s.occupied[1] && !s.occupied[2] && s.occupied[3]);
  CHECK(s.slot_seed[1] == 0 && s.slot_seed[2] == 0);  // the seeds of the other kinds are not read
  CHECK((p.order == U32{0, 1, 2, 3}) && p.launches() == 1);
  // no kind array: every entry is a filter
  CHECK(update(&s, {1}, {42}, {}, &p) == 0);
  CHECK(s.kind[1] == F && s.occupied[1] && s.slot_seed[1] == 42);
}

static void check_last_entry_wins() {
  SetState s;
  s.init(8);
  SetUpdatePlan p;
  // id 3: filter, unfiltered, NULL, unfiltered; id 5: unfiltered, then filter; id 6: NULL, filter, NULL
  CHECK(update(&s, {3, 5, 3, 6, 3, 5, 6, 3, 6}, {1, 2, 3, 4, 5, 77, 7, 8, 9}, {F, U, U, N, N, F, F, U, N}, &p) == 0);
  CHECK((p.order == U32{5, 7, 8}));  // the last entry of 5, of 3, of 6, in the call's order
  CHECK(s.kind[3] == U && !s.occupied[3] && s.slot_seed[3] == 0);
  CHECK(s.kind[5] == F && s.occupied[5] && s.slot_seed[5] == 77);
  CHECK(s.kind[6] == N && !s.occupied[6]);
  CHECK(s.one_seed && s.seed == 77);
  // and the other way round in a later call
  CHECK(update(&s, {3, 5, 5}, {42, 0, 0}, {F, N, U}, &p) == 0);
  CHECK((p.order == U32{0, 2}));
  CHECK(s.kind[3] == F && s.slot_seed[3] == 42 && s.kind[5] == U && !s.occupied[5]);
  CHECK(s.one_seed && s.seed == 42);
}

static void check_seed_rule() {
  SetState s;
  s.init(8);
  SetUpdatePlan p;
  // filters with seed 7 plus unfiltered members keep one seed, whatever the entries' seed words say
  CHECK(update(&s, {0, 1, 2, 3}, {7, 1234, 7, 99}, {F, U, F, U}, &p) == 0);
  CHECK(s.one_seed && s.seed == 7);
  // an unfiltered member first in the table: the seed is the first filter's
  CHECK(update(&s, {0}, {55}, {U}, &p) == 0);
  CHECK(s.one_seed && s.seed == 7);
  // a filter with another seed breaks the rule; an unfiltered member in its place restores it
  CHECK(update(&s, {4}, {8}, {F}, &p) == 0);
  CHECK(!s.one_seed);
  CHECK(update(&s, {4}, {8}, {U}, &p) == 0);
  CHECK(s.one_seed && s.seed == 7);
  // replacing the last filter by an unfiltered member gives seed 0
  CHECK(update(&s, {2}, {7}, {U}, &p) == 0);
  CHECK(s.one_seed && s.seed == 0);
  for (uint32_t g = 0; g < 8; g++) CHECK(!s.occupied[g]);
  CHECK((s.kind == U8{U, U, U, U, U, N, N, N}));
  // a set of unfiltered members takes filters of any one seed afterwards
  CHECK(update(&s, {6}, {43}, {F}, &p) == 0);
  CHECK(s.one_seed && s.seed == 43);
}

static void check_num_members() {
  SetState s;
  s.init(16);
  SetUpdatePlan p;
  CHECK(update(&s, {0, 1}, {42, 0}, {F, U}, &p) == 0);
  CHECK(s.num_members == 2);
  CHECK(update(&s, {9}, {0}, {U}, &p) == 0);  // past the members: the count grows past it
  CHECK(s.num_members == 10 && s.kind[9] == U);
  for (uint32_t g = 2; g < 9; g++) CHECK(s.kind[g] == N);  // the gap: NULL members
  CHECK(update(&s, {9}, {0}, {N}, &p) == 0);  // cleared: a set does not shrink
  CHECK(s.num_members == 10 && s.kind[9] == N);
  CHECK(update(&s, {15}, {0}, {U}, &p) == 0);
  CHECK(s.num_members == 16);
}

static void check_refusal() {
  SetState s;
  s.init(8);
  SetUpdatePlan p;
  CHECK(update(&s, {0, 1, 5}, {42, 0, 42}, {F, U, F}, &p) == 0);
  const SetState before = s;
  const SetUpdatePlan plan_before = p;
  auto same = [&]() {
    return s.kind == before.kind && s.occupied == before.occupied && s.slot_seed == before.slot_seed &&
           s.num_members == before.num_members && s.seed == before.seed && s.one_seed == before.one_seed &&
           p.order == plan_before.order && p.cuts == plan_before.cuts;
  };
  std::string err;
  // the bad id last, so that every earlier entry has been looked at
  CHECK(update(&s, {1, 0, 8}, {42, 0, 0}, {F, U, U}, &p, &err) == RF_AMD_EINVAL);
  CHECK(!err.empty() && same());
  // a kind that does not exist, after entries that do
  err.clear();
  CHECK(update(&s, {1, 0, 6}, {42, 0, 0}, {F, U, 3}, &p, &err) == RF_AMD_EINVAL);
  CHECK(!err.empty() && same());
  CHECK(update(&s, {2}, {0}, {255}, &p) == RF_AMD_EINVAL);
  CHECK(same());
  // and the set still takes a legal call
  CHECK(update(&s, {1, 7}, {42, 0}, {F, U}, &p) == 0);
  CHECK(s.kind[1] == F && s.kind[7] == U && s.num_members == 8);
}

int main() {
  check_kinds();
  check_last_entry_wins();
  check_seed_rule();
  check_num_members();
  check_refusal();
  if (g_failed) {
    printf("set_kind_check: %d checks FAILED\n", g_failed);
    return 1;
  }
  printf("set_kind_check: OK\n");
  return 0;
}
