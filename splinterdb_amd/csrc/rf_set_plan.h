// rf_set_plan.h -- host-only planning of a filter set's member updates: everything
// rf_amd_filter_set_update (and rf_amd_filter_set_create_cap, which is an update of an empty
// set) decides before its first launch -- whether the call is legal, which entry of a repeated
// id wins, how the surviving entries are cut into launches, the member count afterwards and the
// seed rule of the keys forms. Plain C++: no HIP calls, no allocation on the device, no engine
// types -- tests/c/set_update_check.cpp checks it without a GPU. plan_set_update returns 0 or
// the RF_AMD_E* code, with the message in *err; a refused call changes nothing.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rf_amd.h"
#include "rf_plan.h"

namespace rf {

// what an entry puts into a slot: a filter, NULL_ROUTING_FILTER (a bundle with no branch), or
// RF_AMD_MEMBER_UNFILTERED (a bundle without a maplet that holds one branch)
enum SetMemberKind : uint8_t { SET_FILTER = 0, SET_NULL = 1, SET_UNFILTERED = 2 };

// what the host keeps of a set: its size, the members' count (one past the largest id ever
// set), each slot's seed, whether a filter sits in it and its kind, and the seed rule these give
// -- `seed` is the seed of the first occupied slot (0: none), one_seed whether every occupied
// slot has it. Only a filter occupies a slot: an unfiltered member hashes nothing.
struct SetState {
  uint32_t capacity = 0, num_members = 0;
  uint32_t seed = 0;
  bool one_seed = true;
  std::vector<uint32_t> slot_seed;  // capacity
  std::vector<uint8_t> occupied;    // capacity
  std::vector<uint8_t> kind;        // capacity: SetMemberKind (a slot never set: SET_NULL)
  // scratch of the deduplication: mark[id] == gen, entry of id seen in this call
  std::vector<uint32_t> mark;
  uint32_t gen = 0;
  void init(uint32_t cap) {
    *this = SetState();
    capacity = cap;
    slot_seed.assign(cap, 0u);
    occupied.assign(cap, 0);
    kind.assign(cap, SET_NULL);
    mark.assign(cap, 0u);
  }
};

// the entries that go out: order[k] is the position, in the call's arrays, of the k-th entry
// launched (the last entry of every id, in the call's order); launch l takes
// order[cuts[l] .. cuts[l + 1]), at most SET_UPD_PER_LAUNCH of them
struct SetUpdatePlan {
  std::vector<uint32_t> order;
  std::vector<uint32_t> cuts;  // launches + 1 (a call without entries: {0})
  uint32_t launches() const { return cuts.empty() ? 0u : (uint32_t)cuts.size() - 1; }
};

// the call: entry i sets member ids[i] to what kind[i] names (SetMemberKind; kind == nullptr:
// every entry is a filter): a filter hashed with seeds[i], NULL_ROUTING_FILTER or an unfiltered
// member (seeds[i] is not read for these two); any other value is refused
inline int plan_set_update(SetState* s, uint32_t count, const uint32_t* ids, const uint8_t* kind,
                           const uint32_t* seeds, SetUpdatePlan* plan, std::string* err) {
  auto refuse = [&](const char* m) {
    if (err) *err = m;
    return RF_AMD_EINVAL;
  };
  if (!s || !plan) return refuse("null set state");
  if (count && (!ids || !seeds)) return refuse("null member arrays");
  for (uint32_t i = 0; i < count; i++)
    if (ids[i] >= s->capacity) return refuse("member id >= capacity");
  for (uint32_t i = 0; kind && i < count; i++)
    if (kind[i] > SET_UNFILTERED) return refuse("unknown member kind");
  // nothing above has written anything; nothing below fails
  if (++s->gen == 0) {  // the counter wrapped: stale marks could match again
    s->mark.assign(s->capacity, 0u);
    s->gen = 1;
  }
  plan->order.clear();
  plan->cuts.clear();
  plan->order.resize(count);
  uint32_t kept = 0, top = s->num_members;
  for (uint32_t i = count; i-- > 0;) {  // backwards: the first entry met of an id is its last
    const uint32_t id = ids[i];
    if (s->mark[id] == s->gen) continue;
    s->mark[id] = s->gen;
    plan->order[count - ++kept] = i;
    const uint8_t k = kind ? kind[i] : (uint8_t)SET_FILTER;
    s->kind[id] = k;
    s->occupied[id] = k == SET_FILTER ? 1 : 0;
    s->slot_seed[id] = k == SET_FILTER ? seeds[i] : 0u;
    if (id + 1 > top) top = id + 1;
  }
  plan->order.erase(plan->order.begin(), plan->order.begin() + (count - kept));
  for (uint32_t at = 0; at < kept; at += SET_UPD_PER_LAUNCH) plan->cuts.push_back(at);
  plan->cuts.push_back(kept);
  s->num_members = top;
  s->seed = 0;
  s->one_seed = true;
  bool any = false;
  for (uint32_t g = 0; g < s->capacity; g++) {
    if (!s->occupied[g]) continue;
    if (!any) s->seed = s->slot_seed[g];
    else if (s->slot_seed[g] != s->seed) s->one_seed = false;
    any = true;
  }
  return 0;
}

}  // namespace rf
