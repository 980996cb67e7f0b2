// range_plan_check -- the planner of a range map (splinterdb_amd/csrc/rf_range_plan.h) checked
// on the host: the refusals, R = 1 with NULL boundary arrays, list offsets rebased to 0, max_list,
// the packed image, the scratch size of a route call, and the search over the image
// (range_route_one: the steps of the routing kernel -- big-endian 8-byte prefixes, then the tie
// run by full compares) against a direct transcription of the reference's find_pivot loop
// (src/trunk.c:5892-5928, less_than_or_equal, pivot 0 = -infinity) on random tables. Built (with
// the address and undefined-behaviour sanitizers) and run by tests/test_range_plan.py; needs no
// device. Prints "range_plan_check: OK".
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "rf_range_plan.h"

using namespace rf;

static int g_failed = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      g_failed++;                                             \
    }                                                         \
  } while (0)

typedef std::vector<uint8_t> Key;

// a table in the caller's form
struct Table {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> boff, loff;
  std::vector<uint32_t> list;
  uint32_t R = 0;
};

static Table make_table(const std::vector<Key>& bounds, const std::vector<std::vector<uint32_t>>& lists,
                        uint64_t boff0 = 0, uint64_t loff0 = 0) {
  Table t;
  t.R = (uint32_t)lists.size();
  t.bytes.assign(boff0, 0xEE);
  t.boff.push_back(boff0);
  for (const Key& b : bounds) {
    t.bytes.insert(t.bytes.end(), b.begin(), b.end());
    t.boff.push_back(t.bytes.size());
  }
  t.bytes.push_back(0xEE);
  t.list.assign(loff0, 0xEEEEEEEEu);
  t.loff.push_back(loff0);
  for (const auto& l : lists) {
    t.list.insert(t.list.end(), l.begin(), l.end());
    t.loff.push_back(t.list.size());
  }
  t.list.push_back(0xEEEEEEEEu);
  return t;
}

static int plan_of(const Table& t, RangePlan* p, std::string* err = nullptr) {
  return plan_range_map(t.R, t.bytes.data(), t.boff.data(), t.list.data(), t.loff.data(), p, err);
}

static Key K(const char* s) { return Key(s, s + strlen(s)); }

static void check_refusals() {
  RangePlan p;
  p.num_ranges = 77;  // a refused call leaves the plan as it was
  std::string err;
  const std::vector<std::vector<uint32_t>> l3 = {{1}, {2}, {3}};
  Table ok = make_table({K("a"), K("b")}, l3);
  CHECK(plan_of(ok, &p) == 0 && p.num_ranges == 3);
  p.num_ranges = 77;
  CHECK(plan_range_map(0, ok.bytes.data(), ok.boff.data(), ok.list.data(), ok.loff.data(), &p, &err) ==
        RF_AMD_EINVAL);
  CHECK(err.find("num_ranges") != std::string::npos);
  CHECK(plan_range_map(3, ok.bytes.data(), ok.boff.data(), ok.list.data(), nullptr, &p, &err) == RF_AMD_EINVAL);
  CHECK(plan_range_map(3, ok.bytes.data(), nullptr, ok.list.data(), ok.loff.data(), &p, &err) == RF_AMD_EINVAL);
  CHECK(plan_range_map(3, nullptr, ok.boff.data(), ok.list.data(), ok.loff.data(), &p, &err) == RF_AMD_EINVAL);
  CHECK(plan_range_map(3, ok.bytes.data(), ok.boff.data(), nullptr, ok.loff.data(), &p, &err) == RF_AMD_EINVAL);
  CHECK(plan_range_map(3, ok.bytes.data(), ok.boff.data(), ok.list.data(), ok.loff.data(), nullptr, &err) ==
        RF_AMD_EINVAL);
  {  // boundary offsets decreasing
    Table t = ok;
    t.boff[1] = 2, t.boff[2] = 1;
    CHECK(plan_of(t, &p, &err) == RF_AMD_EINVAL && err.find("boundary offsets") != std::string::npos);
  }
  {  // not strictly ascending: descending, equal, equal empty keys, a prefix after its extension
    CHECK(plan_of(make_table({K("b"), K("a")}, l3), &p, &err) == RF_AMD_EINVAL);
    CHECK(err.find("ascending") != std::string::npos);
    CHECK(plan_of(make_table({K("a"), K("a")}, l3), &p) == RF_AMD_EINVAL);
    CHECK(plan_of(make_table({K(""), K("")}, l3), &p) == RF_AMD_EINVAL);
    CHECK(plan_of(make_table({K("ab"), K("a")}, l3), &p) == RF_AMD_EINVAL);
    CHECK(plan_of(make_table({Key{0x80}, Key{0x7f}}, l3), &p) == RF_AMD_EINVAL);
    // and the legal neighbours of those: unsigned bytes, the shorter first, a trailing zero byte
    CHECK(plan_of(make_table({Key{0x7f}, Key{0x80}}, l3), &p) == 0);
    CHECK(plan_of(make_table({K("a"), K("ab")}, l3), &p) == 0);
    CHECK(plan_of(make_table({K("ab"), Key{'a', 'b', 0}}, l3), &p) == 0);
    CHECK(plan_of(make_table({K(""), Key{0}}, l3), &p) == 0);
    p.num_ranges = 77;
  }
  {  // list offsets decreasing
    Table t = ok;
    t.loff[2] = 0;
    CHECK(plan_of(t, &p, &err) == RF_AMD_EINVAL && err.find("list offsets") != std::string::npos);
  }
  {  // a list of 65,536 ids; 65,535 is legal
    std::vector<std::vector<uint32_t>> l = {{}, std::vector<uint32_t>(65536, 7u)};
    CHECK(plan_of(make_table({K("m")}, l), &p, &err) == RF_AMD_EINVAL && err.find("65,535") != std::string::npos);
    CHECK(p.num_ranges == 77);
    l[1].pop_back();
    CHECK(plan_of(make_table({K("m")}, l), &p) == 0 && p.max_list == 65535 && p.num_ranges == 2);
  }
}

static void check_layout() {
  RangePlan p;
  // R = 1: no boundary, NULL boundary arrays
  const uint32_t ids[] = {9, 8, 7};
  const uint64_t loff1[] = {0, 3};
  CHECK(plan_range_map(1, nullptr, nullptr, ids, loff1, &p, nullptr) == 0);
  CHECK(p.num_ranges == 1 && p.max_list == 3);
  const uint8_t key[] = {0xff, 0xff};
  CHECK(range_route_one(p, key, 2) == 0 && range_route_one(p, key, 0) == 0);
  const uint64_t loff0[] = {5, 5};  // an empty list, NULL ids
  CHECK(plan_range_map(1, nullptr, nullptr, nullptr, loff0, &p, nullptr) == 0 && p.max_list == 0);
  // offsets that do not start at 0 are rebased; the image holds exactly the caller's table
  const std::vector<Key> bounds = {K(""), K("ab"), Key{'a', 'b', 0}, Key{'a', 'b', 0, 0}, K("abcdefghi"), Key{0xff}};
  const std::vector<std::vector<uint32_t>> lists = {{}, {1, 2}, {}, {3}, {4, 5, 6, 7, 8}, {}, {9}};
  Table t = make_table(bounds, lists, 11, 1000);
  CHECK(plan_of(t, &p) == 0);
  CHECK(p.num_ranges == 7 && p.max_list == 5);
  const uint64_t* prefix = reinterpret_cast<const uint64_t*>(p.image.data() + p.o_prefix);
  const uint64_t* boff = reinterpret_cast<const uint64_t*>(p.image.data() + p.o_boff);
  const uint64_t* loff = reinterpret_cast<const uint64_t*>(p.image.data() + p.o_loff);
  const uint32_t* list = reinterpret_cast<const uint32_t*>(p.image.data() + p.o_list);
  CHECK(boff[0] == 0 && loff[0] == 0 && loff[7] == 9);
  CHECK(p.o_boff % 8 == 0 && p.o_loff % 8 == 0 && p.o_list % 8 == 0 && p.o_bytes % 8 == 0);
  CHECK(p.o_bytes + boff[6] <= p.image.size());
  uint32_t at = 0;
  for (size_t r = 0; r < lists.size(); r++) {
    CHECK(loff[r + 1] - loff[r] == lists[r].size());
    for (uint32_t id : lists[r]) CHECK(list[at++] == id);
  }
  for (size_t j = 0; j < bounds.size(); j++) {
    CHECK(boff[j + 1] - boff[j] == bounds[j].size());
    if (!bounds[j].empty())
      CHECK(memcmp(p.image.data() + p.o_bytes + boff[j], bounds[j].data(), bounds[j].size()) == 0);
    CHECK(prefix[j] == range_prefix(bounds[j].data(), bounds[j].size()));
    if (j) CHECK(prefix[j - 1] <= prefix[j]);
  }
  CHECK(prefix[0] == 0 && prefix[1] == 0x6162000000000000ull && prefix[2] == prefix[1] && prefix[3] == prefix[1]);
  CHECK(prefix[4] == 0x6162636465666768ull && prefix[5] == 0xff00000000000000ull);
  // keys at, between and around the zero-padded ties
  auto route = [&](const Key& k) { return range_route_one(p, k.data(), k.size()); };
  CHECK(route(K("")) == 1 && route(Key{0}) == 1 && route(K("a")) == 1 && route(K("ab")) == 2);
  CHECK(route(Key{'a', 'b', 0}) == 3 && route(Key{'a', 'b', 0, 0}) == 4 && route(Key{'a', 'b', 0, 0, 0}) == 4);
  CHECK(route(Key{'a', 'b', 0, 1}) == 4 && route(K("abcdefgh")) == 4 && route(K("abcdefghi")) == 5);
  CHECK(route(K("abcdefghh")) == 4 && route(Key{0xfe}) == 5 && route(Key{0xff}) == 6 && route(Key{0xff, 0}) == 6);
}

static void check_scratch() {
  CHECK(range_route_scratch_bytes(0) >= 16);
  uint64_t last = 0;
  const uint64_t ns[] = {0, 1, 1023, 1024, 1025, 2381, 4096, 1u << 20, (1u << 24) + 1, 1ull << 40, (1ull << 56) - 1};
  for (uint64_t n : ns) {
    const uint64_t s = range_route_scratch_bytes(n), tiles = range_route_tiles(n);
    CHECK(s >= last && s % 8 == 0);
    CHECK(tiles * RANGE_TILE >= n && (tiles == 0 || (tiles - 1) * RANGE_TILE < n));
    CHECK(s >= 12 * tiles);  // 8 bytes of offset and 4 of count per tile
    last = s;
  }
  for (uint64_t n = 0; n < 5000; n++) CHECK(range_route_scratch_bytes(n + 1) >= range_route_scratch_bytes(n));
}

// trunk_ondisk_node_find_pivot's loop with less_than_or_equal: pivot 0 is the node's lower bound
// (-infinity here), pivots 1.. are the boundaries; the last pivot whose key is <= the key
static uint32_t find_pivot(const std::vector<Key>& bounds, const Key& k) {
  uint32_t lo = 0, hi = (uint32_t)bounds.size() + 1;  // pivots [lo, hi)
  while (lo + 1 < hi) {
    const uint32_t mid = (lo + hi) / 2;  // mid >= 1: boundary mid - 1
    const Key& b = bounds[mid - 1];
    const size_t m = std::min(b.size(), k.size());
    int c = m ? memcmp(k.data(), b.data(), m) : 0;  // slice_lex_cmp(key, pivot)
    if (c == 0) c = k.size() < b.size() ? -1 : k.size() > b.size() ? 1 : 0;
    if (c < 0) hi = mid;
    else lo = mid;
  }
  return lo;
}

static void check_random_tables() {
  std::mt19937_64 rng(20260101);
  const uint8_t alphabet[] = {0x00, 0x61, 0x7f, 0x80, 0xff};
  const uint32_t lens[] = {0, 1, 2, 7, 8, 9, 10, 16, 17, 40};
  auto rand_key = [&](uint32_t len, uint32_t nsym) {
    Key k(len);
    for (auto& b : k) b = alphabet[rng() % nsym];
    return k;
  };
  uint64_t cases = 0, ties = 0, equal = 0;
  for (int table = 0; table < 200; table++) {
    // few symbols: long common prefixes and many boundaries with the same 8-byte prefix
    const uint32_t nsym = table % 3 == 0 ? 2 : 5;
    std::vector<Key> bounds;
    const uint32_t want = 1 + (uint32_t)(rng() % 200);
    for (uint32_t j = 0; j < want; j++) bounds.push_back(rand_key(lens[rng() % 10], nsym));
    std::sort(bounds.begin(), bounds.end());  // vector<uint8_t> order is slice_lex_cmp's
    bounds.erase(std::unique(bounds.begin(), bounds.end()), bounds.end());
    std::vector<std::vector<uint32_t>> lists(bounds.size() + 1);
    for (auto& l : lists) l.assign(rng() % 4, (uint32_t)(rng() % 100));
    RangePlan p;
    CHECK(plan_of(make_table(bounds, lists, rng() % 9, rng() % 9), &p) == 0);
    for (int q = 0; q < 900; q++) {
      Key k;
      const uint32_t how = (uint32_t)(rng() % 10);
      const Key& b = bounds[rng() % bounds.size()];
      if (how < 3) k = b;  // equal to a boundary: the range to its right
      else if (how == 3) k = Key(b.begin(), b.begin() + (b.empty() ? 0 : rng() % b.size()));  // a proper prefix
      else if (how == 4) { k = b; k.push_back(alphabet[rng() % 5]); }                          // a byte appended
      else k = rand_key(lens[rng() % 10], nsym);
      const uint32_t got = range_route_one(p, k.data(), k.size()), ref = find_pivot(bounds, k);
      if (got != ref) {
        printf("table %d key of %zu bytes: range %u, find_pivot %u\n", table, k.size(), got, ref);
        g_failed++;
      }
      cases++;
      equal += how < 3;
      // how often the prefix alone did not decide
      const uint64_t kp = range_prefix(k.data(), k.size());
      for (const Key& x : bounds)
        if (range_prefix(x.data(), x.size()) == kp) {
          ties++;
          break;
        }
    }
  }
  CHECK(cases == 180000 && ties > cases / 10 && equal > cases / 5);
  printf("random tables: %llu cases, %llu with a boundary of the key's prefix\n", (unsigned long long)cases,
         (unsigned long long)ties);
}

int main() {
  check_refusals();
  check_layout();
  check_scratch();
  check_random_tables();
  if (g_failed) {
    printf("range_plan_check: %d FAILED\n", g_failed);
    return 1;
  }
  printf("range_plan_check: OK\n");
  return 0;
}
