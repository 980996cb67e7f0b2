// range_seg_check -- the planner of a range map made from segments
// (splinterdb_amd/csrc/rf_range_seg_plan.h) checked on the host: every refusal of
// plan_range_map_segments and plan_range_seg_update, and that a refused call wrote nothing; the
// legal edge cases; max_list = the largest path capacity; the host flatten against a naive
// concatenation on random tables; random sequences of updates applied to the plan's image
// (the launches' arguments scattered by the kernel's host mirror, then the flatten) against the
// naive model after every step; and the cut of an update into launches and pieces. Built (with
// the address and undefined-behaviour sanitizers) and run by tests/test_range_seg_plan.py; needs
// no device. Prints "range_seg_check: OK".
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "rf_range_seg_plan.h"

using namespace rf;

static int g_failed = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      g_failed++;                                             \
    }                                                         \
  } while (0)

typedef std::vector<uint32_t> Ids;

// a segmented table in the caller's form; boundaries are the 2-byte big-endian numbers 1..R-1
struct Table {
  uint32_t R = 0, S = 0;
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> boff, poff, soff;
  std::vector<uint32_t> path, cap, ids;
};

static Table make_table(const std::vector<Ids>& paths, const std::vector<Ids>& lists, const Ids& caps,
                        uint64_t poff0 = 0, uint64_t soff0 = 0) {
  Table t;
  t.R = (uint32_t)paths.size();
  t.S = (uint32_t)lists.size();
  t.boff.push_back(0);
  for (uint32_t j = 1; j < t.R; j++) {
    t.bytes.push_back((uint8_t)(j >> 8));
    t.bytes.push_back((uint8_t)j);
    t.boff.push_back(t.bytes.size());
  }
  t.bytes.push_back(0xEE);
  t.path.assign(poff0, 0xEEEEEEEEu);
  t.poff.push_back(poff0);
  for (const Ids& p : paths) {
    t.path.insert(t.path.end(), p.begin(), p.end());
    t.poff.push_back(t.path.size());
  }
  t.path.push_back(0xEEEEEEEEu);
  t.ids.assign(soff0, 0xEEEEEEEEu);
  t.soff.push_back(soff0);
  for (const Ids& l : lists) {
    t.ids.insert(t.ids.end(), l.begin(), l.end());
    t.soff.push_back(t.ids.size());
  }
  t.ids.push_back(0xEEEEEEEEu);
  t.cap = caps;
  t.cap.push_back(0);
  return t;
}

static int plan_of(const Table& t, RangeSegPlan* p, std::string* err = nullptr) {
  return plan_range_map_segments(t.R, t.bytes.data(), t.boff.data(), t.path.data(), t.poff.data(), t.S,
                                 t.cap.data(), t.ids.data(), t.soff.data(), p, err);
}

// the naive model: range r's list is the concatenation of its path's lists
static std::vector<Ids> naive(const std::vector<Ids>& paths, const std::vector<Ids>& lists) {
  std::vector<Ids> out;
  for (const Ids& p : paths) {
    Ids l;
    for (uint32_t s : p) l.insert(l.end(), lists[s].begin(), lists[s].end());
    out.push_back(l);
  }
  return out;
}

// the plan's flat table equals `want`, and the segment sections hold `lists`
static bool image_equals(RangeSegPlan& p, const std::vector<Ids>& want, const std::vector<Ids>& lists) {
  const RangeSegDev d = range_seg_dev(p, p.image.data());
  bool ok = d.loff[0] == 0;
  for (size_t r = 0; r < want.size() && ok; r++) {
    ok = d.loff[r + 1] - d.loff[r] == want[r].size() && d.loff[r + 1] <= p.list_cap;
    for (size_t i = 0; i < want[r].size() && ok; i++) ok = d.list[d.loff[r] + i] == want[r][i];
  }
  for (size_t s = 0; s < lists.size() && ok; s++) {
    ok = d.slen[s] == lists[s].size() && d.slen[s] <= d.scap[s];
    for (size_t i = 0; i < lists[s].size() && ok; i++) ok = d.slots[d.sbase[s] + i] == lists[s][i];
  }
  return ok;
}

static void check_refusals() {
  RangeSegPlan p;
  p.num_ranges = 77;  // a refused call leaves the plan as it was
  std::string err;
  const std::vector<Ids> paths = {{0, 1}, {0, 2}, {0}}, lists = {{1, 2}, {3}, {}};
  const Ids caps = {4, 1, 2};
  const Table ok = make_table(paths, lists, caps);
  CHECK(plan_of(ok, &p) == 0 && p.num_ranges == 3 && p.num_segments == 3 && p.max_list == 6);
  p = RangeSegPlan();
  p.num_ranges = 77;
  auto refused = [&](const Table& t, const char* word) {
    err.clear();
    const bool r = plan_of(t, &p, &err) == RF_AMD_EINVAL && err.find(word) != std::string::npos &&
                   p.num_ranges == 77 && p.image.empty();
    if (!r) printf("  expected a refusal with '%s', message '%s'\n", word, err.c_str());
    return r;
  };
#define ARGS(t) \
  t.R, t.bytes.data(), t.boff.data(), t.path.data(), t.poff.data(), t.S, t.cap.data(), t.ids.data(), t.soff.data()
  CHECK(plan_range_map_segments(ARGS(ok), nullptr, &err) == RF_AMD_EINVAL);
  {
    Table t = ok;
    t.R = 0;
    CHECK(refused(t, "num_ranges"));
  }
  // NULL arrays where they are needed
  CHECK(plan_range_map_segments(3, ok.bytes.data(), ok.boff.data(), ok.path.data(), nullptr, 3, ok.cap.data(),
                                ok.ids.data(), ok.soff.data(), &p, &err) == RF_AMD_EINVAL);
  CHECK(plan_range_map_segments(3, ok.bytes.data(), ok.boff.data(), nullptr, ok.poff.data(), 3, ok.cap.data(),
                                ok.ids.data(), ok.soff.data(), &p, &err) == RF_AMD_EINVAL);
  CHECK(plan_range_map_segments(3, ok.bytes.data(), ok.boff.data(), ok.path.data(), ok.poff.data(), 3, nullptr,
                                ok.ids.data(), ok.soff.data(), &p, &err) == RF_AMD_EINVAL);
  CHECK(plan_range_map_segments(3, ok.bytes.data(), ok.boff.data(), ok.path.data(), ok.poff.data(), 3, ok.cap.data(),
                                nullptr, ok.soff.data(), &p, &err) == RF_AMD_EINVAL);
  CHECK(plan_range_map_segments(3, ok.bytes.data(), ok.boff.data(), ok.path.data(), ok.poff.data(), 3, ok.cap.data(),
                                ok.ids.data(), nullptr, &p, &err) == RF_AMD_EINVAL);
  CHECK(plan_range_map_segments(3, ok.bytes.data(), nullptr, ok.path.data(), ok.poff.data(), 3, ok.cap.data(),
                                ok.ids.data(), ok.soff.data(), &p, &err) == RF_AMD_EINVAL);
  CHECK(plan_range_map_segments(3, nullptr, ok.boff.data(), ok.path.data(), ok.poff.data(), 3, ok.cap.data(),
                                ok.ids.data(), ok.soff.data(), &p, &err) == RF_AMD_EINVAL);
  CHECK(p.num_ranges == 77 && p.image.empty());
  {  // what the flat create refuses about boundaries
    Table t = ok;
    t.boff[1] = 3, t.boff[2] = 2;
    CHECK(refused(t, "boundary offsets"));
    t = ok;
    t.bytes[1] = 2, t.bytes[3] = 1;
    CHECK(refused(t, "ascending"));
    t = ok;
    t.bytes[3] = t.bytes[1];
    CHECK(refused(t, "ascending"));
  }
  {
    Table t = ok;
    t.poff[1] = 3, t.poff[2] = 2;
    CHECK(refused(t, "path offsets"));
    t = ok;
    t.soff[1] = 1, t.soff[2] = 0;
    CHECK(refused(t, "segment offsets"));
    t = ok;
    t.path[3] = 3;
    CHECK(refused(t, "path entry"));
    t = ok;
    t.cap[1] = 0;  // an initial list of one id
    CHECK(refused(t, "longer than its capacity"));
  }
  {  // a path's capacities: 65,535 is legal, 65,536 is not, whatever the lengths are
    Table t = make_table({{0, 1}, {1}}, {{7}, {}}, {65000, 535});
    CHECK(plan_of(t, &p) == 0 && p.max_list == 65535 && p.list_cap == 65535 + 535);
    p = RangeSegPlan();
    p.num_ranges = 77;
    t.cap[1] = 536;
    CHECK(refused(t, "65,535"));
    t = make_table({{0, 0}}, {{}}, {32768});  // a segment twice in one path counts twice
    CHECK(refused(t, "65,535"));
  }
}

static void check_legal_edges() {
  RangeSegPlan p;
  // no segments at all: every path empty, NULL segment arrays and NULL paths
  const uint64_t poff[] = {4, 4, 4};
  const uint8_t b[] = {'m'};
  const uint64_t boff[] = {0, 1};
  CHECK(plan_range_map_segments(2, b, boff, nullptr, poff, 0, nullptr, nullptr, nullptr, &p, nullptr) == 0);
  CHECK(p.num_segments == 0 && p.max_list == 0 && p.list_cap == 0 && image_equals(p, {{}, {}}, {}));
  // R = 1 with NULL boundary arrays; an empty path; cap == 0; a segment in no path; a segment
  // twice in a path; offsets that do not start at 0
  CHECK(plan_range_map_segments(1, nullptr, nullptr, nullptr, poff, 0, nullptr, nullptr, nullptr, &p, nullptr) == 0);
  const std::vector<Ids> paths = {{}, {0, 1, 0}, {2, 1}, {1}}, lists = {{5, 6}, {}, {9}, {1, 2, 3}};
  const Ids caps = {2, 0, 4, 3};
  Table t = make_table(paths, lists, caps, 7, 3);
  CHECK(plan_of(t, &p) == 0);
  CHECK(p.max_list == 4 && p.list_cap == 0 + 4 + 4 + 0);
  CHECK(image_equals(p, naive(paths, lists), lists));
  CHECK(image_equals(p, {{}, {5, 6, 5, 6}, {9}, {}}, lists));
  CHECK(p.o_poff % 8 == 0 && p.o_sbase % 8 == 0 && p.o_toff % 8 == 0 && p.o_tcnt % 4 == 0 && p.o_slots % 4 == 0);
  CHECK(p.o_slots + 4 * (2 + 0 + 4 + 3) <= p.image.size());
  // the search part of the image is the flat map's: the same routing
  const uint8_t k[] = {0, 2};
  CHECK(range_route_one(p, k, 2) == 2 && range_route_one(p, k, 1) == 0);
  // h_seg_ids NULL when every list is empty
  const uint64_t soff[] = {0, 0};
  const uint32_t cap1[] = {5}, path1[] = {0};
  const uint64_t poff1[] = {0, 1};
  CHECK(plan_range_map_segments(1, nullptr, nullptr, path1, poff1, 1, cap1, nullptr, soff, &p, nullptr) == 0);
  CHECK(p.max_list == 5 && p.list_cap == 5 && image_equals(p, {{}}, {{}}));
}

// a random table: a root segment in every non-empty path, paths of 0-5 segments
struct Model {
  std::vector<Ids> paths, lists;
  Ids caps;
};
static Model random_model(std::mt19937_64& rng, uint32_t R, uint32_t S, uint32_t max_cap) {
  Model m;
  for (uint32_t s = 0; s < S; s++) {
    const uint32_t cap = rng() % 5 == 0 ? 0 : (uint32_t)(rng() % (max_cap + 1));
    m.caps.push_back(cap);
    Ids l(rng() % 4 == 0 ? cap : rng() % (cap + 1));
    for (auto& x : l) x = (uint32_t)(rng() % 1000);
    m.lists.push_back(l);
  }
  for (uint32_t r = 0; r < R; r++) {
    Ids p;
    const uint32_t n = (uint32_t)(rng() % 6);
    if (n) p.push_back(0);
    for (uint32_t j = 1; j < n; j++) p.push_back((uint32_t)(rng() % S));
    m.paths.push_back(p);
  }
  return m;
}

static void check_flatten_random() {
  std::mt19937_64 rng(20261021);
  uint64_t tables = 0, multi_tile = 0;
  for (int i = 0; i < 60; i++) {
    const uint32_t R = i % 10 == 0 ? 2 * RANGE_TILE + 1 + (uint32_t)(rng() % 500) : 1 + (uint32_t)(rng() % 300);
    const uint32_t S = 1 + (uint32_t)(rng() % 40);
    Model m = random_model(rng, R, S, 70);
    RangeSegPlan p;
    CHECK(plan_of(make_table(m.paths, m.lists, m.caps, rng() % 5, rng() % 5), &p) == 0);
    uint32_t want_max = 0;
    uint64_t want_cap = 0;
    for (const Ids& path : m.paths) {
      uint32_t c = 0;
      for (uint32_t s : path) c += m.caps[s];
      want_max = std::max(want_max, c);
      want_cap += c;
    }
    CHECK(p.max_list == want_max && p.list_cap == want_cap);
    CHECK(image_equals(p, naive(m.paths, m.lists), m.lists));
    tables++;
    multi_tile += R > RANGE_TILE;
  }
  CHECK(tables == 60 && multi_tile >= 6);
}

// what a plan's launches hold, checked against the call: returns false on any breach
static bool check_cut(const RangeSegUpdatePlan& plan, const Ids& seg_id, const Ids& ids,
                      const std::vector<uint64_t>& off) {
  bool ok = true;
  const uint32_t count = (uint32_t)seg_id.size();
  // the kept entries: the last of every id, in the call's order
  std::vector<uint32_t> want;
  for (uint32_t i = 0; i < count; i++) {
    bool last = true;
    for (uint32_t j = i + 1; j < count; j++) last = last && seg_id[j] != seg_id[i];
    if (last) want.push_back(i);
  }
  ok = ok && plan.order == want;
  ok = ok && (count == 0 ? plan.launches() == 0 : plan.launches() >= 1 && plan.cuts.front() == 0 &&
                                                      plan.cuts.back() == plan.pieces.size());
  size_t at = 0;  // the next kept entry, and how much of it has gone out
  uint32_t done = 0;
  for (uint32_t l = 0; l < plan.launches() && ok; l++) {
    const uint32_t first = plan.cuts[l], np = plan.cuts[l + 1] - first;
    ok = ok && np >= 1;
    uint64_t words = (uint64_t)RANGE_SEG_PIECE_WORDS * np;
    std::set<uint32_t> segs;
    for (uint32_t k = 0; k < np && ok; k++) {
      const RangeSegPiece& pc = plan.pieces[first + k];
      words += pc.n;
      ok = ok && segs.insert(pc.seg).second;  // no segment twice in one launch
      ok = ok && at < want.size();
      if (!ok) break;
      const uint32_t i = want[at], n = (uint32_t)(off[i + 1] - off[i]);
      // pieces of a list contiguous and in order, the length on the last alone
      ok = ok && pc.seg == seg_id[i] && pc.dst == done && pc.src == off[i] + done && done + pc.n <= n;
      done += pc.n;
      ok = ok && pc.len == (done == n ? n : RANGE_SEG_NO_LEN);
      if (done == n) at++, done = 0;
      else ok = ok && k + 1 == np && pc.n > 0;  // a cut list ends its launch
    }
    ok = ok && words <= RANGE_SEG_WORDS;  // no launch over the argument room
    RangeSegUpdate a{};
    if (ok) {
      range_seg_fill_launch(plan, l, ids.data(), &a);
      ok = ok && a.npieces == np;
      for (uint32_t k = 0; k < np && ok; k++) {
        const RangeSegPiece& pc = plan.pieces[first + k];
        const uint32_t* w = a.w + RANGE_SEG_PIECE_WORDS * k;
        ok = ok && w[0] == pc.seg && w[1] == pc.dst && w[3] == pc.n && w[4] == pc.len && w[2] + pc.n <= RANGE_SEG_WORDS;
        for (uint32_t j = 0; j < pc.n && ok; j++) ok = a.w[w[2] + j] == ids[pc.src + j];
      }
    }
  }
  return ok && at == want.size() && done == 0;
}

static void check_update_refusals() {
  RangeSegState st;
  const uint32_t caps[] = {4, 0, 2000};
  st.init(caps, 3);
  RangeSegUpdatePlan plan;
  plan.cuts = {0, 9};  // a refused call leaves the plan and the state as they were
  std::string err;
  const uint32_t seg[] = {0, 2}, ids[] = {1, 2, 3, 4, 5};
  const uint64_t off[] = {0, 2, 5};
  const RangeSegState before = st;
  auto untouched = [&] {
    return plan.cuts == std::vector<uint32_t>({0, 9}) && st.gen == before.gen && st.mark == before.mark &&
           st.cap == before.cap;
  };
  CHECK(plan_range_seg_update(nullptr, 2, seg, ids, off, &plan, &err) == RF_AMD_EINVAL);
  CHECK(plan_range_seg_update(&st, 2, seg, ids, off, nullptr, &err) == RF_AMD_EINVAL);
  CHECK(plan_range_seg_update(&st, 2, nullptr, ids, off, &plan, &err) == RF_AMD_EINVAL && untouched());
  CHECK(plan_range_seg_update(&st, 2, seg, ids, nullptr, &plan, &err) == RF_AMD_EINVAL && untouched());
  CHECK(plan_range_seg_update(&st, 2, seg, nullptr, off, &plan, &err) == RF_AMD_EINVAL && untouched());
  CHECK(err.find("null ids") != std::string::npos);
  const uint32_t bad_seg[] = {0, 3};
  CHECK(plan_range_seg_update(&st, 2, bad_seg, ids, off, &plan, &err) == RF_AMD_EINVAL && untouched());
  CHECK(err.find("num_segments") != std::string::npos);
  const uint64_t dec[] = {0, 3, 2};
  CHECK(plan_range_seg_update(&st, 2, seg, ids, dec, &plan, &err) == RF_AMD_EINVAL && untouched());
  CHECK(err.find("offsets decrease") != std::string::npos);
  const uint64_t lng[] = {0, 5, 5};  // 5 ids into a segment of 4
  CHECK(plan_range_seg_update(&st, 2, seg, ids, lng, &plan, &err) == RF_AMD_EINVAL && untouched());
  CHECK(err.find("capacity") != std::string::npos);
  const uint32_t zero_seg[] = {1};  // cap == 0: the empty list is its only legal one
  const uint64_t one[] = {0, 1}, none[] = {3, 3};
  CHECK(plan_range_seg_update(&st, 1, zero_seg, ids, one, &plan, &err) == RF_AMD_EINVAL && untouched());
  CHECK(plan_range_seg_update(&st, 1, zero_seg, nullptr, none, &plan, nullptr) == 0);
  CHECK(plan.launches() == 1 && plan.pieces.size() == 1 && plan.pieces[0].n == 0 && plan.pieces[0].len == 0);
  // count == 0: no launch
  CHECK(plan_range_seg_update(&st, 0, nullptr, nullptr, nullptr, &plan, nullptr) == 0 && plan.launches() == 0);
  CHECK(plan_range_seg_update(&st, 2, seg, ids, off, &plan, nullptr) == 0 && plan.launches() == 1);
}

static void check_cuts() {
  CHECK(RANGE_SEG_LAUNCH_IDS + RANGE_SEG_PIECE_WORDS == RANGE_SEG_WORDS);
  const uint32_t big = 4 * RANGE_SEG_LAUNCH_IDS;
  const Ids caps = {big, big, big, 3, 0};
  RangeSegState st;
  st.init(caps.data(), (uint32_t)caps.size());
  RangeSegUpdatePlan plan;
  auto run = [&](const Ids& seg_id, const std::vector<uint32_t>& lens) {
    std::vector<uint64_t> off = {0};
    for (uint32_t n : lens) off.push_back(off.back() + n);
    Ids ids(off.back());
    for (size_t i = 0; i < ids.size(); i++) ids[i] = (uint32_t)(i * 2654435761u);
    const int rc = plan_range_seg_update(&st, (uint32_t)seg_id.size(), seg_id.data(), ids.data(), off.data(), &plan,
                                         nullptr);
    return rc == 0 && check_cut(plan, seg_id, ids, off);
  };
  // one list that just fits, one id more, three times the room
  CHECK(run({0}, {RANGE_SEG_LAUNCH_IDS}) && plan.launches() == 1);
  CHECK(run({0}, {RANGE_SEG_LAUNCH_IDS + 1}) && plan.launches() == 2 && plan.pieces[1].n == 1);
  CHECK(run({0}, {3 * RANGE_SEG_LAUNCH_IDS}) && plan.launches() == 3);
  CHECK(run({0}, {3 * RANGE_SEG_LAUNCH_IDS + 1}) && plan.launches() == 4);
  // a list cut behind others in its launch; an empty list where exactly a piece header fits
  CHECK(run({3, 0, 1}, {3, RANGE_SEG_LAUNCH_IDS, 10}) && plan.launches() == 2);
  CHECK(run({0, 4, 3}, {RANGE_SEG_WORDS - 2 * RANGE_SEG_PIECE_WORDS, 0, 2}) && plan.launches() == 2 &&
        plan.cuts[1] == 2);
  CHECK(run({0, 3}, {RANGE_SEG_WORDS - 2 * RANGE_SEG_PIECE_WORDS, 2}) && plan.launches() == 2 &&
        plan.pieces.size() == 2);  // a header alone is no room for a list with ids: it is not cut there
  // repeated ids: the last entry wins and keeps its place
  CHECK(run({0, 3, 0, 1, 3}, {5, 1, 7, 2, 3}) && plan.order == std::vector<uint32_t>({2, 3, 4}));
  CHECK(run({1, 1, 1}, {big, 1, RANGE_SEG_LAUNCH_IDS + 1}) && plan.order == std::vector<uint32_t>({2}) &&
        plan.launches() == 2);
  // many small lists: 200 pieces of 1 id, 6 words each
  {
    std::vector<uint32_t> caps2(200, 1);
    RangeSegState st2;
    st2.init(caps2.data(), 200);
    Ids seg_id(200), ids(200, 7u);
    std::vector<uint64_t> off(201);
    for (uint32_t i = 0; i < 200; i++) seg_id[i] = 199 - i, off[i + 1] = i + 1;
    CHECK(plan_range_seg_update(&st2, 200, seg_id.data(), ids.data(), off.data(), &plan, nullptr) == 0);
    CHECK(check_cut(plan, seg_id, ids, off) && plan.launches() == 2 && plan.cuts[1] == RANGE_SEG_WORDS / 6);
  }
  // random calls
  std::mt19937_64 rng(99);
  for (int it = 0; it < 300; it++) {
    const uint32_t count = 1 + (uint32_t)(rng() % 12);
    Ids seg_id;
    std::vector<uint32_t> lens;
    for (uint32_t i = 0; i < count; i++) {
      const uint32_t s = (uint32_t)(rng() % caps.size());
      seg_id.push_back(s);
      const uint32_t how = (uint32_t)(rng() % 6);
      const uint32_t want = how == 0 ? RANGE_SEG_LAUNCH_IDS + (uint32_t)(rng() % 3) - 1
                            : how == 1 ? (uint32_t)(rng() % big) : (uint32_t)(rng() % 300);
      lens.push_back(std::min(want, caps[s]));
    }
    if (!run(seg_id, lens)) {
      printf("random cut %d failed\n", it);
      g_failed++;
    }
  }
}

static void check_update_sequences() {
  std::mt19937_64 rng(4242);
  uint64_t steps = 0, repeats = 0, cut_lists = 0;
  for (int table = 0; table < 12; table++) {
    const uint32_t R = table % 4 == 0 ? 2 * RANGE_TILE + 5 : 1 + (uint32_t)(rng() % 200);
    const uint32_t S = 2 + (uint32_t)(rng() % 30);
    Model m = random_model(rng, R, S, table % 4 == 1 ? 2500 : 60);  // lists longer than a launch's room
    // a path's capacities must stay under the limit: cut the paths where they do not
    for (Ids& p : m.paths) {
      uint64_t room = 0;
      size_t keep = 0;
      while (keep < p.size() && room + m.caps[p[keep]] <= RANGE_MAX_LIST) room += m.caps[p[keep++]];
      p.resize(keep);
    }
    RangeSegPlan p;
    CHECK(plan_of(make_table(m.paths, m.lists, m.caps), &p) == 0);
    const uint32_t max_list = p.max_list;
    RangeSegState st;
    st.init(m.caps.data(), S);
    RangeSegUpdatePlan plan;
    const RangeSegDev d = range_seg_dev(p, p.image.data());
    RangeSegUpdate a{};
    a.slots = d.slots, a.slen = d.slen, a.sbase = d.sbase, a.scap = d.scap, a.num_segments = S;
    for (int step = 0; step < 25; step++) {
      const uint32_t count = 1 + (uint32_t)(rng() % 6);
      Ids seg_id, ids;
      std::vector<uint64_t> off = {0};
      for (uint32_t i = 0; i < count; i++) {
        const uint32_t s = i && rng() % 4 == 0 ? seg_id[rng() % i] : (uint32_t)(rng() % S);
        const uint32_t n = rng() % 3 == 0 ? m.caps[s] : (uint32_t)(rng() % (m.caps[s] + 1));
        seg_id.push_back(s);
        for (uint32_t j = 0; j < n; j++) ids.push_back((uint32_t)(rng() % 100000));
        off.push_back(ids.size());
      }
      ids.push_back(0xEEEEEEEEu);
      CHECK(plan_range_seg_update(&st, count, seg_id.data(), ids.data(), off.data(), &plan, nullptr) == 0);
      CHECK(check_cut(plan, seg_id, ids, off));
      repeats += plan.order.size() < count;
      cut_lists += plan.pieces.size() > plan.order.size();
      for (uint32_t l = 0; l < plan.launches(); l++) {
        range_seg_fill_launch(plan, l, ids.data(), &a);
        range_seg_scatter_host(a);
      }
      range_seg_flatten_host(d);
      for (uint32_t i = 0; i < count; i++)  // the model: in the call's order, so the last entry wins
        m.lists[seg_id[i]].assign(ids.begin() + off[i], ids.begin() + off[i + 1]);
      if (!image_equals(p, naive(m.paths, m.lists), m.lists)) {
        printf("table %d step %d: the image differs from the model\n", table, step);
        g_failed++;
      }
      CHECK(p.max_list == max_list);
      steps++;
    }
  }
  CHECK(steps == 300 && repeats > 20 && cut_lists > 5);
  printf("update sequences: %llu steps, %llu with a repeated id, %llu with a list cut into pieces\n",
         (unsigned long long)steps, (unsigned long long)repeats, (unsigned long long)cut_lists);
}

int main() {
  check_refusals();
  check_legal_edges();
  check_flatten_random();
  check_update_refusals();
  check_cuts();
  check_update_sequences();
  if (g_failed) {
    printf("range_seg_check: %d FAILED\n", g_failed);
    return 1;
  }
  printf("range_seg_check: OK\n");
  return 0;
}
