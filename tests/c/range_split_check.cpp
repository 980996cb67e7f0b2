// range_split_check -- the planner of a range map that follows node splits
// (splinterdb_amd/csrc/rf_range_split_plan.h) checked on the host: the create with room and its
// refusals; random sequences of splits and set_paths applied to the plan's image by the host
// mirror of the splice (the launches' arguments stored into the other structural copy, poisoned
// beforehand, then the flatten) against a naive model -- vectors of byte strings and of paths,
// rebuilt from scratch with plan_range_map_segments after every edit: the structural sections and
// the flat table must be equal byte for byte; every refusal with its code and nothing changed;
// the cut into launches at the exact word limits; RF_AMD_ENOSPC at exactly one past each room
// field and success at exactly full. Built (with the address and undefined-behaviour sanitizers)
// and run by tests/test_range_split_plan.py; needs no device. Prints "range_split_check: OK".
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "rf_range_split_plan.h"

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
typedef std::string Key;  // compared as unsigned bytes below, never with operator<

static bool key_lt(const Key& a, const Key& b) {  // slice_lex_cmp(a, b) < 0
  return !range_key_le((const uint8_t*)b.data(), b.size(), (const uint8_t*)a.data(), a.size());
}

// the naive model: the map is its boundaries, its paths and its segments
struct Model {
  std::vector<Key> bounds;
  std::vector<Ids> paths, lists;
  Ids caps;
};

// the caller's arrays of some boundaries and paths, with spare elements behind and offsets that
// do not start at 0
struct Arrays {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> boff, poff;
  std::vector<uint32_t> path;
  Arrays(const std::vector<Key>& bounds, const std::vector<Ids>& paths, uint64_t b0 = 0, uint64_t p0 = 0) {
    bytes.assign(b0, 0xEE);
    boff.push_back(b0);
    for (const Key& k : bounds) {
      bytes.insert(bytes.end(), k.begin(), k.end());
      boff.push_back(bytes.size());
    }
    bytes.push_back(0xEE);
    path.assign(p0, 0xEEEEEEEEu);
    poff.push_back(p0);
    for (const Ids& p : paths) {
      path.insert(path.end(), p.begin(), p.end());
      poff.push_back(path.size());
    }
    path.push_back(0xEEEEEEEEu);
  }
};

struct SegArrays {
  std::vector<uint32_t> cap, ids;
  std::vector<uint64_t> soff;
  explicit SegArrays(const Model& m) : cap(m.caps) {
    soff.push_back(0);
    for (const Ids& l : m.lists) {
      ids.insert(ids.end(), l.begin(), l.end());
      soff.push_back(ids.size());
    }
    ids.push_back(0);
    cap.push_back(0);
  }
};

static rf_amd_range_room used_of(const Model& m) {
  rf_amd_range_room u{};
  u.ranges = (uint32_t)m.paths.size();
  for (const Key& k : m.bounds) u.bound_bytes += k.size();
  for (const Ids& p : m.paths) {
    uint64_t c = 0;
    for (uint32_t s : p) c += m.caps[s];
    u.path_entries += p.size();
    u.list_ids += c;
    if (c > u.max_list) u.max_list = (uint32_t)c;
  }
  return u;
}

static int plan_compact(const Model& m, RangeSegPlan* p) {
  const Arrays a(m.bounds, m.paths);
  const SegArrays s(m);
  return plan_range_map_segments((uint32_t)m.paths.size(), a.bytes.data(), a.boff.data(), a.path.data(),
                                 a.poff.data(), (uint32_t)m.lists.size(), s.cap.data(), s.ids.data(), s.soff.data(),
                                 p, nullptr);
}

// a roomy map on the host: the plan's image, the state and what the engine keeps beside them
struct HostMap {
  RangeRoomPlan plan;
  RangeSplitState st;
  RangeSegState seg;
  RangeSegDev dev{};
  uint32_t launches = 0;  // of the last edit
};

static int create(const Model& m, const rf_amd_range_room& room, HostMap* h, std::string* err = nullptr,
                  bool null_bounds = false) {
  const Arrays a(m.bounds, m.paths, 3, 5);
  const SegArrays s(m);
  const uint32_t R = (uint32_t)m.paths.size(), S = (uint32_t)m.lists.size();
  const uint8_t* bb = null_bounds ? nullptr : a.bytes.data();
  const uint64_t* bo = null_bounds ? nullptr : a.boff.data();
  if (int rc = plan_range_map_segments_room(R, bb, bo, a.path.data(), a.poff.data(), S, s.cap.data(), s.ids.data(),
                                            s.soff.data(), &room, &h->plan, err))
    return rc;
  h->seg.init(s.cap.data(), S);
  h->st.init(room, R, bb, bo, a.path.data(), a.poff.data(), s.cap.data());
  h->dev = range_seg_dev(h->plan, h->plan.image.data());
  return 0;
}

// what rf_amd_range_map_split and _set_paths do behind an accepted plan, on the host
static void run_plan(HostMap* h, const RangeSplicePlan& sp, const Arrays& a) {
  uint8_t* base = h->plan.image.data();
  const RangeStructDev to = range_struct_dev(h->plan, base, h->st.live);
  // poison the copy the edit writes: an element the splice leaves out shows
  const rf_amd_range_room& rm = h->plan.room;
  memset(to.prefix, 0xEE, 8ull * (rm.ranges - 1));
  memset(to.boff, 0xEE, 8ull * rm.ranges);
  memset(to.poff, 0xEE, 8ull * (rm.ranges + 1));
  memset(to.bytes, 0xEE, rm.bound_bytes);
  memset(to.path, 0xEE, 4 * rm.path_entries);
  RangeSpliceArgs args{};
  args.src = range_struct_dev(h->plan, base, h->st.live ^ 1u);
  args.dst = to;
  for (uint32_t l = 0; l < sp.launches(); l++) {
    memset(args.w, 0xEE, sizeof(args.w));
    range_splice_fill_launch(sp, l, a.bytes.data(), a.boff.data(), a.path.data(), a.poff.data(), &args);
    CHECK(args.bulk == (l == 0));
    const uint64_t words = range_splice_words(args.bn, args.yn, args.pn, args.qn);
    CHECK(words <= RANGE_SPLICE_WORDS && args.qw + args.qn == words);
    CHECK(l + 1 == sp.launches() || words + RANGE_SPLICE_BOUND_WORDS > RANGE_SPLICE_WORDS);  // full but the last
    range_splice_host(args);
  }
  h->launches = sp.launches();
  h->dev.num_ranges = sp.e.r_new;
  h->dev.poff = to.poff;
  h->dev.path = to.path;
  range_seg_flatten_host(h->dev);
}

static int split(HostMap* h, uint32_t r, const std::vector<Key>& nb, const std::vector<Ids>& np,
                 std::string* err = nullptr) {
  const Arrays a(nb, np, 7, 2);
  RangeSplicePlan sp;
  if (int rc = plan_range_split(&h->st, h->seg, r, (uint32_t)np.size(), a.bytes.data(), a.boff.data(), a.path.data(),
                                a.poff.data(), &sp, err))
    return rc;
  run_plan(h, sp, a);
  return 0;
}

static int set_paths(HostMap* h, uint32_t first, const std::vector<Ids>& np, std::string* err = nullptr) {
  const Arrays a({}, np, 0, 9);
  RangeSplicePlan sp;
  if (int rc = plan_range_set_paths(&h->st, h->seg, first, (uint32_t)np.size(), a.path.data(), a.poff.data(), &sp,
                                    err))
    return rc;
  run_plan(h, sp, a);
  return 0;
}

static void model_split(Model* m, uint32_t r, const std::vector<Key>& nb, const std::vector<Ids>& np) {
  m->bounds.insert(m->bounds.begin() + r, nb.begin(), nb.end());
  m->paths.erase(m->paths.begin() + r);
  m->paths.insert(m->paths.begin() + r, np.begin(), np.end());
}

// the live structural sections, the flat table and the host state equal the plan rebuilt from the
// model, byte for byte
static bool equals_rebuilt(HostMap& h, const Model& m) {
  RangeSegPlan c;
  if (plan_compact(m, &c)) return false;
  const uint64_t R = m.paths.size();
  const rf_amd_range_room u = used_of(m);
  uint8_t* base = h.plan.image.data();
  const uint8_t* want = c.image.data();
  const RangeStructDev s = range_struct_dev(h.plan, base, h.st.live);
  const uint64_t* loff = reinterpret_cast<const uint64_t*>(want + c.o_loff);
  bool ok = h.dev.num_ranges == R && h.st.num_ranges() == R;
  ok = ok && !memcmp(s.prefix, want + c.o_prefix, 8 * (R - 1)) && !memcmp(s.boff, want + c.o_boff, 8 * R);
  ok = ok && !memcmp(s.bytes, want + c.o_bytes, u.bound_bytes) && !memcmp(s.poff, want + c.o_poff, 8 * (R + 1));
  ok = ok && !memcmp(s.path, want + c.o_path, 4 * u.path_entries);
  ok = ok && !memcmp(h.dev.loff, loff, 8 * (R + 1)) && !memcmp(h.dev.list, want + c.o_list, 4 * loff[R]);
  // the state the host validates the next edit with
  ok = ok && h.st.bound_bytes() == u.bound_bytes && h.st.path_entries() == u.path_entries &&
       h.st.list_ids == u.list_ids && h.st.list_ids == c.list_cap;
  ok = ok && !memcmp(h.st.boff.data(), want + c.o_boff, 8 * R) && !memcmp(h.st.poff.data(), want + c.o_poff, 8 * (R + 1));
  ok = ok && (u.bound_bytes == 0 || !memcmp(h.st.bytes.data(), want + c.o_bytes, u.bound_bytes));
  for (uint64_t r = 0; r < R && ok; r++) {
    uint64_t cap = 0;
    for (uint32_t x : m.paths[r]) cap += m.caps[x];
    ok = h.st.pcap[r] == cap;
  }
  return ok;
}

struct Snapshot {
  std::vector<uint8_t> image;
  RangeSplitState st;
  explicit Snapshot(const HostMap& h) : image(h.plan.image), st(h.st) {}
  bool same(const HostMap& h) const {
    return image == h.plan.image && st.boff == h.st.boff && st.bytes == h.st.bytes && st.poff == h.st.poff &&
           st.pcap == h.st.pcap && st.list_ids == h.st.list_ids && st.live == h.st.live;
  }
};

static const rf_amd_range_room BIG_ROOM = {5000, 200000, 100000, 4000000, 4000};

static Model small_model() {
  Model m;
  m.bounds = {"b", "d", "dd"};
  m.paths = {{0, 1}, {0, 2}, {0}, {}};
  m.lists = {{1, 2}, {3}, {}, {9}, {}};
  m.caps = {4, 1, 2, 5, 0};
  return m;
}

static void check_create() {
  const Model m = small_model();
  const rf_amd_range_room u = used_of(m);
  CHECK(u.ranges == 4 && u.bound_bytes == 4 && u.path_entries == 5 && u.list_ids == 15 && u.max_list == 6);
  HostMap h;
  std::string err;
  CHECK(create(m, u, &h) == 0 && equals_rebuilt(h, m));  // a room that is exactly the table
  CHECK(h.plan.max_list == 6 && h.plan.list_cap == 15 && h.plan.num_ranges == 4);
  rf_amd_range_room big = u;
  big.max_list = RANGE_MAX_LIST;
  CHECK(create(m, big, &h) == 0 && h.plan.max_list == RANGE_MAX_LIST && equals_rebuilt(h, m));
  HostMap keep;
  CHECK(create(m, u, &keep) == 0);
  const Snapshot before(keep);
  auto refused = [&](rf_amd_range_room r, const char* word) {
    err.clear();
    const bool ok = create(m, r, &keep, &err) == RF_AMD_EINVAL && err.find(word) != std::string::npos &&
                    before.same(keep);
    if (!ok) printf("  expected a refusal with '%s', message '%s'\n", word, err.c_str());
    return ok;
  };
  rf_amd_range_room r = u;
  r.ranges--;
  CHECK(refused(r, "room.ranges"));
  r = u, r.bound_bytes--;
  CHECK(refused(r, "room.bound_bytes"));
  r = u, r.path_entries--;
  CHECK(refused(r, "room.path_entries"));
  r = u, r.list_ids--;
  CHECK(refused(r, "room.list_ids"));
  r = u, r.max_list--;
  CHECK(refused(r, "room.max_list"));
  r = big, r.max_list++;
  CHECK(refused(r, "65,535"));
  // what the roomless create refuses, the roomy one refuses
  Model bad = m;
  bad.bounds = {"b", "b", "c"};
  err.clear();
  CHECK(create(bad, BIG_ROOM, &keep, &err) == RF_AMD_EINVAL && err.find("ascending") != std::string::npos);
  bad = m, bad.paths[1] = {0, 5};
  CHECK(create(bad, BIG_ROOM, &keep, &err) == RF_AMD_EINVAL && err.find("num_segments") != std::string::npos);
  CHECK(before.same(keep));
  RangeRoomPlan p;
  const Arrays a(m.bounds, m.paths);
  const SegArrays s(m);
  CHECK(plan_range_map_segments_room(4, a.bytes.data(), a.boff.data(), a.path.data(), a.poff.data(), 5, s.cap.data(),
                                     s.ids.data(), s.soff.data(), nullptr, &p, &err) == RF_AMD_EINVAL &&
        err.find("null room") != std::string::npos && p.image.empty());
  // R == 1 with NULL boundary arrays, the map every trunk starts as
  Model one;
  one.paths = {{0}};
  one.lists = {{4, 5}};
  one.caps = {3};
  CHECK(create(one, BIG_ROOM, &h, nullptr, true) == 0 && equals_rebuilt(h, one) && h.st.bound_bytes() == 0);
  printf("create with room: OK\n");
}

static void check_refusals() {
  const Model m = small_model();
  rf_amd_range_room room = BIG_ROOM;
  room.max_list = 9;
  HostMap h;
  CHECK(create(m, room, &h) == 0);
  const Snapshot before(h);
  std::string err;
  auto refused = [&](int rc, int want, const char* word) {
    const bool ok = rc == want && err.find(word) != std::string::npos && before.same(h);
    if (!ok) printf("  expected %d with '%s', got %d '%s'\n", want, word, rc, err.c_str());
    err.clear();
    return ok;
  };
  const int E = RF_AMD_EINVAL;
  // ranges: (-inf, b) [b, d) [d, dd) [dd, +inf)
  CHECK(refused(split(&h, 4, {}, {{0}}, &err), E, "num_ranges"));
  CHECK(refused(split(&h, 0xFFFFFFFFu, {}, {{0}}, &err), E, "num_ranges"));
  CHECK(refused(split(&h, 1, {}, {}, &err), E, "pieces == 0"));
  CHECK(refused(split(&h, 1, {"b"}, {{0}, {0}}, &err), E, "lower boundary"));    // equal to the lower
  CHECK(refused(split(&h, 1, {"a"}, {{0}, {0}}, &err), E, "lower boundary"));
  CHECK(refused(split(&h, 1, {"d"}, {{0}, {0}}, &err), E, "upper boundary"));    // equal to the upper
  CHECK(refused(split(&h, 1, {"c", "e"}, {{0}, {0}, {0}}, &err), E, "upper boundary"));
  CHECK(refused(split(&h, 1, {"c", "c"}, {{0}, {0}, {0}}, &err), E, "ascending"));
  CHECK(refused(split(&h, 1, {"cc", "c"}, {{0}, {0}, {0}}, &err), E, "ascending"));
  CHECK(refused(split(&h, 2, {Key("d\0", 2), "dd"}, {{0}, {0}, {0}}, &err), E, "upper boundary"));
  CHECK(refused(split(&h, 1, {""}, {{0}, {0}}, &err), E, "lower boundary"));     // zero-length: only the first
  CHECK(refused(split(&h, 3, {"dd"}, {{0}, {0}}, &err), E, "lower boundary"));
  CHECK(refused(split(&h, 0, {"b"}, {{0}, {0}}, &err), E, "upper boundary"));
  CHECK(refused(split(&h, 1, {"c"}, {{0}, {5}}, &err), E, "num_segments"));
  CHECK(refused(split(&h, 1, {}, {{0xFFFFFFFFu}}, &err), E, "num_segments"));
  CHECK(refused(split(&h, 1, {"c"}, {{0}, {0, 3, 1}}, &err), E, "room.max_list"));  // 4 + 5 + 1 > 9
  CHECK(refused(set_paths(&h, 0, {{0}, {0}, {0}, {0}, {0}}, &err), E, "num_ranges"));
  CHECK(refused(set_paths(&h, 4, {{0}}, &err), E, "num_ranges"));
  CHECK(refused(set_paths(&h, 5, {}, &err), E, "num_ranges"));
  CHECK(refused(set_paths(&h, 2, {{0}, {7}}, &err), E, "num_segments"));
  CHECK(refused(set_paths(&h, 2, {{3, 3}}, &err), E, "room.max_list"));
  // the raw arrays: decreasing offsets and NULLs
  RangeSplicePlan sp;
  const uint8_t bytes[4] = {'c', 'c', 'c', 'c'};
  const uint32_t path[4] = {0, 0, 0, 0};
  const uint64_t up[3] = {0, 1, 2}, down[3] = {2, 1, 2}, flat0[3] = {0, 0, 0};
  auto raw = [&](uint32_t r, uint32_t pieces, const uint8_t* bb, const uint64_t* bo, const uint32_t* pp,
                 const uint64_t* po) { return plan_range_split(&h.st, h.seg, r, pieces, bb, bo, pp, po, &sp, &err); };
  CHECK(refused(raw(1, 2, bytes, down, path, up), E, "boundary offsets decrease"));
  CHECK(refused(raw(1, 2, bytes, up, path, down), E, "path offsets decrease"));
  CHECK(refused(raw(1, 2, bytes, nullptr, path, up), E, "null boundary offsets"));
  CHECK(refused(raw(1, 2, nullptr, up, path, up), E, "null boundary bytes"));
  CHECK(refused(raw(1, 2, bytes, up, nullptr, up), E, "null paths"));
  CHECK(refused(raw(1, 2, bytes, up, path, nullptr), E, "null path offsets"));
  CHECK(refused(plan_range_set_paths(&h.st, h.seg, 1, 2, nullptr, up, &sp, &err), E, "null paths"));
  CHECK(refused(plan_range_set_paths(&h.st, h.seg, 1, 2, path, nullptr, &sp, &err), E, "null path offsets"));
  CHECK(refused(plan_range_split(nullptr, h.seg, 1, 1, nullptr, nullptr, path, up, &sp, &err), E, "null split state"));
  // legal with NULLs: pieces == 1 without boundary arrays, empty paths without a path array
  CHECK(raw(1, 1, nullptr, nullptr, nullptr, flat0) == 0 && sp.launches() == 1);
  CHECK(plan_range_set_paths(&h.st, h.seg, 0, 2, nullptr, flat0, &sp, &err) == 0);
  // and what was refused above is legal once well-formed
  Model now = small_model();
  CHECK(create(now, room, &h) == 0);
  CHECK(split(&h, 1, {"c"}, {{0}, {0, 3}}) == 0);
  model_split(&now, 1, {"c"}, {{0}, {0, 3}});
  CHECK(equals_rebuilt(h, now));
  CHECK(split(&h, 0, {""}, {{}, {1}}) == 0);  // a zero-length boundary as the very first of the map
  model_split(&now, 0, {""}, {{}, {1}});
  CHECK(equals_rebuilt(h, now));
  CHECK(split(&h, 0, {"a"}, {{0}, {0}}, &err) == E);  // nothing lies below the empty key
  printf("refusals: OK\n");
}

// ---- random sequences --------------------------------------------------------------------------
static Key rand_key(std::mt19937& g, const Key& head) {
  static const char alphabet[] = {'\0', 'a', '\x7f', '\x80', '\xff'};
  Key k = head;
  for (uint32_t n = g() % 6; n; n--) k.push_back(alphabet[g() % 5]);
  return k;
}

static Ids rand_path(std::mt19937& g, uint32_t S, uint32_t most) {
  Ids p;
  for (uint32_t n = g() % (most + 1); n; n--) p.push_back(g() % S);
  return p;
}

static uint32_t check_sequence(uint32_t seed, uint32_t steps, bool from_one) {
  std::mt19937 g(seed);
  Model m;
  const uint32_t S = 12;
  for (uint32_t s = 0; s < S; s++) {
    m.caps.push_back(g() % 4 ? g() % 9 : 0);
    Ids l;
    for (uint32_t n = m.caps[s] ? g() % (m.caps[s] + 1) : 0; n; n--) l.push_back(g() % 1000);
    m.lists.push_back(l);
  }
  if (from_one) {
    m.paths = {rand_path(g, S, 4)};
  } else {
    std::set<Key, bool (*)(const Key&, const Key&)> b(key_lt);
    while (b.size() < 40) b.insert(rand_key(g, g() % 2 ? "aaaaaaaa" : ""));
    m.bounds.assign(b.begin(), b.end());
    for (size_t r = 0; r <= m.bounds.size(); r++) m.paths.push_back(rand_path(g, S, 4));
  }
  HostMap h;
  CHECK(create(m, BIG_ROOM, &h, nullptr, from_one) == 0 && equals_rebuilt(h, m));
  uint32_t multi = 0;
  for (uint32_t step = 0; step < steps; step++) {
    const uint32_t R = (uint32_t)m.paths.size();
    const uint32_t kind = g() % 10;
    if (kind < 6) {  // a split: candidates strictly inside the range, in order
      const uint32_t r = kind == 0 ? 0 : kind == 1 ? R - 1 : g() % R;
      const uint32_t want = step % 37 == 5 ? 300 : g() % 5;  // now and then one of several launches
      std::set<Key, bool (*)(const Key&, const Key&)> in(key_lt);
      for (uint32_t t = 0; t < 4 * want + 4 && in.size() < want; t++) {
        // behind the lower boundary, so that a narrow range is hit too; or anywhere
        const Key k = rand_key(g, r && g() % 2 ? m.bounds[r - 1] : g() % 2 ? "aaaaaaaa" : "");
        if (r && !key_lt(m.bounds[r - 1], k)) continue;
        if (r < R - 1 && !key_lt(k, m.bounds[r])) continue;
        in.insert(k);
      }
      const std::vector<Key> nb(in.begin(), in.end());
      std::vector<Ids> np;
      for (size_t i = 0; i <= nb.size(); i++) np.push_back(rand_path(g, S, want == 300 ? 9 : 4));
      CHECK(split(&h, r, nb, np) == 0);
      model_split(&m, r, nb, np);
    } else if (kind < 9) {  // paths that grow, shrink and become empty
      const uint32_t first = g() % R, count = 1 + g() % std::min(R - first, 20u);
      std::vector<Ids> np;
      for (uint32_t i = 0; i < count; i++) np.push_back(g() % 3 ? rand_path(g, S, 6) : Ids());
      CHECK(set_paths(&h, first, np) == 0);
      std::copy(np.begin(), np.end(), m.paths.begin() + first);
    } else {  // a new root level: every path
      std::vector<Ids> np;
      for (uint32_t i = 0; i < R; i++) {
        Ids p = m.paths[i];
        p.insert(p.begin(), g() % S);
        np.push_back(p);
      }
      CHECK(set_paths(&h, 0, np) == 0);
      m.paths = np;
    }
    multi += h.launches > 1;
    if (!equals_rebuilt(h, m)) {
      printf("  seed %u step %u: the mirror differs from the rebuilt plan (R %zu)\n", seed, step, m.paths.size());
      g_failed++;
      break;
    }
  }
  return multi;
}

// ---- the cut into launches ---------------------------------------------------------------------
static void check_cuts() {
  const uint32_t W = RANGE_SPLICE_WORDS;
  Model m;
  m.paths = {{}};
  m.lists = {{}};
  m.caps = {0};
  // pieces == 1: two words for the range, the rest path entries
  for (int d = -1; d <= 1; d++) {
    HostMap h;
    CHECK(create(m, BIG_ROOM, &h, nullptr, true) == 0);
    const Ids p(W - 2 + d, 0u);
    CHECK(range_splice_words(0, 0, 1, p.size()) == W + d);
    CHECK(split(&h, 0, {}, {p}) == 0 && h.launches == (d > 0 ? 2u : 1u));
    Model now = m;
    now.paths = {p};
    CHECK(equals_rebuilt(h, now));
  }
  // two pieces: a boundary of 4 b - 3 .. 4 b bytes takes b words; one word under, at, one over
  for (int d = -1; d <= 1; d++)
    for (uint32_t blen : {1u, 4u, 5u, 105u}) {
      HostMap h;
      CHECK(create(m, BIG_ROOM, &h, nullptr, true) == 0);
      const uint32_t fixed = RANGE_SPLICE_BOUND_WORDS + (blen + 3) / 4 + 2 * RANGE_SPLICE_RANGE_WORDS;
      const Ids p(W - fixed + d, 0u);
      const Key k(blen, 'k');
      CHECK(range_splice_words(1, blen, 2, p.size()) == W + d);
      CHECK(split(&h, 0, {k}, {{}, p}) == 0 && h.launches == (d > 0 ? 2u : 1u));
      Model now = m;
      model_split(&now, 0, {k}, {{}, p});
      CHECK(equals_rebuilt(h, now));
    }
  // every kind cut in the middle: boundaries alone fill more than a launch, their bytes another
  {
    HostMap h;
    CHECK(create(m, BIG_ROOM, &h, nullptr, true) == 0);
    std::vector<Key> nb;
    std::vector<Ids> np = {{}};
    for (uint32_t j = 0; j < W / 4 + 10; j++) {
      char buf[16];
      snprintf(buf, sizeof buf, "%06u-key", j);
      nb.push_back(Key(buf) + Key(j % 7, 'x'));
      np.push_back(Ids(j % 5, 0u));
    }
    const uint64_t words = range_splice_words(nb.size(), used_of(Model{nb, np, m.lists, m.caps}).bound_bytes,
                                              np.size(), used_of(Model{nb, np, m.lists, m.caps}).path_entries);
    CHECK(split(&h, 0, nb, np) == 0 && h.launches >= 3 && h.launches <= words / W + 4);
    Model now = m;
    model_split(&now, 0, nb, np);
    CHECK(equals_rebuilt(h, now));
    // three launches with the last one partly filled
    const Ids p(2 * W + W / 3, 0u);
    CHECK(set_paths(&h, 5, {p, {}, p}) == 0 && h.launches == 5);
    now.paths[5] = p, now.paths[6] = {}, now.paths[7] = p;
    CHECK(equals_rebuilt(h, now));
    CHECK(set_paths(&h, 5, {{}, p}) == 0 && h.launches == 3);
    now.paths[5] = {}, now.paths[6] = p;
    CHECK(equals_rebuilt(h, now));
  }
  printf("cuts: OK\n");
}

// ---- room --------------------------------------------------------------------------------------
static void check_room() {
  const Model m = small_model();
  const rf_amd_range_room u = used_of(m);  // 4 ranges, 4 bytes, 5 entries, 15 ids
  std::string err;
  // each field in turn exactly filled by an edit, then one past it
  struct Case {
    const char* word;
    rf_amd_range_room room;
  };
  // the edit: range 1 [b, d) into three, boundaries "c", "cc" (3 bytes), paths {0} {0 3} {0 2}:
  // ranges + 2, bytes + 3, entries 5 - 2 + 5 = 8, ids 15 - 6 + (4 + 9 + 6) = 28
  const std::vector<Key> nb = {"c", "cc"};
  const std::vector<Ids> np = {{0}, {0, 3}, {0, 2}};
  const rf_amd_range_room full = {6, 7, 8, 28, 9};
  Model after = m;
  model_split(&after, 1, nb, np);
  const rf_amd_range_room ua = used_of(after);
  CHECK(ua.ranges == full.ranges && ua.bound_bytes == full.bound_bytes && ua.path_entries == full.path_entries &&
        ua.list_ids == full.list_ids && ua.max_list == full.max_list);
  HostMap h;
  CHECK(create(m, full, &h) == 0 && split(&h, 1, nb, np) == 0 && equals_rebuilt(h, after));  // exactly full
  // a full map still takes edits that do not grow it
  CHECK(split(&h, 2, {}, {{0, 3}}) == 0 && set_paths(&h, 0, {{1, 0}}) == 0);
  after.paths[0] = {1, 0};
  CHECK(equals_rebuilt(h, after));
  {
    const Snapshot before(h);
    CHECK(split(&h, 5, {"e"}, {{}, {}}, &err) == RF_AMD_ENOSPC && err.find("room.ranges") != std::string::npos);
    CHECK(set_paths(&h, 5, {{4}}, &err) == RF_AMD_ENOSPC && err.find("room.path_entries") != std::string::npos);
    CHECK(set_paths(&h, 2, {{0, 3, 4, 4, 4}}, &err) == RF_AMD_ENOSPC);  // entries, with ids to spare
    CHECK(set_paths(&h, 5, {{1}}, &err) == RF_AMD_ENOSPC);
    CHECK(before.same(h));
  }
  const Case cases[] = {{"room.ranges", {5, 7, 8, 28, 9}},
                        {"room.bound_bytes", {6, 6, 8, 28, 9}},
                        {"room.path_entries", {6, 7, 7, 28, 9}},
                        {"room.list_ids", {6, 7, 8, 27, 9}}};
  for (const Case& c : cases) {
    HostMap one;
    CHECK(create(m, c.room, &one) == 0);
    const Snapshot before(one);
    err.clear();
    CHECK(split(&one, 1, nb, np, &err) == RF_AMD_ENOSPC && err.find(c.word) != std::string::npos && before.same(one));
    // the same map takes an edit that fits
    CHECK(split(&one, 1, {"c"}, {{0}, {0}}) == 0);
  }
  // max_list is EINVAL, not ENOSPC: the call is malformed for this map whatever is free
  rf_amd_range_room r = full;
  r.max_list = 8;
  HostMap one;
  CHECK(create(m, r, &one) == 0 && split(&one, 1, nb, np, &err) == RF_AMD_EINVAL);
  (void)u;
  printf("room: OK\n");
}

int main() {
  static_assert(RANGE_SPLICE_WORDS % 4 == 0 && RANGE_SPLICE_WORDS > 64, "the cut tests' shapes");
  check_create();
  check_refusals();
  uint32_t multi = 0, steps = 0;
  for (uint32_t seed = 1; seed <= 6; seed++) {
    multi += check_sequence(seed, 60, seed % 2 == 1);
    steps += 60;
  }
  CHECK(multi >= 4);
  printf("edit sequences: %u steps, %u of several launches\n", steps, multi);
  check_cuts();
  check_room();
  if (g_failed) {
    printf("range_split_check: %d checks FAILED\n", g_failed);
    return 1;
  }
  printf("range_split_check: OK\n");
  return 0;
}
