// rf_engine.cpp -- host runtime of the MI355X routing-filter engine (C ABI: include/rf_amd.h).
//
// Owns device workspaces, gives each batch the buffers its plan asks for (the plan itself --
// geometry of src/routing_filter.c:357-389 per filter, plus the coarse-bucket / page-bound
// bookkeeping of this engine -- is rf_batch_plan.h's, host-only) and issues the kernel
// sequence of rf_kernels.hip on one HIP stream. No compute happens on the host: there is no
// CPU fallback, and every entry point fails with ENODEV when no HIP device is present.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <x86intrin.h>

#include <map>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rf_amd.h"
#include "../../include/rf_amd_diag.h"
#include "rf_plan.h"
#include "rf_batch_plan.h"
#include "rf_set_plan.h"
#include "rf_launch.h"

using namespace rf;

static thread_local std::string g_err;
static int fail(int rc, const std::string& msg) {
  g_err = msg;
  return rc;
}
#define HIPCHK(x)                                                                     \
  do {                                                                                \
    hipError_t _e = (x);                                                              \
    if (_e != hipSuccess)                                                             \
      return fail(_e == hipErrorOutOfMemory ? RF_AMD_ENOMEM : RF_AMD_EINVAL,          \
                  std::string(#x) + ": " + hipGetErrorString(_e));                    \
  } while (0)

// Device allocations of an engine's batches are recycled through a pool: SplinterDB builds
// a new set of filters on every compaction, so in steady state rf_amd_batch_create finds
// its ~25 work buffers here instead of calling hipMalloc. Sizes are rounded up to classes
// of 1/8 of a power of two (at most 12.5 % slack); a block returns to the pool when its
// batch is destroyed unless the pool already holds RF_AMD_POOL_MIB MiB (default: a quarter
// of the device memory free at engine creation; rf_amd_engine_pool_trim
// hands blocks back).
// rf_amd_batch_destroy synchronises the device first; rf_amd_batch_destroy_on instead
// parks the blocks behind an event on the caller's stream (stream-ordered release, as
// hipFreeAsync): they become reusable once that event has completed.
// RF_AMD_POOL_TRACE=<ms>: diagnostics, every pool hipMalloc / hipFree slower than that
static uint64_t pool_trace_ns() {
  static const char* v = getenv("RF_AMD_POOL_TRACE");
  if (!v) return 0;
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}
static void pool_trace(const char* what, size_t bytes, uint64_t t0) {
  if (!t0) return;
  static const double lim = atof(getenv("RF_AMD_POOL_TRACE"));
  const double ms = (pool_trace_ns() - t0) * 1e-6;
  fprintf(stderr, "rf_amd pool: %s %zu B %.3f ms%s\n", what, bytes, ms, ms >= lim ? " SLOW" : "");
}

struct DevPool {
  std::mutex mu;
  std::multimap<size_t, void*> free_blocks;
  struct Parked {
    hipEvent_t ev;
    std::vector<std::pair<void*, size_t>> blocks;  // size 0: not pooled, hipFree when released
  };
  std::vector<Parked> parked;
  size_t pooled = 0, limit = 0;
  uint64_t hits = 0, misses = 0;
  static size_t size_class(size_t bytes) {
    if (bytes <= 4096) return 4096;
    const int lg = 63 - __builtin_clzll((unsigned long long)bytes);
    const size_t step = (size_t)1 << (lg - 3);
    return (bytes + step - 1) / step * step;
  }
  void give_locked(void* p, size_t cls) {
    if (cls == 0 || pooled + cls > limit) {
      const uint64_t t0 = pool_trace_ns();
      (void)hipFree(p);
      pool_trace("hipFree", cls, t0);
      return;
    }
    free_blocks.emplace(cls, p);
    pooled += cls;
  }
  // parked blocks whose event has completed (wait: every parked block) go to free_blocks
  void reap_locked(bool wait) {
    for (size_t i = 0; i < parked.size();) {
      Parked& k = parked[i];
      if (wait) (void)hipEventSynchronize(k.ev);
      if (!wait && hipEventQuery(k.ev) != hipSuccess) {
        i++;
        continue;
      }
      for (auto& b : k.blocks) give_locked(b.first, b.second);
      (void)hipEventDestroy(k.ev);
      parked[i] = std::move(parked.back());
      parked.pop_back();
    }
  }
  // best fit: the smallest pooled block of at least `*cls` bytes and at most twice that
  // (compaction rounds grow from one round to the next, so exact classes rarely recur within
  // a chain); *cls becomes the block's size
  void* take(size_t* cls) {
    std::lock_guard<std::mutex> g(mu);
    if (!parked.empty()) reap_locked(false);
    auto it = free_blocks.lower_bound(*cls);
    if (it == free_blocks.end() || it->first > 2 * *cls) {
      misses++;
      return nullptr;
    }
    void* p = it->second;
    *cls = it->first;
    free_blocks.erase(it);
    pooled -= *cls;
    hits++;
    return p;
  }
  bool give(void* p, size_t cls) {
    std::lock_guard<std::mutex> g(mu);
    if (pooled + cls > limit) return false;
    free_blocks.emplace(cls, p);
    pooled += cls;
    return true;
  }
  void park(Parked&& k) {
    std::lock_guard<std::mutex> g(mu);
    parked.push_back(std::move(k));
  }
  void drain() {
    std::lock_guard<std::mutex> g(mu);
    reap_locked(true);
    for (auto& kv : free_blocks) (void)hipFree(kv.second);
    free_blocks.clear();
    pooled = 0;
  }
};

// host-buffer entry points stage through these (rf_amd_batch_*_host): pinned host memory
// and a device buffer per engine, grown on demand, one caller at a time
struct HostStage {
  std::mutex mu;
  void* h = nullptr;
  void* d = nullptr;
  size_t cap = 0;
};

// A lookup channel of the host-buffer probe entry points (rf_amd_probe_filters_host and the
// forms built on it). Callers on different threads take different slots, so their round
// trips -- stream, pinned buffers, completion word -- run concurrently. A round trip is ONE
// kernel launch: the kernel reads the probes from `h` (pinned, device-mapped) or, for large
// calls, from `d` after one H2D copy, writes every result straight into `h`, and its last
// workgroup stores the call's sequence number into `flag`, which the host polls.
struct ProbeSlot {
  hipStream_t st = nullptr;
  uint8_t* h = nullptr;  // pinned coherent host memory: [hashes | groups ids | group table | results]
  size_t hcap = 0;
  uint8_t* d = nullptr;  // device copy of the inputs (copy mode)
  size_t dcap = 0;
  uint32_t* flag = nullptr;       // pinned coherent: the kernel's completion word
  uint32_t* d_counter = nullptr;  // device: workgroups finished (k_probe_groups)
  uint32_t seq = 0;
};

// The engine's lookup server (k_lookup_server): rings in pinned coherent host memory, the
// persistent kernel's generation and state, and the host-side bookkeeping of tickets.
// Submitting threads and the reaping thread run on different cores (often different CCDs of
// the host, where moving a written cache line costs ~300 ns), so the words each side writes
// sit on lines of their own: the submitters' ticket counter, the reaper's lock and cursor, and
// the read-mostly server state each get a 128-byte block (round 5 had them on one line, and a
// reaper spinning on its lock cost each submit several such transfers: 0.7 us per submit,
// profiles/r06_async_submit.txt).
struct LookupServer {
  std::once_flag once;
  int init_rc = 0;
  SrvReq* ring = nullptr;  // device memory the host writes through the BAR (or pinned host memory)
  bool ring_dev = false;
  SrvRes* res = nullptr;   // pinned coherent host memory
  SrvCtl* ctl = nullptr;
  hipStream_t st = nullptr;             // its own HSA queue (CU-masked), so it never blocks other work
  std::atomic<uint64_t> idle_ticks{0}, life_ticks{0};  // of the next launch (rf_amd_lookup_server_set_times)
  std::atomic<bool> ready{false};  // rings allocated and initialised (srv_init done)
  // read-mostly: written when a server is launched or fails
  alignas(128) std::atomic<uint64_t> state{0};  // generation << 1 | running
  std::atomic<uint64_t> launches{0};
  // sticky: the first error of the server (a launch that failed, a faulted stream). Every
  // waiter then returns it, submits fail at once, and rf_amd_lookup_server_failed hands the
  // unanswered tickets' tags back, so no caller spins on an answer that cannot come
  std::atomic<int> dead{0};
  // the submitters'
  alignas(128) std::atomic<uint64_t> tail{0};  // the next ticket
  // the reaper's
  alignas(128) std::mutex reap_mu;
  uint64_t reap_next = 0;                      // the next ticket reap() looks at (under reap_mu)
  std::atomic<uint64_t> reap_hint{0};          // reap_next, for the lock-free look of an idle reap
  std::atomic<uint64_t> last_check_ns{0};      // the reaper's last look at the server stream
  // per slot, host-only: the slot's ticket (published after the tag) and the submitter's tag
  // (NULL: a waiter's) -- read by rf_amd_lookup_server_failed (tags of tickets a dead server
  // never answered) and by the next submitter of the slot; the reaper reads answer lines only
  struct Meta {
    std::atomic<uint64_t> ticket{~0ull};
    void* tag = nullptr;
  };
  alignas(128) Meta meta[SRV_RING];
  std::atomic<uint64_t> consumed[SRV_RING];  // per slot: 1 + the last ticket whose result was taken
  // per slot: a ticket whose submitter gave up before publishing it (the server died while it
  // waited for the slot): the reap and failure cursors step over it instead of waiting on it
  std::atomic<uint64_t> abandoned[SRV_RING];
};

struct rf_amd_engine {
  int device;
  uint64_t uid = 0;  // unique per engine created in this process (per-thread caches key on it)
  LookupServer srv;
  // completion points on the engine stream (rf_amd_engine_fence): recycled events
  std::mutex fence_mu;
  std::vector<hipEvent_t> fence_free;
  // host ranges registered for direct image placement (rf_amd_host_register): host base,
  // bytes, device address of the base
  struct HostReg {
    uintptr_t h;
    uint64_t bytes;
    uintptr_t d;
  };
  std::mutex reg_mu;
  std::vector<HostReg> regs;
  hipStream_t stream;
  DevPool pool;
  HostStage stage;
  std::mutex slot_mu;
  std::vector<ProbeSlot*> slots_all, slots_free;
  // builds issued on `stream` (do_build) and the count last seen finished: a lookup slot
  // queries the engine stream only when a build may still be in flight (a HIP call less on
  // the lookup round trip)
  std::atomic<uint64_t> builds_issued{0}, builds_seen_idle{0};
};

struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  DevPool* pool = nullptr;
  ~DevBuf() { release(); }
  void release() {
    if (p && !(pool && pool->give(p, n))) (void)hipFree(p);
    p = nullptr;
  }
  int alloc(size_t bytes, DevPool* from = nullptr) {
    release();
    pool = from;
    n = from ? DevPool::size_class(bytes ? bytes : 16) : (bytes ? bytes : 16);
    if (from && (p = from->take(&n)) != nullptr) return 0;
    const uint64_t t0 = pool_trace_ns();
    hipError_t e = hipMalloc(&p, n);
    pool_trace("hipMalloc", n, t0);
    if (e != hipSuccess && from) {  // the pool may hold what this needs: give it back, retry
      from->drain();
      e = hipMalloc(&p, n);
    }
    if (e != hipSuccess) {
      p = nullptr;
      return fail(RF_AMD_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    return 0;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

// the stream of a call: the caller's, or the engine's own for NULL
static hipStream_t stream_of(const rf_amd_engine* e, void* stream) { return stream ? (hipStream_t)stream : e->stream; }

// a launcher's return value (rf_launch.h: 0 or a HIP error) as the call's
static int launch_rc(const char* what, int rc) {
  return rc ? fail(RF_AMD_EINVAL, std::string(what) + " launch: " + hipGetErrorString((hipError_t)rc)) : 0;
}

// Stream-ordered release: the live blocks of bufs[0..n) are parked behind an event recorded on
// `st` and return to the pool (a block of another origin: to hipFree) once it has completed; the
// buffers are left empty. Returns false, having touched no buffer, when the event could not be
// created or recorded: the caller then releases them its own way.
static bool park_behind(rf_amd_engine* e, hipStream_t st, DevBuf* const* bufs, size_t n) {
  DevPool::Parked k{};
  for (size_t i = 0; i < n; i++)
    if (bufs[i]->p) k.blocks.emplace_back(bufs[i]->p, bufs[i]->pool == &e->pool ? bufs[i]->n : 0);
  if (k.blocks.empty()) return true;
  hipError_t he = hipEventCreateWithFlags(&k.ev, hipEventDisableTiming);
  if (he == hipSuccess) he = hipEventRecord(k.ev, st);
  if (he != hipSuccess) {
    if (k.ev) (void)hipEventDestroy(k.ev);
    return false;
  }
  for (size_t i = 0; i < n; i++) {
    bufs[i]->p = nullptr;
    bufs[i]->n = 0;
  }
  e->pool.park(std::move(k));
  return true;
}

// every device buffer of a batch, named once: the members and bufs() (what destroy_on, trim and
// device_bytes walk) both come from this list
#define RF_BATCH_DEVBUFS(X)                                                                        \
  X(d_runs) X(d_wave_tab) /* probe run bounds (rf_amd_batch_probe_*_runs), their wave table */     \
  X(d_plans) X(d_outs) X(d_ent) X(d_part) X(d_sorted) X(d_cb_count) X(d_cb_start) X(d_cb_cursor)   \
  X(d_cb_filter) X(d_overflow) X(d_idx_cnt) X(d_idx_start) X(d_slots) X(d_page_first)              \
  X(d_pg_filter) X(d_pages) X(d_tile_filter) X(d_tile_start) X(d_old_tile_filter)                  \
  X(d_old_tile_start) X(d_old_cnt) X(d_old_pos) X(d_first_old) X(d_has_old) X(d_pplans) X(d_lines) \
  X(d_idx_filter) X(d_spill) X(d_old_idx_filter) X(d_old32) X(d_old_tot) X(d_ob_lo) X(d_ob_n)      \
  X(d_pg_noline) X(d_pre) X(d_cb_out) X(d_lay_wg) X(d_lay_hand)                                    \
  X(d_tile_value) X(d_tile_end) /* chained batches: each tile's run value and end */

// a batch is its plan (rf_batch_plan.h: geometry, totals, maps) plus the device buffers that
// plan asks for and the state of its builds
struct rf_amd_batch : BatchPlan {
  rf_amd_engine* eng = nullptr;
  rf_amd_config cfg{};
#define X(name) DevBuf name;
  RF_BATCH_DEVBUFS(X)
#undef X
  std::vector<uint64_t> runs_host;  // d_runs' last uploaded value
  // the sequence number that tags a build's K5 hand-offs (never 0: the words start out zero)
  uint32_t lay_seq = 0;
  bool counters_clean = false;  // the last build ran to its end and left the per-build counters zero (do_build)
  bool built = false;
  bool has_entries = false;  // built here: its sorted entries (d_part / d_sorted) are current
  std::vector<uint32_t> err_host;  // per-filter build error bits once read back (err_ready)
  std::atomic<bool> err_ready{false};
  std::mutex err_mu;
  hipEvent_t built_ev = nullptr;   // recorded after the last build's kernels (on the stream it ran on)
  std::vector<hipEvent_t> events;  // per-stage timing: ev_sets rings of NUM_EVENTS (rf_amd_batch_set_timing)
  uint32_t ev_sets = 0, ev_set = 0;  // each build starts the next set; probes record into the current one
  uint32_t ev_mask = EV_MASK_ALL;     // EV_MASK_PROBE: the probe's two events only
  ~rf_amd_batch() {
    if (built_ev) (void)hipEventDestroy(built_ev);
    for (auto ev : events) (void)hipEventDestroy(ev);
  }
  std::vector<DevBuf*> bufs() {
    return {
#define X(name) &name,
        RF_BATCH_DEVBUFS(X)
#undef X
    };
  }
};

// The environment switches of batch planning, read at every create and import (tests set them
// between batches of one process).
// RF_AMD_LAYOUT_SEG: indices per K5 workgroup, a power of two in [256, 4096] (default 4096;
// larger values mean 4096, 0 or anything else the one-workgroup kernel for every filter).
// RF_AMD_LINE_SIGMA: line_log_group's margin (tuning knob, default 3.5).
// RF_AMD_LINES_DENSE: 0 = no filter takes dense probe lines, anything else = every filter that
// has a dense geometry does; unset = those whose line table outgrows one XCD's L2.
// RF_AMD_DENSE_SIGMA: line_dense_group's margin (tuning knob, default 2.5).
// RF_AMD_WIDE64, RF_AMD_OLD_DECODE, RF_AMD_OLD_RESPLIT_OFF (set at all): incremental adds keep
// 64-bit entries / always decode old filters' images / decode them when the geometry changed.
static PlanKnobs plan_knobs_env() {
  PlanKnobs k;
  k.wide64 = getenv("RF_AMD_WIDE64") != nullptr;
  k.old_decode = getenv("RF_AMD_OLD_DECODE") != nullptr;
  k.old_resplit_off = getenv("RF_AMD_OLD_RESPLIT_OFF") != nullptr;
  if (const char* e = getenv("RF_AMD_LAYOUT_SEG"); e && *e) {
    const unsigned long v = strtoul(e, nullptr, 10);
    k.layout_seg = (v < LAYOUT_SEG_MIN || (v & (v - 1))) ? 0 : v > LAYOUT_SEG_MAX ? LAYOUT_SEG_MAX : (uint32_t)v;
  }
  if (const char* e = getenv("RF_AMD_LINE_SIGMA"); e && atof(e) > 0.0) k.line_sigma = atof(e);
  if (const char* e = getenv("RF_AMD_LINES_DENSE"); e && *e) k.lines_dense = e[0] == '0' ? 0 : 1;
  if (const char* e = getenv("RF_AMD_DENSE_SIGMA"); e && atof(e) > 0.0) k.dense_sigma = atof(e);
  return k;
}

extern "C" const char* rf_amd_last_error(void) { return g_err.c_str(); }

// filters whose probe lines were cut in the dense format, over every build and import of the
// process (rf_amd_diag_dense_line_filters)
static std::atomic<uint64_t> g_dense_line_filters{0};
template <typename Batch>
static void note_dense_lines(const Batch* b) {
  uint64_t n = 0;
  for (const FilterPlan& p : b->plans) n += line_is_dense(p.lg_line) ? 1 : 0;
  if (n) g_dense_line_filters.fetch_add(n, std::memory_order_relaxed);
}

// ---- engines alive at process exit ---------------------------------------------------------
// The compiler-generated constructor of this library registers its kernels with HIP when the
// library loads and registers, with atexit, the destructor that unregisters them again. An
// engine still alive at exit then has a lookup-server wave that may be running, pinned rings
// the GPU writes, host registrations and streams -- and the process's other threads (a
// drop-in's completion threads) may still be inside HIP calls -- while HIP tears the code
// objects down (a free() of an invalid pointer in __hipUnregisterFatBinary at the
// exit of the two-stack latency tool). Every engine alive at exit is therefore destroyed by a
// handler registered at the first engine creation, i.e. after the library's own destructor,
// so it runs before it (atexit order): server waves stopped, streams drained, pinned memory
// freed, registrations dropped. A drop-in that owns threads stops them in its own handler,
// registered after its engine's creation, so that one runs first (shim/routing_filter_amd.c).
static std::mutex g_live_mu;
static std::vector<rf_amd_engine*>* g_live = nullptr;  // never destroyed: read by the exit handler
static bool engine_quiesce(rf_amd_engine* e, int budget_ms);
static void engine_destroy_now(rf_amd_engine* e, bool device_sync);
static void engines_at_exit() {
  std::vector<rf_amd_engine*> v;
  {
    std::lock_guard<std::mutex> g(g_live_mu);
    if (g_live) v.swap(*g_live);
  }
  for (rf_amd_engine* e : v) {
    // a stream that does not drain in time (a hung kernel) leaves the engine as it is: exit
    // must not wait forever
    if (engine_quiesce(e, 2000)) engine_destroy_now(e, false);
  }
}

extern "C" int rf_amd_engine_create(int device, rf_amd_engine** out) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return fail(RF_AMD_ENODEV, "no HIP device: the routing-filter engine has no CPU fallback");
  if (device < 0 || device >= n) return fail(RF_AMD_EINVAL, "bad device ordinal");
  HIPCHK(hipSetDevice(device));
  auto* e = new rf_amd_engine();
  static std::atomic<uint64_t> next_uid{1};
  e->uid = next_uid.fetch_add(1);
  e->device = device;
  {
    // default: a quarter of the memory free at engine creation (~62 GB on an idle MI355X);
    // other allocators of the process can reclaim it with rf_amd_engine_pool_trim. The
    // compaction chain of 64 x 8M-fingerprint filters keeps 7.4 GB pooled beside the ~10 GB
    // its last round parks; a cap below that (round 5 had 16 GiB) makes every chain free and
    // re-allocate blocks of up to 2.7 GB, and hipFree of those costs ~28 ms per GB once the
    // driver clears released memory (profiles/r06_pool_churn.txt)
    const char* lim = getenv("RF_AMD_POOL_MIB");
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const size_t dflt = free_b / 4;
    e->pool.limit = lim ? (size_t)atoll(lim) << 20 : dflt;
  }
  // a BLOCKING stream: ordered with the legacy null stream that torch and most callers use
  if (hipStreamCreateWithFlags(&e->stream, hipStreamDefault) != hipSuccess) {
    delete e;
    return fail(RF_AMD_EINVAL, "hipStreamCreate failed");
  }
  {
    static std::once_flag at_exit_once;
    std::call_once(at_exit_once, [] { (void)atexit(engines_at_exit); });
    std::lock_guard<std::mutex> g(g_live_mu);
    if (!g_live) g_live = new std::vector<rf_amd_engine*>();
    g_live->push_back(e);
  }
  *out = e;
  return 0;
}

static void srv_stop(rf_amd_engine* e);
extern "C" void rf_amd_engine_destroy(rf_amd_engine* e) {
  if (!e) return;
  {
    std::lock_guard<std::mutex> g(g_live_mu);
    if (g_live) g_live->erase(std::remove(g_live->begin(), g_live->end(), e), g_live->end());
  }
  engine_destroy_now(e, true);
}

// device_sync false: the engine's own streams are known drained (engines_at_exit)
static void engine_destroy_now(rf_amd_engine* e, bool device_sync) {
  (void)hipSetDevice(e->device);
  srv_stop(e);
  if (device_sync) (void)hipDeviceSynchronize();
  (void)hipStreamDestroy(e->stream);
  for (ProbeSlot* s : e->slots_all) {
    if (s->st) (void)hipStreamDestroy(s->st);
    if (s->h) (void)hipHostFree(s->h);
    if (s->d) (void)hipFree(s->d);
    if (s->flag) (void)hipHostFree(s->flag);
    if (s->d_counter) (void)hipFree(s->d_counter);
    delete s;
  }
  e->pool.drain();
  for (hipEvent_t ev : e->fence_free) (void)hipEventDestroy(ev);
  for (const auto& r : e->regs) (void)hipHostUnregister((void*)r.h);
  if (e->stage.h) (void)hipHostFree(e->stage.h);
  if (e->stage.d) (void)hipFree(e->stage.d);
  delete e;
}

static int check_cfg(const rf_amd_config* cfg) {
  std::string msg;
  if (int rc = check_config(cfg, &msg)) return fail(rc, msg);
  return 0;
}

// what the planner needs to know of the old filters a batch names (empty: none)
static std::vector<OldFilter> old_filters_of(const rf_amd_engine* e, uint32_t F, rf_amd_batch* const* old_batch,
                                             const uint32_t* old_index) {
  std::vector<OldFilter> olds;
  if (!old_batch) return olds;
  olds.resize(F);
  for (uint32_t f = 0; f < F; f++) {
    const rf_amd_batch* ob = old_batch[f];
    if (!ob) continue;
    const uint32_t oi = old_index ? old_index[f] : 0;
    OldFilter& o = olds[f];
    o.present = true;
    o.plan = oi < ob->F ? &ob->plans[oi] : nullptr;
    o.fingerprint_size = ob->cfg.fingerprint_size;
    o.log_index_size = ob->cfg.log_index_size;
    o.has_entries = ob->has_entries;
    o.wide = ob->wide;
    o.built = ob->built;
    o.same_device = ob->eng->device == e->device;
  }
  return olds;
}

// batch_create, step 2: the device buffers the plan asks for
static int create_alloc(rf_amd_batch* b) {
  const size_t esz = (b->wide && !b->flag32) ? 8 : 4;
  const uint32_t P = b->cfg.page_size;
  int rc = 0;
  DevPool* pool = &b->eng->pool;
  const uint64_t ta0 = pool_trace_ns();
  rc |= b->d_plans.alloc(sizeof(FilterPlan) * b->F, pool);
  rc |= b->d_pplans.alloc(16ull * b->F, pool);
  rc |= b->d_outs.alloc(sizeof(FilterOut) * b->F, pool);
  rc |= b->d_ent.alloc(esz * b->E + 64, pool);
  rc |= b->d_part.alloc(esz * b->E + 64, pool);
  if (b->wide) rc |= b->d_sorted.alloc(4 * b->E + 64, pool);
  if (b->flag32) rc |= b->d_cb_out.alloc(4 * b->CB, pool);
  rc |= b->d_cb_count.alloc(4 * b->CB, pool);
  rc |= b->d_cb_start.alloc(4 * b->CB, pool);
  rc |= b->d_cb_cursor.alloc(4 * b->CB, pool);
  rc |= b->d_cb_filter.alloc(4 * b->CB, pool);
  rc |= b->d_overflow.alloc(4 * (b->CB + 1), pool);
  rc |= b->d_spill.alloc(8, pool);  // the spill flag, the folded K2's ticket
  rc |= b->d_idx_cnt.alloc(4 * b->I, pool);
  rc |= b->d_idx_start.alloc(4 * b->I, pool);
  rc |= b->d_slots.alloc(8 * b->I, pool);
  rc |= b->d_lines.alloc(64ull * b->NL + 64, pool);
  rc |= b->d_idx_filter.alloc(4ull * b->I, pool);
  rc |= b->d_page_first.alloc(4 * b->PF, pool);
  rc |= b->d_pg_filter.alloc(4 * b->PS, pool);
  rc |= b->d_pg_noline.alloc(4 * b->PS + 4, pool);
  rc |= b->d_pages.alloc((size_t)b->PS * P + 256, pool);
  rc |= b->d_tile_filter.alloc(4ull * b->num_tiles, pool);
  rc |= b->d_tile_start.alloc(4ull * b->num_tiles, pool);
  if (b->chained) {
    rc |= b->d_tile_value.alloc(4ull * b->num_tiles, pool);
    rc |= b->d_tile_end.alloc(4ull * b->num_tiles, pool);
  }
  rc |= b->d_old_tile_filter.alloc(4ull * b->num_old_tiles, pool);
  rc |= b->d_old_tile_start.alloc(4ull * b->num_old_tiles, pool);
  rc |= b->d_pre.alloc(4 * b->pre.size(), pool);
  if (b->lay_grid) {
    rc |= b->d_lay_wg.alloc(4ull * b->lay_grid, pool);
    rc |= b->d_lay_hand.alloc(16ull * b->lay_grid, pool);
  }
  if (b->wide || b->chained) {  // the num_unique quirk's per-index old entries (K4 -> K5)
    rc |= b->d_first_old.alloc(4 * b->I, pool);
    rc |= b->d_has_old.alloc(4 * b->I, pool);
  }
  if (b->wide) {
    rc |= b->d_old_cnt.alloc(4ull * b->num_old_idx, pool);
    rc |= b->d_old_pos.alloc(4ull * b->num_old_idx, pool);
    rc |= b->d_old_idx_filter.alloc(4ull * b->num_old_idx, pool);
    if (b->flag32) {
      rc |= b->d_old32.alloc(4 * b->old_total + 64, pool);
      rc |= b->d_old_tot.alloc(4 * b->F, pool);
      rc |= b->d_ob_lo.alloc(4 * b->CB, pool);
      rc |= b->d_ob_n.alloc(4 * b->CB, pool);
    }
  }
  pool_trace("create allocs", 0, ta0);
  return rc ? fail(RF_AMD_ENOMEM, "device allocation failed") : 0;
}

// batch_create, step 3a: where each filter's old filter lies on the device -- its image, and
// for those read in place (old_direct) its batch's sorted entries with their index runs
static void fill_old_pointers(rf_amd_batch* b, rf_amd_batch* const* old_batch, const uint32_t* old_index) {
  for (uint32_t f = 0; old_batch && f < b->F; f++) {
    const rf_amd_batch* ob = old_batch[f];
    if (!ob) continue;
    const FilterPlan* op = &ob->plans[old_index ? old_index[f] : 0];
    FilterPlan& p = b->plans[f];
    p.old_pages = ob->d_pages.as<uint8_t>() + (uint64_t)op->page_base * b->cfg.page_size;
    p.old_slots = ob->d_slots.as<uint64_t>() + op->idx_base;
    p.old_out = ob->d_outs.as<FilterOut>() + (old_index ? old_index[f] : 0);
    if (!p.old_direct) continue;
    const uint32_t* es = ob->wide ? ob->d_sorted.as<uint32_t>() : ob->d_part.as<uint32_t>();
    p.old_entries = es + op->e_first;
    p.old_idx_start = ob->d_idx_start.as<uint32_t>() + op->idx_base;
    p.old_idx_cnt = ob->d_idx_cnt.as<uint32_t>() + op->idx_base;
  }
}

// batch_create, steps 3b and 4: uploads, map fills, and the wait for them (the batch's host
// vectors may change once it is handed out). On failure work may still be queued.
static int create_enqueue(rf_amd_batch* b) {
  hipStream_t st = b->eng->stream;
  // Page bytes the reference never writes are zero on a fresh cache page (SURVEY finding 4).
  // K6 writes every byte of every page it assembles (block bytes and the zero tail), and no
  // reader looks past a filter's num_pages, so the reserved pages a build does not use are
  // not cleared (page_cap reserves ~2x the pages: clearing them cost a compaction round
  // ~0.3 ms); only the tail pad that windowed reads of the last page may touch is zeroed.
  HIPCHK(hipMemsetAsync(b->d_pages.as<uint8_t>() + (size_t)b->PS * b->cfg.page_size, 0, 256, st));
  if (const char* pz = getenv("RF_AMD_POISON")) {
    // test hook: fill every work buffer -- the page images included -- with a pattern, so
    // that a kernel reading memory it did not write in this build, or leaving page bytes
    // unwritten, cannot pass the parity tests
    const int v = atoi(pz) & 0xff;
    for (DevBuf* d : {&b->d_ent, &b->d_part, &b->d_sorted, &b->d_cb_start, &b->d_idx_cnt, &b->d_idx_start,
                      &b->d_slots, &b->d_lines, &b->d_page_first, &b->d_pages, &b->d_first_old, &b->d_has_old,
                      &b->d_old32, &b->d_old_tot, &b->d_ob_lo, &b->d_ob_n})
      if (d->p) HIPCHK(hipMemsetAsync(d->p, v, d->n, st));
  }
#define UP(buf, vec) \
  if (!(vec).empty()) HIPCHK(hipMemcpyAsync(buf.p, (vec).data(), sizeof((vec)[0]) * (vec).size(), hipMemcpyHostToDevice, st))
  UP(b->d_plans, b->plans);
  UP(b->d_pplans, b->pplans);
  UP(b->d_pre, b->pre);
  UP(b->d_lay_wg, b->lay_wg);
  UP(b->d_tile_filter, b->tile_filter);  // the tile maps of a chained batch
  UP(b->d_tile_start, b->tile_start);
  UP(b->d_tile_value, b->tile_value);
  UP(b->d_tile_end, b->tile_end);
#undef UP
  // hand-off tags start out zero, once per batch: a build's tag is never 0
  if (b->lay_grid) HIPCHK(hipMemsetAsync(b->d_lay_hand.p, 0, 16ull * b->lay_grid, st));
  {
    // element -> filter maps (and tile -> first key) from the prefix arrays, on the device
    const uint32_t F1 = b->F + 1;
    const uint32_t* dp = b->d_pre.as<uint32_t>();
    struct M { int k; DevBuf* fof; DevBuf* start; };
    const M maps[] = {{PRE_TILE, &b->d_tile_filter, &b->d_tile_start},
                      {PRE_OTILE, &b->d_old_tile_filter, &b->d_old_tile_start},
                      {PRE_CB, &b->d_cb_filter, nullptr},
                      {PRE_PG, &b->d_pg_filter, nullptr},
                      {PRE_IDX, &b->d_idx_filter, nullptr},
                      {PRE_OIDX, &b->d_old_idx_filter, nullptr}};
    for (const M& m : maps) {
      const uint32_t n = b->pre_of(m.k)[b->F];
      if (n == 0 || !m.fof->p) continue;
      if (b->chained && m.k == PRE_TILE) continue;  // uploaded above
      if (rf_launch_seg_fill(st, dp + (size_t)m.k * F1, b->F, n, m.fof->as<uint32_t>(),
                             m.start ? m.start->as<uint32_t>() : nullptr, TILE_KEYS))
        return fail(RF_AMD_EINVAL, "map fill launch failed");
    }
  }
  const uint64_t ts0 = pool_trace_ns();
  HIPCHK(hipStreamSynchronize(st));
  pool_trace("create sync", 0, ts0);
  return 0;
}

// rf_amd_batch_create, and rf_amd_batch_create_runs with num_runs != nullptr: filter f's new
// inputs are then num_runs[f] runs (run_len / run_value, filter-major) and num_new / value are
// not read. Four steps: check and plan (rf_batch_plan.h; nothing is allocated or launched
// before the arguments have been checked), allocate, fill in pointers and upload, launch and
// synchronise.
static int batch_create(rf_amd_engine* e, const rf_amd_config* cfg, uint32_t num_filters,
                        const uint32_t* num_new, const uint16_t* value, const uint32_t* num_runs,
                        const uint32_t* run_len, const uint16_t* run_value,
                        rf_amd_batch* const* old_batch, const uint32_t* old_index, rf_amd_batch** out) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (int rc = check_cfg(cfg)) return rc;
  if (num_filters == 0 || !(num_runs ? (run_len && run_value) : num_new != nullptr) || !out)
    return fail(RF_AMD_EINVAL, "empty batch");
  const std::vector<OldFilter> olds = old_filters_of(e, num_filters, old_batch, old_index);
  BatchInput in;
  in.cfg = cfg;
  in.num_filters = num_filters;
  in.num_new = num_new;
  in.value = value;
  in.num_runs = num_runs;
  in.run_len = run_len;
  in.run_value = run_value;
  in.olds = olds.empty() ? nullptr : olds.data();
  auto b = std::make_unique<rf_amd_batch>();
  std::string msg;
  if (int rc = plan_batch(in, plan_knobs_env(), b.get(), &msg)) return fail(rc, msg);
  b->eng = e;
  b->cfg = *cfg;

  HIPCHK(hipSetDevice(e->device));
  if (int rc = create_alloc(b.get())) return rc;

  fill_old_pointers(b.get(), old_batch, old_index);
  if (int rc = create_enqueue(b.get())) {
    // queued work may still read the batch's host vectors and write the blocks that go back
    // to the pool with it
    (void)hipStreamSynchronize(e->stream);
    return rc;
  }
  *out = b.release();
  return 0;
}

extern "C" int rf_amd_batch_create(rf_amd_engine* e, const rf_amd_config* cfg, uint32_t num_filters,
                                   const uint32_t* num_new, const uint16_t* value,
                                   rf_amd_batch* const* old_batch, const uint32_t* old_index,
                                   rf_amd_batch** out) {
  return batch_create(e, cfg, num_filters, num_new, value, nullptr, nullptr, nullptr, old_batch, old_index, out);
}

extern "C" int rf_amd_batch_create_runs(rf_amd_engine* e, const rf_amd_config* cfg, uint32_t num_filters,
                                        const uint32_t* num_runs, const uint32_t* run_len,
                                        const uint16_t* run_value, rf_amd_batch* const* old_batch,
                                        const uint32_t* old_index, rf_amd_batch** out) {
  if (!num_runs || !run_len || !run_value) return fail(RF_AMD_EINVAL, "null run arrays");
  // (one run per filter: the planner makes that exactly rf_amd_batch_create's batch)
  return batch_create(e, cfg, num_filters, nullptr, nullptr, num_runs, run_len, run_value, old_batch, old_index, out);
}

extern "C" void rf_amd_batch_destroy(rf_amd_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->eng->device);
  // work on a caller's stream may still read the batch: its blocks go back to the pool only
  // once the device is idle (what hipFree would have waited for)
  (void)hipDeviceSynchronize();
  delete b;
}

// stream-ordered destroy: every use of the batch is ordered before the current end of
// `stream`; its device blocks are parked behind an event recorded there and reused (or
// freed) once it completes. Returns without waiting.
extern "C" int rf_amd_batch_destroy_on(rf_amd_batch* b, void* stream) {
  if (!b) return 0;
  HIPCHK(hipSetDevice(b->eng->device));
  const std::vector<DevBuf*> bufs = b->bufs();
  if (park_behind(b->eng, stream_of(b->eng, stream), bufs.data(), bufs.size())) delete b;
  else rf_amd_batch_destroy(b);  // fall back to the synchronising destroy
  return 0;
}

// Drops a built batch's work buffers (entries, maps, counters), keeping what lookups, image
// reads, estimates and use as an old filter by image decode need: plans, outs, pages, slots,
// probe lines, index map, probe runs. Stream-ordered like rf_amd_batch_destroy_on. A trimmed
// batch no longer offers its entries in place to incremental adds (they decode its image).
extern "C" int rf_amd_batch_trim(rf_amd_batch* b, void* stream) {
  if (!b || !b->built) return fail(RF_AMD_EINVAL, "trim of an unbuilt batch");
  HIPCHK(hipSetDevice(b->eng->device));
  DevBuf* keep[] = {&b->d_plans, &b->d_pplans, &b->d_outs, &b->d_pages, &b->d_slots, &b->d_lines,
                    &b->d_idx_filter, &b->d_runs, &b->d_wave_tab};
  std::vector<DevBuf*> drop;
  for (DevBuf* d : b->bufs())
    if (d->p && std::find(std::begin(keep), std::end(keep), d) == std::end(keep)) drop.push_back(d);
  b->has_entries = false;
  hipStream_t st = stream_of(b->eng, stream);
  if (!park_behind(b->eng, st, drop.data(), drop.size())) {  // cannot order the release: wait, then release
    (void)hipStreamSynchronize(st);
    std::lock_guard<std::mutex> g(b->eng->pool.mu);
    for (DevBuf* d : drop) {
      b->eng->pool.give_locked(d->p, d->pool == &b->eng->pool ? d->n : 0);
      d->p = nullptr;
      d->n = 0;
    }
  }
  return 0;
}

// device bytes a batch holds (its buffers, pooled sizes)
extern "C" uint64_t rf_amd_batch_device_bytes(const rf_amd_batch* b) {
  if (!b) return 0;
  uint64_t s = 0;
  for (DevBuf* d : const_cast<rf_amd_batch*>(b)->bufs())
    if (d->p) s += d->n;
  return s;
}

// the engine's own stream (builds from host buffers, imports run there)
extern "C" void* rf_amd_engine_stream(rf_amd_engine* e) { return e ? (void*)e->stream : nullptr; }
extern "C" int rf_amd_engine_sync(rf_amd_engine* e) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

extern "C" int rf_amd_host_alloc(rf_amd_engine* e, uint64_t bytes, void** out) {
  if (!e || !out) return fail(RF_AMD_EINVAL, "null argument");
  HIPCHK(hipSetDevice(e->device));
  *out = nullptr;
  if (hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) {
    *out = nullptr;
    return fail(RF_AMD_ENOMEM, "hipHostMalloc failed");
  }
  return 0;
}

extern "C" void rf_amd_host_free(rf_amd_engine* e, void* p) {
  (void)e;
  if (p) (void)hipHostFree(p);
}

// a fence is an event recorded on the engine stream; its handle travels as a uint64
extern "C" int rf_amd_engine_fence(rf_amd_engine* e, uint64_t* fence) {
  if (!e || !fence) return fail(RF_AMD_EINVAL, "null argument");
  HIPCHK(hipSetDevice(e->device));
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> g(e->fence_mu);
    if (!e->fence_free.empty()) {
      ev = e->fence_free.back();
      e->fence_free.pop_back();
    }
  }
  if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIPCHK(hipEventRecord(ev, e->stream));
  *fence = (uint64_t)(uintptr_t)ev;
  return 0;
}

extern "C" int rf_amd_engine_fence_wait(rf_amd_engine* e, uint64_t fence) {
  if (!e || !fence) return fail(RF_AMD_EINVAL, "null argument");
  hipEvent_t ev = (hipEvent_t)(uintptr_t)fence;
  const hipError_t r = hipEventSynchronize(ev);
  {
    std::lock_guard<std::mutex> g(e->fence_mu);
    e->fence_free.push_back(ev);
  }
  if (r != hipSuccess) return fail(RF_AMD_EINVAL, std::string("fence: ") + hipGetErrorString(r));
  return 0;
}

static int batch_errors(rf_amd_batch* b);

extern "C" int rf_amd_host_register(rf_amd_engine* e, void* p, uint64_t bytes) {
  if (!e || !p || !bytes) return fail(RF_AMD_EINVAL, "null argument");
  HIPCHK(hipSetDevice(e->device));
  std::lock_guard<std::mutex> g(e->reg_mu);
  const uintptr_t h = (uintptr_t)p;
  for (const auto& r : e->regs)
    if (h < r.h + r.bytes && r.h < h + bytes) return fail(RF_AMD_EINVAL, "range overlaps a registered one");
  if (hipHostRegister(p, bytes, hipHostRegisterMapped) != hipSuccess) {
    (void)hipGetLastError();
    return fail(RF_AMD_ENOMEM, "hipHostRegister failed");
  }
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess || !d) {
    (void)hipHostUnregister(p);
    return fail(RF_AMD_EINVAL, "no device address for the registered range");
  }
  e->regs.push_back({h, bytes, (uintptr_t)d});
  return 0;
}

extern "C" int rf_amd_host_unregister(rf_amd_engine* e, void* p) {
  if (!e || !p) return fail(RF_AMD_EINVAL, "null argument");
  std::lock_guard<std::mutex> g(e->reg_mu);
  for (size_t i = 0; i < e->regs.size(); i++) {
    if (e->regs[i].h == (uintptr_t)p) {
      HIPCHK(hipSetDevice(e->device));
      (void)hipHostUnregister(p);
      e->regs.erase(e->regs.begin() + i);
      return 0;
    }
  }
  return fail(RF_AMD_EINVAL, "not a registered range");
}

// Filter f's image pages [first_page, first_page + count) (and, with_index, its index slots)
// written straight into host pages (D2H by the kernel's own stores, no staging copy): table (rf_amd_host_alloc'd, 2 * num_pages + ceil(num_indices /
// addrs_per_page) words) = the destination of each image page (host addresses inside a
// registered range), each page's disk address, and each index page's destination. The
// destinations are checked against the registered ranges and replaced in place by their
// device addresses; index slot i becomes disk_addr[slot / page_size] + slot % page_size,
// written at word i % addrs_per_page of index page i / addrs_per_page (src/routing_filter.c
// :612-620). Stream-ordered; the caller waits (rf_amd_engine_fence) before using the pages.
extern "C" int rf_amd_batch_place_image(rf_amd_batch* b, uint32_t f, uint64_t* table, uint32_t num_pages,
                                        uint32_t first_page, uint32_t count, int with_index,
                                        uint32_t addrs_per_page, void* stream) {
  if (!b || f >= b->F || !table || !addrs_per_page) return fail(RF_AMD_EINVAL, "bad argument");
  if (int rc = batch_errors(b)) return rc;
  if (b->err_host[f]) return fail(RF_AMD_EINVAL, "the filter's build failed");
  const FilterPlan& p = b->plans[f];
  const uint32_t P = b->cfg.page_size;
  if (num_pages > p.page_cap || first_page > num_pages || count > num_pages - first_page)
    return fail(RF_AMD_EINVAL, "pages outside the filter's reservation");
  const uint32_t nidx = with_index ? p.num_indices : 0u, nip = (nidx + addrs_per_page - 1) / addrs_per_page;
  if ((uint64_t)addrs_per_page * 8 > P) return fail(RF_AMD_EINVAL, "index page overflow");
  rf_amd_engine* e = b->eng;
  {
    std::lock_guard<std::mutex> g(e->reg_mu);
    size_t hint = 0;
    auto xlate = [&](uint64_t& w, uint64_t len) -> bool {
      const uintptr_t h = (uintptr_t)w;
      for (size_t k = 0; k < e->regs.size(); k++) {
        const auto& r = e->regs[(hint + k) % e->regs.size()];
        if (h >= r.h && h + len <= r.h + r.bytes) {
          hint = (hint + k) % e->regs.size();
          w = r.d + (h - r.h);
          return true;
        }
      }
      return false;
    };
    // a refused call leaves the table as it was: check every destination, then translate
    for (uint32_t k = first_page; k < first_page + count; k++) {
      uint64_t w = table[k];
      if (!xlate(w, P)) return fail(RF_AMD_EINVAL, "page destination outside the registered ranges");
    }
    for (uint32_t k = 0; k < nip; k++) {
      uint64_t w = table[2ull * num_pages + k];
      if (!xlate(w, P)) return fail(RF_AMD_EINVAL, "index page outside the registered ranges");
    }
    for (uint32_t k = first_page; k < first_page + count; k++) (void)xlate(table[k], P);
    for (uint32_t k = 0; k < nip; k++) (void)xlate(table[2ull * num_pages + k], P);
  }
  void* dt = nullptr;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipHostGetDevicePointer(&dt, table, 0));
  return launch_rc("place", rf_launch_place(stream_of(e, stream), b->d_pages.as<uint8_t>() + (uint64_t)p.page_base * P,
                                            b->d_slots.as<uint64_t>() + p.idx_base, first_page, count, num_pages,
                                            nidx, P, (const uint64_t*)dt, addrs_per_page));
}

extern "C" int rf_amd_engine_pool_stats(rf_amd_engine* e, uint64_t* pooled_bytes, uint64_t* hits, uint64_t* misses) {
  if (!e) return fail(RF_AMD_EINVAL, "null engine");
  std::lock_guard<std::mutex> g(e->pool.mu);
  if (pooled_bytes) *pooled_bytes = e->pool.pooled;
  if (hits) *hits = e->pool.hits;
  if (misses) *misses = e->pool.misses;
  return 0;
}

// hands pooled device blocks back to the device until at most keep_bytes stay pooled (blocks
// parked behind stream events are released once those complete)
extern "C" int rf_amd_engine_pool_trim(rf_amd_engine* e, uint64_t keep_bytes) {
  if (!e) return fail(RF_AMD_EINVAL, "null engine");
  HIPCHK(hipSetDevice(e->device));
  std::lock_guard<std::mutex> g(e->pool.mu);
  e->pool.reap_locked(false);
  for (auto it = e->pool.free_blocks.begin(); it != e->pool.free_blocks.end() && e->pool.pooled > keep_bytes;) {
    (void)hipFree(it->second);
    e->pool.pooled -= it->first;
    it = e->pool.free_blocks.erase(it);
  }
  return 0;
}

// the most device memory the pool keeps parked for reuse (RF_AMD_POOL_MIB at creation), trimmed
// to it now
extern "C" int rf_amd_engine_set_pool_limit(rf_amd_engine* e, uint64_t bytes) {
  if (!e) return fail(RF_AMD_EINVAL, "null engine");
  {
    std::lock_guard<std::mutex> g(e->pool.mu);
    e->pool.limit = bytes;
  }
  return rf_amd_engine_pool_trim(e, bytes);
}

extern "C" uint32_t rf_amd_batch_num_filters(const rf_amd_batch* b) { return b ? b->F : 0; }

static LaunchArgs make_args(rf_amd_batch* b, hipStream_t st) {
  LaunchArgs a;
  memset(&a, 0, sizeof(a));
  a.stream = st;
  a.wide = b->wide;
  a.plans = b->d_plans.as<FilterPlan>();
  a.pplans = b->d_pplans.as<uint4>();
  a.pplans_mut = b->d_pplans.as<uint4>();
  a.num_filters = b->F;
  a.tile_filter = b->d_tile_filter.as<uint32_t>();
  a.tile_start = b->d_tile_start.as<uint32_t>();
  a.num_tiles = b->num_tiles;
  a.tile_value = b->chained ? b->d_tile_value.as<uint32_t>() : nullptr;
  a.tile_end = b->chained ? b->d_tile_end.as<uint32_t>() : nullptr;
  a.old_tile_filter = b->d_old_tile_filter.as<uint32_t>();
  a.old_tile_start = b->d_old_tile_start.as<uint32_t>();
  a.num_old_tiles = b->num_old_tiles;
  a.old_idx_filter = b->d_old_idx_filter.as<uint32_t>();
  a.num_old_idx = b->num_old_idx;
  a.old_cnt = b->d_old_cnt.as<uint32_t>();
  a.old_pos = b->d_old_pos.as<uint32_t>();
  a.flag32 = b->flag32 ? 1u : 0u;
  a.old32 = b->d_old32.as<uint32_t>();
  a.old_tot = b->d_old_tot.as<uint32_t>();
  a.ob_lo = b->d_ob_lo.as<uint32_t>();
  a.ob_n = b->d_ob_n.as<uint32_t>();
  a.fp_size = b->cfg.fingerprint_size;
  a.seed = b->cfg.seed;
  a.lis = b->cfg.log_index_size;
  a.page_size = b->cfg.page_size;
  a.ent = b->d_ent.p;
  a.part = b->d_part.p;
  a.sorted32 = b->wide ? b->d_sorted.as<uint32_t>() : b->d_part.as<uint32_t>();
  a.cb_count = b->d_cb_count.as<uint32_t>();
  a.cb_start = b->d_cb_start.as<uint32_t>();
  a.cb_cursor = b->d_cb_cursor.as<uint32_t>();
  a.cb_filter = b->d_cb_filter.as<uint32_t>();
  a.num_cb = b->CB;
  a.overflow = b->d_overflow.as<uint32_t>();
  a.spill = b->d_spill.p ? b->d_spill.as<uint32_t>() : nullptr;
  a.cb_outs = b->d_cb_out.p ? b->d_cb_out.as<uint32_t>() : nullptr;
  a.idx_cnt = b->d_idx_cnt.as<uint32_t>();
  a.idx_start = b->d_idx_start.as<uint32_t>();
  a.first_old = b->d_first_old.as<uint32_t>();
  a.has_old = b->d_has_old.as<uint32_t>();
  a.slots = b->d_slots.as<uint64_t>();
  a.lines = b->d_lines.as<uint4>();
  a.line_lmax = b->line_lmax;
  a.lines_dense = b->lines_dense ? 1u : 0u;
  a.plines_needed = b->plines_needed ? 1u : 0u;
  a.pg_noline = b->d_pg_noline.as<uint32_t>();
  a.idx_filter = b->d_idx_filter.as<uint32_t>();
  a.num_idx = b->I;
  a.page_first = b->d_page_first.as<uint32_t>();
  a.pg_filter = b->d_pg_filter.as<uint32_t>();
  a.num_page_slots = b->PS;
  a.pages = b->d_pages.as<uint8_t>();
  a.outs = b->d_outs.p ? b->d_outs.as<FilterOut>() : nullptr;
  a.lay_wg = b->d_lay_wg.as<uint32_t>();
  a.lay_grid = b->d_lay_wg.p && b->d_lay_hand.p ? b->lay_grid : 0;
  a.lay_hand = b->d_lay_hand.as<uint64_t>();
  a.lay_seq = b->lay_seq;
  a.lay_seg = b->lay_seg;
  a.lay_whole = b->lay_whole ? 1u : 0u;
  a.k4_bitmap = b->k4_bitmap ? 1u : 0u;
  a.k4_pack = b->k4_pack ? 1u : 0u;
  a.events = b->events.empty() ? nullptr : reinterpret_cast<void**>(b->events.data() + (size_t)b->ev_set * NUM_EVENTS);
  a.ev_mask = b->ev_mask;
  return a;
}

static int do_probe(rf_amd_batch* b, int kind, const void* in0, const uint64_t* offs, uint32_t key_len,
                    const uint32_t* fid, uint64_t n, uint64_t* found, void* stream,
                    const uint64_t* d_runs = nullptr);

// The build's completion point: host reads of the batch (info, images) wait for this event
// and then copy on the engine stream -- never a device-wide synchronisation or a null-stream
// copy, which would also wait for the lookup server's wave
static int note_built(rf_amd_batch* b, hipStream_t st) {
  if (!b->built_ev) HIPCHK(hipEventCreateWithFlags(&b->built_ev, hipEventDisableTiming));
  HIPCHK(hipEventRecord(b->built_ev, st));
  return 0;
}
static int wait_built(rf_amd_batch* b) {
  if (b->built_ev) HIPCHK(hipEventSynchronize(b->built_ev));
  return 0;
}

static int do_build(rf_amd_batch* b, int kind, const void* in0, const uint64_t* offs, uint32_t key_len,
                    void* stream) {
  if (!b) return fail(RF_AMD_EINVAL, "null batch");
  if (b->keys_total && !in0) return fail(RF_AMD_EINVAL, "null input");
  HIPCHK(hipSetDevice(b->eng->device));
  hipStream_t st = stream_of(b->eng, stream);
  (void)hipGetLastError();  // launch checks below must see only their own errors
  if (b->ev_sets) b->ev_set = (b->ev_set + 1) % b->ev_sets;
  if (++b->lay_seq == 0) b->lay_seq = 1;
  LaunchArgs a = make_args(b, st);
  a.kind = kind;
  a.in0 = in0;
  a.offs = offs;
  a.key_len = key_len;
  if (a.events && (a.ev_mask >> EV_B_START & 1u)) HIPCHK(hipEventRecord(((hipEvent_t*)a.events)[EV_B_START], st));
  // A fresh build's last kernels leave the per-build counters zero (K5, BuildClean) and its
  // gated K1 zeroes `outs`, so the init launch runs only for a batch's first build and after
  // a build whose launches did not all go out. Incremental builds, batches whose probe lines
  // come from k_plines_list (its page count is read after K5) and the hand-back diagnostics
  // (read after the build) keep the init launch every time. RF_AMD_SELF_CLEAN=0: always init.
  const char* sc = getenv("RF_AMD_SELF_CLEAN");
  a.self_clean = (!b->wide && !b->plines_needed && b->num_tiles && !(sc && sc[0] == '0') &&
                  !getenv("RF_AMD_DIAG_OVERFLOW")) ? 1u : 0u;
  a.zero_outs = (a.self_clean && b->counters_clean) ? 1u : 0u;
  b->counters_clean = false;
  if (!a.zero_outs &&
      rf_launch_build_init(st, b->d_cb_count.as<uint32_t>(), (b->wide && !b->flag32) ? nullptr : b->d_cb_cursor.as<uint32_t>(),
                           b->CB, b->d_outs.as<uint32_t>(), (uint32_t)(sizeof(FilterOut) / 4 * b->F),
                           b->d_overflow.as<uint32_t>(), (b->wide && !b->flag32) ? nullptr : b->d_spill.as<uint32_t>(),
                           b->d_pg_noline.as<uint32_t>()))
    return fail(RF_AMD_EINVAL, "init kernel launch failed");
  if (b->wide) {
    // every old filter of the batch decoded by one launch sequence (which also marks the
    // unused tail of each old region); the new regions are written whole by the hashing pass
    if (int rc = launch_rc("old decode", rf_launch_old_decode(&a))) return rc;
  }
  b->err_ready.store(false, std::memory_order_release);  // a rebuild: read the new bits back
  note_dense_lines(b);
  int rc = rf_launch_build(&a);
  // counted once every kernel of the build is queued: a lookup that finds the stream idle
  // after reading this count cannot miss a build it covers
  if (st == b->eng->stream) b->eng->builds_issued.fetch_add(1, std::memory_order_acq_rel);
  if (rc) return launch_rc("build", rc);
  b->counters_clean = a.self_clean != 0;  // every launch of the build went out
  if (getenv("RF_AMD_DIAG_OVERFLOW") && b->d_overflow.p) {  // diagnostics: coarse buckets handed back by K4/K4m
    uint32_t nov = 0;
    if (hipMemcpyAsync(&nov, b->d_overflow.p, 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
        hipStreamSynchronize(st) == hipSuccess)
      fprintf(stderr, "rf_amd: %u of %u coarse buckets handed back (K4b / list mode)\n", nov, b->CB);
  }
  if (int erc = note_built(b, st)) return erc;
  b->built = true;
  // a packed build leaves index-block bodies in d_part, not sorted entries (unless it spilled,
  // which the host cannot know): a later add onto this batch decodes its image
  b->has_entries = !rf_build_packs(&a);
  return 0;
}

extern "C" int rf_amd_batch_build_keys(rf_amd_batch* b, const void* d_keys, uint32_t key_len, void* stream) {
  if (key_len == 0) return fail(RF_AMD_EINVAL, "key_len 0");
  return do_build(b, fixed_kind(d_keys, key_len), d_keys, nullptr, key_len, stream);
}
extern "C" int rf_amd_batch_build_var_keys(rf_amd_batch* b, const uint8_t* d_bytes, const uint64_t* d_offsets,
                                           void* stream) {
  if (!d_offsets) return fail(RF_AMD_EINVAL, "null offsets");
  return do_build(b, IN_VAR, d_bytes, d_offsets, 0, stream);
}
extern "C" int rf_amd_batch_build_hashes(rf_amd_batch* b, const uint32_t* d_hashes, void* stream) {
  return do_build(b, IN_HASH, d_hashes, nullptr, 4, stream);
}

// the engine's host staging area, grown to `bytes`; the caller holds e->stage.mu
static int stage_reserve(rf_amd_engine* e, size_t bytes) {
  HostStage& s = e->stage;
  if (s.cap >= bytes) return 0;
  if (s.h) (void)hipHostFree(s.h);
  if (s.d) (void)hipFree(s.d);
  s.h = s.d = nullptr;
  s.cap = 0;
  const size_t c = std::max<size_t>(bytes, (size_t)1 << 20);
  if (hipHostMalloc(&s.h, c, hipHostMallocDefault) != hipSuccess) {
    s.h = nullptr;
    return fail(RF_AMD_ENOMEM, "pinned staging allocation failed");
  }
  if (hipMalloc(&s.d, c) != hipSuccess) {
    (void)hipHostFree(s.h);
    s.h = nullptr;
    return fail(RF_AMD_ENOMEM, "device staging allocation failed");
  }
  s.cap = c;
  return 0;
}

// Host-buffer forms for callers that hold no device memory (the routing_filter.h shim,
// shim/routing_filter_amd.c): inputs are staged through the engine's pinned buffer on the
// engine stream, and the call returns once the results are complete.
// Two-step form of rf_amd_batch_build_hashes_host for callers that fill the staging buffer
// themselves, e.g. from several threads at once (the shim's coalesced adds: each adding
// thread copies its own fingerprints): stage_begin takes the engine's pinned staging buffer,
// sized for the batch's keys_total hashes (filter f's at its run offset), and returns it;
// stage_build uploads it, builds, waits, and releases the buffer. Every stage_begin must be
// followed by one stage_build (or stage_abort) on the same batch.
extern "C" int rf_amd_batch_stage_begin(rf_amd_batch* b, uint32_t** h_stage) {
  if (!b || !h_stage) return fail(RF_AMD_EINVAL, "null batch / out-param");
  rf_amd_engine* e = b->eng;
  HIPCHK(hipSetDevice(e->device));
  e->stage.mu.lock();
  if (int rc = stage_reserve(e, 4ull * b->keys_total + 16)) {
    e->stage.mu.unlock();
    return rc;
  }
  *h_stage = static_cast<uint32_t*>(e->stage.h);
  return 0;
}

extern "C" int rf_amd_batch_stage_build(rf_amd_batch* b) {
  rf_amd_engine* e = b->eng;
  std::lock_guard<std::mutex> g(e->stage.mu, std::adopt_lock);  // taken by stage_begin
  const size_t bytes = 4ull * b->keys_total;
  if (bytes) HIPCHK(hipMemcpyAsync(e->stage.d, e->stage.h, bytes, hipMemcpyHostToDevice, e->stream));
  if (int rc = do_build(b, IN_HASH, e->stage.d, nullptr, 4, e->stream)) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

extern "C" void rf_amd_batch_stage_abort(rf_amd_batch* b) {
  if (b) b->eng->stage.mu.unlock();
}

extern "C" int rf_amd_batch_build_hashes_host(rf_amd_batch* b, const uint32_t* h_hashes) {
  if (!b) return fail(RF_AMD_EINVAL, "null batch");
  if (b->keys_total && !h_hashes) return fail(RF_AMD_EINVAL, "null hashes");
  rf_amd_engine* e = b->eng;
  HIPCHK(hipSetDevice(e->device));
  std::lock_guard<std::mutex> g(e->stage.mu);
  const size_t bytes = 4ull * b->keys_total;
  if (int rc = stage_reserve(e, bytes + 16)) return rc;
  if (bytes) {
    memcpy(e->stage.h, h_hashes, bytes);
    HIPCHK(hipMemcpyAsync(e->stage.d, e->stage.h, bytes, hipMemcpyHostToDevice, e->stream));
  }
  if (int rc = do_build(b, IN_HASH, e->stage.d, nullptr, 4, e->stream)) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// ---- host-buffer lookups over the engine's lookup slots (ProbeSlot) -----------------------
static ProbeSlot* slot_take(rf_amd_engine* e) {
  {
    std::lock_guard<std::mutex> g(e->slot_mu);
    if (!e->slots_free.empty()) {
      ProbeSlot* s = e->slots_free.back();
      e->slots_free.pop_back();
      return s;
    }
  }
  auto* s = new ProbeSlot();
  // non-blocking: a lookup does not wait for unrelated work on the legacy null stream
  bool ok = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) == hipSuccess &&
            hipHostMalloc((void**)&s->flag, 64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess &&
            hipMalloc((void**)&s->d_counter, 64) == hipSuccess &&
            hipMemsetAsync(s->d_counter, 0, 64, s->st) == hipSuccess && hipStreamSynchronize(s->st) == hipSuccess;
  if (!ok) {
    if (s->st) (void)hipStreamDestroy(s->st);
    if (s->flag) (void)hipHostFree(s->flag);
    if (s->d_counter) (void)hipFree(s->d_counter);
    delete s;
    fail(RF_AMD_ENOMEM, "lookup slot allocation failed");
    return nullptr;
  }
  *s->flag = 0;
  std::lock_guard<std::mutex> g(e->slot_mu);
  e->slots_all.push_back(s);
  return s;
}

static void slot_give(rf_amd_engine* e, ProbeSlot* s) {
  std::lock_guard<std::mutex> g(e->slot_mu);
  e->slots_free.push_back(s);
}

static int slot_reserve(ProbeSlot* s, size_t hbytes, size_t dbytes) {
  if (s->hcap < hbytes) {
    if (s->h) (void)hipHostFree(s->h);
    s->h = nullptr;
    s->hcap = 0;
    const size_t c = std::max<size_t>(hbytes, (size_t)1 << 16);
    if (hipHostMalloc((void**)&s->h, c, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
      s->h = nullptr;
      return fail(RF_AMD_ENOMEM, "pinned lookup buffer allocation failed");
    }
    s->hcap = c;
  }
  if (dbytes && s->dcap < dbytes) {
    if (s->d) (void)hipFree(s->d);
    s->d = nullptr;
    s->dcap = 0;
    const size_t c = std::max<size_t>(dbytes, (size_t)1 << 20);
    if (hipMalloc((void**)&s->d, c) != hipSuccess) {
      s->d = nullptr;
      return fail(RF_AMD_ENOMEM, "device lookup buffer allocation failed");
    }
    s->dcap = c;
  }
  return 0;
}

// per-filter build error bits of a built batch, read back once (a batch is immutable once
// built; a filter whose build failed finds nothing, as k_probe does through pplans.w)
static int batch_errors(rf_amd_batch* b) {
  // concurrent lookups of one batch may both get here first (rf_amd.h: host lookups are
  // thread-safe): the read-back happens once, under the batch's lock, and err_host is
  // published (err_ready) only once filled
  if (b->err_ready.load(std::memory_order_acquire)) return 0;
  std::lock_guard<std::mutex> lk(b->err_mu);
  if (b->err_ready.load(std::memory_order_relaxed)) return 0;
  std::vector<FilterOut> o(b->F);
  HIPCHK(hipMemcpyAsync(o.data(), b->d_outs.p, sizeof(FilterOut) * b->F, hipMemcpyDeviceToHost, b->eng->stream));
  HIPCHK(hipStreamSynchronize(b->eng->stream));
  b->err_host.resize(b->F);
  for (uint32_t f = 0; f < b->F; f++) b->err_host[f] = o[f].error;
  b->err_ready.store(true, std::memory_order_release);
  return 0;
}

// filter f's entry of a group table, with the error bits `err`
static ProbeGroup probe_group_with(const rf_amd_batch* b, uint32_t f, uint32_t err) {
  const FilterPlan& p = b->plans[f];
  ProbeGroup g;
  g.x = pplan_word(p);
  g.err = err;
  g.fpl = b->cfg.fingerprint_size | (b->cfg.log_index_size << 8);
  g.pad = 0;
  g.lines = b->d_lines.as<uint4>() + 4ull * p.line_base;
  g.pages = b->d_pages.as<uint8_t>() + (uint64_t)p.page_base * b->cfg.page_size;
  g.slots = b->d_slots.as<uint64_t>() + p.idx_base;
  return g;
}
// the same with the build's own bits (after batch_errors)
static ProbeGroup probe_group_of(const rf_amd_batch* b, uint32_t f) { return probe_group_with(b, f, b->err_host[f]); }

// Probe modes of a round trip: inputs read by the kernel from pinned host memory (small
// calls: no copy command) or copied to the device with one H2D first; results always written
// by the kernel into pinned host memory; completion by polling the slot's flag word (or, with
// RF_AMD_PROBE_WAIT=sync, hipStreamSynchronize). RF_AMD_PROBE_MODE=mapped|copy forces a mode.
static int env_mode(const char* name, const char* a, const char* b) {
  const char* v = getenv(name);
  if (!v) return 0;
  return !strcmp(v, a) ? 1 : (!strcmp(v, b) ? 2 : 0);
}
// measured on MI355X (profiles/r03_probe_latency.txt): reading the inputs over PCIe from the
// kernel beats one H2D copy first up to at least 8,192 probes (17.7 vs 34.9 us per round trip)
static const uint64_t MAPPED_MAX_PROBES = 32768;

// The common body: n probes, probe i in group h_group[i] (NULL: group 0) of the ng-entry group
// table, results into h_found. Waits for any work still queued on the engine stream (builds
// issued there), then runs on a lookup slot of its own.
// waits for a slot's kernel to publish `seq` (or fails if the stream errored without it)
static int slot_wait(ProbeSlot* s, uint32_t seq, bool sync) {
  if (sync) {
    HIPCHK(hipStreamSynchronize(s->st));
    return 0;
  }
  for (uint32_t spin = 1;; spin++) {
    if (__atomic_load_n(s->flag, __ATOMIC_ACQUIRE) == seq) return 0;
    __builtin_ia32_pause();
    if ((spin & 4095) == 0) {  // a kernel that faulted never stores the flag
      const hipError_t q = hipStreamQuery(s->st);
      if (q == hipErrorNotReady) continue;
      if (q != hipSuccess) return fail(RF_AMD_EINVAL, std::string("probe kernel: ") + hipGetErrorString(q));
      if (__atomic_load_n(s->flag, __ATOMIC_ACQUIRE) != seq)
        return fail(RF_AMD_EINVAL, "probe kernel finished without its completion flag");
      return 0;
    }
  }
}

// ---- the lookup server (host side) --------------------------------------------------------
static const uint64_t SRV_UNPUBLISHED = ~0ull, SRV_BUSY = ~0ull - 1;
static_assert(SRV_RING == RF_AMD_SERVER_RING, "rf_amd.h and the kernels agree on the ring size");

// the host's stop word, after the request ring (the wave polls it with the requests)
static inline volatile uint64_t* srv_stop_word(SrvReq* ring) { return reinterpret_cast<volatile uint64_t*>(ring + SRV_RING); }
static void srv_set_stop(LookupServer& v) {
  if (!v.ring) return;
  *srv_stop_word(v.ring) = 1;
  _mm_sfence();  // out of the write-combining buffer now
}
// answer of ticket t in its slot: 1 = all four words carry t's check (found/tag filled in),
// -1 = the slot holds a later ticket's answer (a waiter took t and the slot moved on), 0 = not yet
static inline int srv_answer(const SrvRes* r, uint64_t t, uint64_t* found, uint64_t* tag) {
  const uint32_t c = srv_check(t);
  uint64_t w[4];
  for (int k = 0; k < 4; k++) w[k] = __atomic_load_n(&r->w[k], __ATOMIC_ACQUIRE);
  const uint32_t c0 = (uint32_t)(w[0] >> 32);
  if (c0 != c) return (c0 != 0 && (int32_t)(c0 - c) > 0) ? -1 : 0;
  for (int k = 1; k < 4; k++)
    if ((uint32_t)(w[k] >> 32) != c) return 0;  // still arriving
  if (found) *found = (w[0] & 0xffffffffull) | (w[1] << 32);
  if (tag) *tag = (w[2] & 0xffffffffull) | (w[3] << 32);
  return 1;
}
// RF_AMD_SRV_RING=host puts the request ring in pinned host memory (the round-6 layout's
// placement); default: fine-grained device memory, written by the host through the BAR
static bool srv_ring_on_device() {
  const char* s = getenv("RF_AMD_SRV_RING");
  return !(s && !strcmp(s, "host"));
}

static int srv_init(rf_amd_engine* e) {
  LookupServer& v = e->srv;
  // once initialised, one load (std::call_once's own fast path measured ~900 TSC cycles per
  // submit, profiles/r06_async_submit.txt)
  if (v.ready.load(std::memory_order_acquire)) return 0;
  std::call_once(v.once, [&] {
    const size_t ring_bytes = sizeof(SrvReq) * SRV_RING + 128;  // + the stop word's line
    if (hipSetDevice(e->device) != hipSuccess) {
      v.init_rc = RF_AMD_ENOMEM;
      return;
    }
    v.ring_dev = srv_ring_on_device() &&
                 hipExtMallocWithFlags((void**)&v.ring, ring_bytes, hipDeviceMallocFinegrained) == hipSuccess;
    if (v.ring_dev) {
      // the host writes it through its mapping of device memory: zero it there, then check on
      // the device that a host store landed (a box whose BAR does not reach it falls back)
      if (hipMemset(v.ring, 0, ring_bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) {
        (void)hipFree(v.ring);
        v.ring = nullptr;
        v.ring_dev = false;
      } else {
        volatile uint64_t* w = &v.ring[SRV_RING - 1].w[SRV_REQ_WORDS - 1];
        *w = 0x5EEDF00Dull;
        _mm_sfence();
        uint64_t back = 0;
        const bool ok = hipMemcpy(&back, (const void*)w, 8, hipMemcpyDeviceToHost) == hipSuccess && back == 0x5EEDF00Dull;
        *w = 0;
        _mm_sfence();
        if (!ok) {
          (void)hipFree(v.ring);
          v.ring = nullptr;
          v.ring_dev = false;
        }
      }
    }
    if (!v.ring_dev) {
      if (hipHostMalloc((void**)&v.ring, ring_bytes, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
        v.ring = nullptr;
        v.init_rc = RF_AMD_ENOMEM;
        return;
      }
      memset((void*)v.ring, 0, ring_bytes);
    }
    if (hipHostMalloc((void**)&v.res, sizeof(SrvRes) * SRV_RING, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
        hipHostMalloc((void**)&v.ctl, sizeof(SrvCtl), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
      v.init_rc = RF_AMD_ENOMEM;
      return;
    }
    memset(v.res, 0, sizeof(SrvRes) * SRV_RING);  // check 0: no answer yet
    for (uint32_t s = 0; s < SRV_RING; s++) {
      v.consumed[s].store(0, std::memory_order_relaxed);
      v.abandoned[s].store(~0ull, std::memory_order_relaxed);
    }
    memset(v.ctl, 0, sizeof(SrvCtl));
    // a CU-masked stream is a queue of its own: the persistent wave never sits in front of
    // another stream's work (one CU is enough for one wave); without it, a plain stream
    // and a short lifetime bound the wait of whatever shares its queue
    uint32_t mask[8] = {1u, 0, 0, 0, 0, 0, 0, 0};
    const bool masked = hipExtStreamCreateWithCUMask(&v.st, 8, mask) == hipSuccess;
    if (!masked && hipStreamCreateWithFlags(&v.st, hipStreamNonBlocking) != hipSuccess) {
      v.init_rc = RF_AMD_EINVAL;
      return;
    }
    // s_memrealtime runs at 100 MHz. Idle exit 400 us, lifetime 800 us (busy or not; waiters
    // relaunch it, a few us per relaunch): the masked stream synchronises with the legacy null
    // stream and hipDeviceSynchronize waits for every stream, so a device-wide sync or a
    // null-stream op waits at most one lifetime, under 1 ms, for a running wave.
    // rf_amd_lookup_server_set_times (or RF_AMD_SERVER_IDLE_US / _LIFE_US) sets others.
    const char* idle = getenv("RF_AMD_SERVER_IDLE_US");
    const char* life = getenv("RF_AMD_SERVER_LIFE_US");
    if (!v.idle_ticks.load()) v.idle_ticks = (idle ? strtoull(idle, nullptr, 10) : 400) * 100;
    if (!v.life_ticks.load()) v.life_ticks = (life ? strtoull(life, nullptr, 10) : 800) * 100;
    v.ready.store(true, std::memory_order_release);  // reapers on other threads may look now
  });
  return v.init_rc ? fail(v.init_rc, "lookup server allocation failed") : 0;
}

// make sure a server wave is running (or queued): the first submit launches one; a server that
// exited (idle, lifetime, stop) while tickets wait is relaunched from the first ticket it did
// not serve. The generation CAS makes exactly one caller launch.
static int srv_dead(rf_amd_engine* e);
static int srv_ensure(rf_amd_engine* e) {
  LookupServer& v = e->srv;
  if (int rc = srv_dead(e)) return rc;  // a dead server is never relaunched
  uint64_t s = v.state.load(std::memory_order_acquire);
  const uint64_t gen = s >> 1;
  if (s & 1) {
    if (__atomic_load_n(&v.ctl->exit_gen, __ATOMIC_ACQUIRE) != gen) return 0;  // running
  }
  const uint64_t next = ((gen + 1) << 1) | 1;
  if (!v.state.compare_exchange_strong(s, next, std::memory_order_acq_rel)) return 0;  // another launched
  const uint64_t head = __atomic_load_n(&v.ctl->exit_head, __ATOMIC_ACQUIRE);
  (void)hipSetDevice(e->device);
  if (int rc = rf_launch_lookup_server(v.st, v.ring, v.res, v.ctl, head, gen + 1, v.idle_ticks.load(),
                                       v.life_ticks.load())) {
    int z = 0;
    v.dead.compare_exchange_strong(z, RF_AMD_EINVAL);
    return launch_rc("lookup server", rc);
  }
  v.launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

static void srv_stop(rf_amd_engine* e) {
  LookupServer& v = e->srv;
  if (!v.ctl || !v.st) return;
  v.ready.store(false, std::memory_order_release);
  srv_set_stop(v);
  (void)hipStreamSynchronize(v.st);
  (void)hipStreamDestroy(v.st);
  if (v.ring_dev)
    (void)hipFree(v.ring);
  else
    (void)hipHostFree(v.ring);
  v.ring = nullptr;
  (void)hipHostFree(v.res);
  (void)hipHostFree(v.ctl);
  v.st = nullptr;
  v.ctl = nullptr;
}

// stops the server wave and waits, at most budget_ms, for the engine's streams to drain (no
// device-wide wait: other streams of the process are not the engine's)
static bool stream_drained(hipStream_t st, uint64_t deadline_ns);
static bool engine_quiesce(rf_amd_engine* e, int budget_ms) {
  (void)hipSetDevice(e->device);
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  const uint64_t deadline = (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec + (uint64_t)budget_ms * 1000000ull;
  LookupServer& v = e->srv;
  if (v.ctl) srv_set_stop(v);
  if (v.st && !stream_drained(v.st, deadline)) return false;
  if (!stream_drained(e->stream, deadline)) return false;
  std::lock_guard<std::mutex> g(e->slot_mu);
  for (ProbeSlot* s : e->slots_all)
    if (s->st && !stream_drained(s->st, deadline)) return false;
  return true;
}
static bool stream_drained(hipStream_t st, uint64_t deadline_ns) {
  for (;;) {
    const hipError_t q = hipStreamQuery(st);
    if (q != hipErrorNotReady) return true;  // idle, or faulted: nothing more will run on it
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    if ((uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec > deadline_ns) return false;
    struct timespec nap = {0, 100000};
    nanosleep(&nap, nullptr);
  }
}

// the server stream's error, if its kernel faulted (checked while waiting)
static int srv_check(rf_amd_engine* e) {
  const hipError_t q = hipStreamQuery(e->srv.st);
  if (q == hipSuccess || q == hipErrorNotReady) return 0;
  int z = 0;
  e->srv.dead.compare_exchange_strong(z, RF_AMD_EINVAL);
  return fail(RF_AMD_EINVAL, std::string("lookup server: ") + hipGetErrorString(q));
}
static int srv_dead(rf_amd_engine* e) {
  const int d = e->srv.dead.load(std::memory_order_acquire);
  return d ? fail(d, "lookup server failed earlier") : 0;
}

static ProbeGroup probe_group_of(const rf_amd_batch* b, uint32_t f);
static int batch_errors(rf_amd_batch* b);

// the request's 16 words (payload | check << 32) into its slot. Each 8-byte word is valid on
// its own, so 16-byte (SSE) stores are as safe as 8-byte ones; no sfence after a request
// (whole lines leave the write-combining buffers without one)
static inline void srv_write_request(uint64_t* dst, const uint32_t* p, uint64_t ck) {
  alignas(16) uint64_t w[SRV_REQ_WORDS];
  for (uint32_t k = 0; k < SRV_REQ_WORDS; k++) w[k] = (uint64_t)p[k] | ck;
  for (uint32_t k = 0; k < SRV_REQ_WORDS; k += 2)
    _mm_store_si128(reinterpret_cast<__m128i*>(dst + k), _mm_load_si128(reinterpret_cast<const __m128i*>(w + k)));
}

// RF_AMD_SUBMIT_PROFILE=1 (diagnostics): TSC cycles of the steps of rf_amd_lookup_submit --
// checks, ticket + slot wait, request write, server check -- printed to stderr at exit
static int g_subprof = -1;
static uint64_t g_subprof_cyc[7], g_subprof_n;
// a TSC stamp that waits for the loads before it (lfence on both sides): each step's misses
// land in its own interval
static inline uint64_t tsc_ser() {
  _mm_lfence();
  const uint64_t t = __rdtsc();
  _mm_lfence();
  return t;
}
// the reaper's side (one completion thread in the profiled runs): TSC cycles of reaps that
// returned states -- the idle look at the next answer, lock + cursor, the answer loop -- and
// the states they returned
static uint64_t g_reapprof_cyc[3], g_reapprof_n, g_reapprof_states;
static rf_amd_engine* g_subprof_eng = nullptr;
static void subprof_print() {
  if (g_subprof_eng && g_subprof_eng->srv.ctl && g_subprof_eng->srv.ctl->prof[5]) {
    const uint64_t* q = g_subprof_eng->srv.ctl->prof;
    const double np = (double)q[5];
    fprintf(stderr, "rf_amd server passes (RF_SRV_PROF build): %llu served, us each: poll %.2f payloads %.2f "
            "probe+answers %.2f; %.1f requests per pass, %llu passes cut by a request still arriving\n",
            (unsigned long long)q[5], q[0] / np / 100, q[1] / np / 100, q[2] / np / 100, q[4] / np,
            (unsigned long long)q[3]);
  }
  if (g_reapprof_n)
    fprintf(stderr, "rf_amd reap profile: %llu reaps with answers, %.1f states each, TSC cycles each: idle look %.0f "
            "lock+cursor %.0f answers %.0f\n", (unsigned long long)g_reapprof_n, (double)g_reapprof_states / g_reapprof_n,
            (double)g_reapprof_cyc[0] / g_reapprof_n, (double)g_reapprof_cyc[1] / g_reapprof_n,
            (double)g_reapprof_cyc[2] / g_reapprof_n);
  if (g_subprof_n)
    fprintf(stderr, "rf_amd submit profile: %llu submissions, TSC cycles each: checks %.0f (args %.0f init %.0f "
            "errors %.0f) ticket %.0f write %.0f ensure %.0f\n",
            (unsigned long long)g_subprof_n, (double)g_subprof_cyc[0] / g_subprof_n, (double)g_subprof_cyc[4] / g_subprof_n,
            (double)g_subprof_cyc[5] / g_subprof_n, (double)g_subprof_cyc[6] / g_subprof_n,
            (double)g_subprof_cyc[1] / g_subprof_n, (double)g_subprof_cyc[2] / g_subprof_n,
            (double)g_subprof_cyc[3] / g_subprof_n);
}

extern "C" int rf_amd_lookup_submit(rf_amd_engine* e, rf_amd_batch* b, uint32_t filter_index, uint32_t hash,
                                    void* tag, uint64_t* ticket) {
  if (g_subprof < 0) {
    const char* pv = getenv("RF_AMD_SUBMIT_PROFILE");
    g_subprof = pv && atoi(pv) > 0;
    if (g_subprof) atexit(subprof_print);
  }
  const uint64_t c0 = g_subprof > 0 ? tsc_ser() : 0;
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (g_subprof > 0) g_subprof_eng = e;
  if (!b || !b->built || b->eng != e) return fail(RF_AMD_EINVAL, "lookup on an unbuilt or foreign batch");
  if (filter_index >= b->F) return fail(RF_AMD_EINVAL, "bad filter index");
  if (!ticket) return fail(RF_AMD_EINVAL, "null ticket");
  const uint64_t c0a = g_subprof > 0 ? tsc_ser() : 0;
  if (__builtin_expect(!e->srv.ready.load(std::memory_order_acquire), 0))
    if (int rc = srv_init(e)) return rc;
  const uint64_t c0b = g_subprof > 0 ? tsc_ser() : 0;
  if (int rc = batch_errors(b)) return rc;
  const uint64_t c0c = g_subprof > 0 ? tsc_ser() : 0;
  if (int rc = srv_dead(e)) return rc;
  LookupServer& v = e->srv;
  const uint64_t c1 = g_subprof > 0 ? tsc_ser() : 0;
  const uint64_t t = v.tail.fetch_add(1, std::memory_order_acq_rel);
  const uint32_t slot = (uint32_t)(t & (SRV_RING - 1));
  if (t >= SRV_RING) {
    // the slot's previous ticket p must have been taken: by the reaper (a tagged ticket: the
    // reap cursor passed it, having copied its answer out), by its waiter (consumed), or never
    // published (abandoned)
    const uint64_t p = t - SRV_RING;
    // the reap cursor only moves forward, and it is usually ~64 tickets behind the tail, far
    // past p = t - SRV_RING: a submitting thread re-reads it (a line the reaper writes on every
    // reap) only when its last look does not already show p reaped
    static thread_local uint64_t hint_uid = 0, hint_seen = 0;
    if (hint_uid != e->uid) {
      hint_uid = e->uid;
      hint_seen = 0;
    }
    auto reaped = [&] {
      if (hint_seen > p) return true;
      hint_seen = v.reap_hint.load(std::memory_order_acquire);
      return hint_seen > p;
    };
    auto taken = [&] {
      if (v.consumed[slot].load(std::memory_order_acquire) == p + 1) return true;
      if (!reaped()) return false;
      if (v.abandoned[slot].load(std::memory_order_acquire) == p) return true;
      return v.meta[slot].ticket.load(std::memory_order_acquire) == p && v.meta[slot].tag != nullptr;
    };
    for (uint32_t spin = 1; !taken(); spin++) {
      __builtin_ia32_pause();
      if ((spin & 1023) == 0) {  // ticket t stays unpublished only on a server that is dead
        int rc = srv_ensure(e);
        if (!rc) rc = srv_check(e);
        if (!rc) rc = srv_dead(e);
        if (rc) {  // ticket t is never published: the cursors step over it
          v.abandoned[slot].store(t, std::memory_order_release);
          return rc;
        }
      }
    }
    // the slot is being rewritten: readers that see this do not trust its tag (the server
    // reads the request only after its new ticket is published)
    v.meta[slot].ticket.store(SRV_BUSY, std::memory_order_relaxed);
    std::atomic_thread_fence(std::memory_order_release);  // BUSY before the new tag (a seqlock)
  }
  const uint64_t c2 = g_subprof > 0 ? tsc_ser() : 0;
  {
    // 16 words, each with t's check in its high half; plain 8-byte stores in any order (two
    // whole 64-byte lines: through the write-combining BAR mapping they leave as two bursts)
    const ProbeGroup g = probe_group_of(b, filter_index);
    const uint64_t tg = (uint64_t)(uintptr_t)tag;
    const uint64_t lp = (uint64_t)(uintptr_t)g.lines, pp = (uint64_t)(uintptr_t)g.pages, sp = (uint64_t)(uintptr_t)g.slots;
    const uint32_t p[SRV_REQ_WORDS] = {g.x, g.err, g.fpl, hash, (uint32_t)lp, (uint32_t)(lp >> 32), (uint32_t)pp, (uint32_t)(pp >> 32),
                                       (uint32_t)sp, (uint32_t)(sp >> 32), (uint32_t)tg, (uint32_t)(tg >> 32), 0u, 0u, 0u, 0u};
    v.meta[slot].tag = tag;
    v.meta[slot].ticket.store(t, std::memory_order_release);
    const uint64_t ck = (uint64_t)srv_check(t) << 32;
    srv_write_request(v.ring[slot].w, p, ck);
  }
  *ticket = t;
  const uint64_t c3 = g_subprof > 0 ? tsc_ser() : 0;
  // published: from here the ticket's tag comes back through rf_amd_lookup_reap or, if the
  // server is (or now becomes) dead, rf_amd_lookup_server_failed -- so a launch failure here is
  // not the submit's error (the caller would complete the state a second time)
  (void)srv_ensure(e);
  if (g_subprof > 0) {  // one submitting thread in the profiled runs: plain sums
    const uint64_t c4 = tsc_ser();
    g_subprof_cyc[0] += c1 - c0;
    g_subprof_cyc[4] += c0a - c0;
    g_subprof_cyc[5] += c0b - c0a;
    g_subprof_cyc[6] += c0c - c0b;
    g_subprof_cyc[1] += c2 - c1;
    g_subprof_cyc[2] += c3 - c2;
    g_subprof_cyc[3] += c4 - c3;
    g_subprof_n++;
  }
  return 0;
}

extern "C" int rf_amd_lookup_wait(rf_amd_engine* e, uint64_t ticket, uint64_t* found_values) {
  if (!e || !e->srv.ready.load(std::memory_order_acquire)) return fail(RF_AMD_EINVAL, "no lookup server");
  LookupServer& v = e->srv;
  const uint32_t slot = (uint32_t)(ticket & (SRV_RING - 1));
  for (uint32_t spin = 1;; spin++) {
    if (srv_answer(&v.res[slot], ticket, found_values, nullptr) == 1) {
      v.consumed[slot].store(ticket + 1, std::memory_order_release);
      return 0;
    }
    __builtin_ia32_pause();
    if ((spin & 255) == 0) {
      if (int rc = srv_dead(e)) return rc;
      if (int rc = srv_ensure(e)) return rc;
      if ((spin & 65535) == 0)
        if (int rc = srv_check(e)) return rc;
    }
  }
}

extern "C" uint64_t rf_amd_lookup_reap(rf_amd_engine* e, void** tags, uint64_t* found_values, uint64_t max) {
  // (ready, not ring: another thread's srv_init may have allocated the request ring only)
  if (!e || !e->srv.ready.load(std::memory_order_acquire) || !tags || !found_values) return 0;
  LookupServer& v = e->srv;
  const bool prof = g_subprof > 0;
  const uint64_t r0 = prof ? __rdtsc() : 0;
  {
    // an idle reap (callers spin on this) looks only at the next ticket's answer line, which
    // only the GPU writes: no lock taken, no line the submitters write read. The full pass
    // below runs once that ticket is answered (or its slot moved on: answered later tickets
    // mean a waiter took it), when it was abandoned, and every few microseconds regardless --
    // it relaunches a server that exited with tickets waiting and notices a faulted one.
    const uint64_t t = v.reap_hint.load(std::memory_order_relaxed);
    const uint32_t slot = (uint32_t)(t & (SRV_RING - 1));
    if (srv_answer(&v.res[slot], t, nullptr, nullptr) == 0 && v.abandoned[slot].load(std::memory_order_relaxed) != t) {
      static thread_local uint64_t last_full = 0;
      const uint64_t now = __rdtsc();
      if (now - last_full < 8192) return 0;  // a few microseconds at the hosts' TSC rates
      last_full = now;
    }
  }
  const uint64_t r1 = prof ? __rdtsc() : 0;
  std::unique_lock<std::mutex> lk(v.reap_mu, std::try_to_lock);
  if (!lk.owns_lock()) return 0;  // another thread is reaping
  uint64_t n = 0, t = v.reap_next;
  // Only the answer lines are read: written by the GPU over PCIe (a miss each, fetched ahead so
  // the misses of consecutive tickets overlap), they carry the request's tag and check -- no line
  // of the submitting threads is touched per state, not even the ticket counter: a slot past
  // the last ticket holds an older check and stops the loop like an unanswered one. Ticket t is
  // done when its answer is there (a waiter's, tag 0, is left to its waiter), when its slot
  // already holds a later answer (a waiter took t and the slot was reused), or when it was
  // abandoned unpublished.
  const uint64_t r2 = prof ? __rdtsc() : 0;
  for (uint64_t q = t; q < t + 16; q += 2) __builtin_prefetch(&v.res[q & (SRV_RING - 1)], 0, 0);
  while (n < max) {
    const uint32_t slot = (uint32_t)(t & (SRV_RING - 1));
    if ((t & 1) == 0) __builtin_prefetch(&v.res[(t + 16) & (SRV_RING - 1)], 0, 0);
    uint64_t found = 0, tag = 0;
    const int a = srv_answer(&v.res[slot], t, &found, &tag);
    if (a == 1) {
      if (tag) {
        tags[n] = (void*)(uintptr_t)tag;
        found_values[n] = found;
        n++;
      }
      t++;
      continue;
    }
    if (a < 0 || v.abandoned[slot].load(std::memory_order_acquire) == t) {
      t++;
      continue;
    }
    break;  // not answered yet (or past the last ticket)
  }
  v.reap_next = t;
  v.reap_hint.store(t, std::memory_order_release);  // the answers before t are copied out
  lk.unlock();
  if (prof && n) {
    const uint64_t r3 = __rdtsc();
    g_reapprof_cyc[0] += r1 - r0;
    g_reapprof_cyc[1] += r2 - r1;
    g_reapprof_cyc[2] += r3 - r2;
    g_reapprof_n++;
    g_reapprof_states += n;
  }
  if (n == 0 && t < v.tail.load(std::memory_order_acquire)) {
    (void)srv_ensure(e);
    // a faulted server stream never answers and nothing else would notice with only tagged
    // tickets outstanding: look at it about once a millisecond, so `dead` gets set and the
    // caller's rf_amd_lookup_server_error / _failed path completes the waiting states
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    const uint64_t now = (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
    uint64_t last = v.last_check_ns.load(std::memory_order_relaxed);
    if (now - last > 1000000 && v.last_check_ns.compare_exchange_strong(last, now)) (void)srv_check(e);
  }
  return n;
}

// a dead server's unanswered tickets: the tags of the published ones from the reap cursor on
// (waiters' tickets skipped: rf_amd_lookup_wait returns the error to them), consumed here
extern "C" uint64_t rf_amd_lookup_server_failed(rf_amd_engine* e, void** tags, uint64_t max) {
  if (!e || !e->srv.ready.load(std::memory_order_acquire) || !tags || !e->srv.dead.load(std::memory_order_acquire)) return 0;
  LookupServer& v = e->srv;
  std::lock_guard<std::mutex> lk(v.reap_mu);
  uint64_t n = 0, t = v.reap_next;
  const uint64_t tail = v.tail.load(std::memory_order_acquire);
  // Stops at the first ticket not yet published: a submitter that passed the dead
  // check before `dead` was set publishes it later, and the next call hands its tag back. A
  // ticket its submitter abandoned is stepped over; a slot already holding a later ticket means
  // a waiter took ticket t (waiters' tickets are not tagged).
  for (; n < max && t < tail; t++) {
    const uint32_t slot = (uint32_t)(t & (SRV_RING - 1));
    const uint64_t tk = v.meta[slot].ticket.load(std::memory_order_acquire);
    if (tk != t) {
      if (v.abandoned[slot].load(std::memory_order_acquire) == t) continue;
      if (tk == SRV_UNPUBLISHED || tk == SRV_BUSY || tk < t) break;
      continue;  // reused: a waiter's ticket, already taken
    }
    void* tag = v.meta[slot].tag;
    std::atomic_thread_fence(std::memory_order_acquire);
    if (v.meta[slot].ticket.load(std::memory_order_relaxed) != t) break;  // being rewritten: next call
    if (!tag) continue;
    if (srv_answer(&v.res[slot], t, nullptr, nullptr) == 1) break;  // answered: reap takes it
    tags[n++] = tag;
    v.consumed[slot].store(t + 1, std::memory_order_release);
  }
  v.reap_next = t;
  v.reap_hint.store(t, std::memory_order_release);
  return n;
}

// diagnostics (rf_amd_diag.h): the server stops answering (its wave told to exit; a relaunched
// wave exits at once), then, after `gap_us`, is marked dead as a failed launch or a faulted
// stream marks it: tickets published in the gap are never answered
extern "C" int rf_amd_diag_lookup_server_kill(rf_amd_engine* e, int err, uint32_t gap_us) {
  if (!e || !err) return fail(RF_AMD_EINVAL, "bad argument");
  if (int rc = srv_init(e)) return rc;
  srv_set_stop(e->srv);
  if (gap_us) {
    struct timespec nap = {(time_t)(gap_us / 1000000), (long)(gap_us % 1000000) * 1000};
    nanosleep(&nap, nullptr);
  }
  int z = 0;
  e->srv.dead.compare_exchange_strong(z, err);
  return 0;
}

extern "C" int rf_amd_lookup_server_error(rf_amd_engine* e) { return e ? e->srv.dead.load() : RF_AMD_ENODEV; }

// the idle exit and lifetime (microseconds) of the server waves launched from now on (a
// host-controlled keep-alive: a caller that needs one wave across a long stretch raises them)
extern "C" int rf_amd_lookup_server_set_times(rf_amd_engine* e, uint64_t idle_us, uint64_t life_us) {
  if (!e || !idle_us || !life_us) return fail(RF_AMD_EINVAL, "bad server times");
  e->srv.idle_ticks = idle_us * 100;
  e->srv.life_ticks = life_us * 100;
  return 0;
}

extern "C" int rf_amd_diag_lookup_ring(rf_amd_engine* e) {
  if (!e || !e->srv.ready.load(std::memory_order_acquire)) return -1;
  return e->srv.ring_dev ? 1 : 0;
}

extern "C" int rf_amd_lookup_server_stats(rf_amd_engine* e, uint64_t* out) {
  if (!e || !out) return fail(RF_AMD_EINVAL, "null argument");
  out[0] = e->srv.tail.load();
  out[1] = e->srv.launches.load();
  out[2] = e->srv.ctl ? __atomic_load_n(&e->srv.ctl->exit_head, __ATOMIC_ACQUIRE) : 0;
  return 0;
}

// where a host-buffer lookup round trip spends its time (rf_amd_diag_lookup_stats): calls,
// ns before the launch (slot, buffers, build ordering, argument packing), ns in the launch
// call, ns waiting for the completion word (and copying the results out)
static std::atomic<uint64_t> g_lk_calls{0}, g_lk_prep_ns{0}, g_lk_launch_ns{0}, g_lk_wait_ns{0};
// which way probe_groups_host sent its round trips (rf_amd_diag_lookup_paths): small, mapped,
// copy, and how many of them waited by synchronising the stream
static std::atomic<uint64_t> g_lk_small{0}, g_lk_mapped{0}, g_lk_copy{0}, g_lk_sync{0};
static inline uint64_t mono_ns() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}
struct LookupClock {
  uint64_t t0 = mono_ns(), t1 = 0, t2 = 0;
  void launching() { t1 = mono_ns(); }
  void launched() { t2 = mono_ns(); }
  ~LookupClock() {
    if (!t2) return;  // failed before the launch
    const uint64_t t3 = mono_ns();
    g_lk_calls.fetch_add(1, std::memory_order_relaxed);
    g_lk_prep_ns.fetch_add(t1 - t0, std::memory_order_relaxed);
    g_lk_launch_ns.fetch_add(t2 - t1, std::memory_order_relaxed);
    g_lk_wait_ns.fetch_add(t3 - t2, std::memory_order_relaxed);
  }
};
#ifndef RF_AMD_SRC_ID
#define RF_AMD_SRC_ID "unknown"
#endif
extern "C" const char* rf_amd_build_id(void) { return RF_AMD_SRC_ID; }

extern "C" uint64_t rf_amd_diag_k4_bitmap_builds(void) { return rf_k4_bitmap_builds(); }
extern "C" uint64_t rf_amd_diag_dense_line_filters(void) { return g_dense_line_filters.load(std::memory_order_relaxed); }
extern "C" uint64_t rf_amd_diag_part16_builds(void) { return rf_part16_builds(); }
extern "C" uint64_t rf_amd_diag_k4_packed_builds(void) { return rf_k4_packed_builds(); }

extern "C" int rf_amd_diag_lookup_stats(uint64_t* out, int reset) {
  if (!out) return fail(RF_AMD_EINVAL, "null output");
  std::atomic<uint64_t>* c[4] = {&g_lk_calls, &g_lk_prep_ns, &g_lk_launch_ns, &g_lk_wait_ns};
  for (int k = 0; k < 4; k++) out[k] = reset ? c[k]->exchange(0) : c[k]->load();
  return 0;
}

extern "C" int rf_amd_diag_lookup_paths(uint64_t* out, int reset) {
  if (!out) return fail(RF_AMD_EINVAL, "null output");
  std::atomic<uint64_t>* c[4] = {&g_lk_small, &g_lk_mapped, &g_lk_copy, &g_lk_sync};
  for (int k = 0; k < 4; k++) out[k] = reset ? c[k]->exchange(0) : c[k]->load();
  return 0;
}

static int probe_groups_host(rf_amd_engine* e, const std::vector<ProbeGroup>& groups,
                             const uint32_t* h_hashes, const uint32_t* h_group, uint64_t n, uint64_t* h_found) {
  if (n == 0) return 0;
  LookupClock clk;
  static const int mode = env_mode("RF_AMD_PROBE_MODE", "mapped", "copy");
  static const int wait = env_mode("RF_AMD_PROBE_WAIT", "flag", "sync");
  static const bool small_ok = !getenv("RF_AMD_PROBE_SMALL") || atoi(getenv("RF_AMD_PROBE_SMALL")) != 0;
  const uint32_t ng = (uint32_t)groups.size();
  const size_t o_g = (8 * n + 15) & ~15ull, o_f = (o_g + sizeof(ProbeGroup) * ng + 63) & ~63ull;
  const bool small = small_ok && wait != 2 && n <= SMALL_PROBES && ng <= SMALL_GROUPS;
  const bool mapped = mode == 1 || (mode == 0 && n <= MAPPED_MAX_PROBES);
  (small ? g_lk_small : mapped ? g_lk_mapped : g_lk_copy).fetch_add(1, std::memory_order_relaxed);
  if (!small && wait == 2) g_lk_sync.fetch_add(1, std::memory_order_relaxed);
  ProbeSlot* s = slot_take(e);
  if (!s) return RF_AMD_ENOMEM;
  struct Give {
    rf_amd_engine* e;
    ProbeSlot* s;
    ~Give() { slot_give(e, s); }
  } give{e, s};
  if (int rc = slot_reserve(s, small ? 8 * n : o_f + 8 * n, (small || mapped) ? 0 : o_f)) return rc;
  const uint64_t issued = e->builds_issued.load(std::memory_order_acquire);
  if (issued != e->builds_seen_idle.load(std::memory_order_acquire)) {
    if (hipStreamQuery(e->stream) == hipErrorNotReady) {  // order after builds still in flight
      hipEvent_t ev;
      HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      HIPCHK(hipEventRecord(ev, e->stream));
      HIPCHK(hipStreamWaitEvent(s->st, ev, 0));
      (void)hipEventDestroy(ev);
    } else {
      e->builds_seen_idle.store(issued, std::memory_order_release);  // every build up to `issued` is done
    }
  }
  const uint32_t seq = ++s->seq ? s->seq : ++s->seq;  // never 0 (the flag's initial value)
  (void)hipGetLastError();
  if (small) {  // everything in the kernel arguments: no host-memory read before the probe
    SmallProbe sp;
    memset(&sp, 0, sizeof(sp));
    sp.n = (uint32_t)n;
    sp.ng = ng;
    sp.seq = seq;
    for (uint64_t i = 0; i < n; i++) {
      sp.h[i] = h_hashes[i];
      const uint32_t g = h_group ? h_group[i] : 0u;
      sp.g[i] = (uint8_t)(g < ng ? g : 255u);
    }
    for (uint32_t g = 0; g < ng; g++) sp.groups[g] = groups[g];
    sp.found = reinterpret_cast<uint64_t*>(s->h);
    sp.done_flag = s->flag;
    clk.launching();
    if (int rc = launch_rc("probe", rf_launch_probe_small(s->st, &sp))) return rc;
    clk.launched();
    if (int rc = slot_wait(s, seq, false)) return rc;
    memcpy(h_found, s->h, 8 * n);
    return 0;
  }
  memcpy(s->h, h_hashes, 4 * n);
  uint32_t* hg = reinterpret_cast<uint32_t*>(s->h + 4 * n);
  if (h_group) memcpy(hg, h_group, 4 * n);
  else memset(hg, 0, 4 * n);
  memcpy(s->h + o_g, groups.data(), sizeof(ProbeGroup) * ng);
  const uint8_t* in = s->h;
  if (!mapped) {
    HIPCHK(hipMemcpyAsync(s->d, s->h, o_f, hipMemcpyHostToDevice, s->st));
    in = s->d;
  }
  uint64_t* found = reinterpret_cast<uint64_t*>(s->h + o_f);
  clk.launching();
  if (int rc = launch_rc("probe", rf_launch_probe_groups(s->st, reinterpret_cast<const uint32_t*>(in),
                                                         reinterpret_cast<const ProbeGroup*>(in + o_g), ng, n, found,
                                                         s->d_counter, wait == 2 ? nullptr : s->flag, seq)))
    return rc;
  clk.launched();
  if (int rc = slot_wait(s, seq, wait == 2)) return rc;
  memcpy(h_found, found, 8 * n);
  return 0;
}

extern "C" int rf_amd_batch_probe_hashes_host(rf_amd_batch* b, const uint32_t* h_hashes, const uint32_t* h_filter_id,
                                              uint64_t n, uint64_t* h_found) {
  if (!b || !b->built) return fail(RF_AMD_EINVAL, "probe on an unbuilt batch");
  if (n == 0) return 0;
  if (!h_hashes || !h_found) return fail(RF_AMD_EINVAL, "null probe buffer");
  rf_amd_engine* e = b->eng;
  HIPCHK(hipSetDevice(e->device));
  if (int rc = batch_errors(b)) return rc;
  std::vector<ProbeGroup> groups(h_filter_id ? b->F : 1);  // group = filter id (ids >= F find nothing)
  for (uint32_t f = 0; f < groups.size(); f++) groups[f] = probe_group_of(b, f);
  return probe_groups_host(e, groups, h_hashes, h_filter_id, n, h_found);
}

extern "C" int rf_amd_probe_filters_host(rf_amd_engine* e, rf_amd_batch* const* batches, const uint32_t* filter_index,
                                         uint32_t num_groups, const uint32_t* h_hashes, const uint32_t* h_group,
                                         uint64_t n, uint64_t* h_found) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (num_groups && !batches) return fail(RF_AMD_EINVAL, "null group arrays");
  if (n == 0) return 0;
  if (!h_hashes || !h_found) return fail(RF_AMD_EINVAL, "null probe buffer");
  HIPCHK(hipSetDevice(e->device));
  // each group carries its own batch's routing config: filters of kvstores with different
  // fingerprint or index sizes go out in the same launch
  std::vector<ProbeGroup> groups(num_groups);
  for (uint32_t g = 0; g < num_groups; g++) {
    rf_amd_batch* b = batches[g];
    const uint32_t f = filter_index ? filter_index[g] : 0u;
    if (!b || !b->built || b->eng != e) return fail(RF_AMD_EINVAL, "group on an unbuilt or foreign batch");
    if (f >= b->F) return fail(RF_AMD_EINVAL, "bad filter index");
    if (int rc = batch_errors(b)) return rc;
    groups[g] = probe_group_of(b, f);
  }
  if (!num_groups) {  // no filters: nothing found
    memset(h_found, 0, 8 * n);
    return 0;
  }
  return probe_groups_host(e, groups, h_hashes, h_group, n, h_found);
}

// Lookups against many resident filters in ONE launch: group g probes counts[g] hashes
// (consecutive in h_hashes) against filter filter_index[g] of batches[g] -- the batch form of
// trunk_merge_lookup's per-bundle routing_filter_lookup calls (src/trunk.c:6008-6075) and of
// a flush of queued routing_filter_lookup_async states.
extern "C" int rf_amd_probe_many_hashes_host(rf_amd_engine* e, rf_amd_batch* const* batches,
                                             const uint32_t* filter_index, const uint64_t* counts,
                                             uint32_t num_groups, const uint32_t* h_hashes, uint64_t* h_found) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (num_groups && (!batches || !counts)) return fail(RF_AMD_EINVAL, "null group arrays");
  uint64_t n = 0;
  for (uint32_t g = 0; g < num_groups; g++) n += counts[g];
  if (n == 0) return 0;
  std::vector<uint32_t> gid(n);
  for (uint32_t g = 0, at = 0; g < num_groups; at += (uint32_t)counts[g], g++)
    std::fill(gid.begin() + at, gid.begin() + at + counts[g], g);
  return rf_amd_probe_filters_host(e, batches, filter_index, num_groups, h_hashes, gid.data(), n, h_found);
}

// ---- multi-get: a resident filter set, fan-out probes, candidate lists --------------------
// The set is the ProbeGroup table of rf_amd_probe_filters_host kept in device memory: member
// g's probe lines, pages and slots by address. Those buffers stay where they are for the
// batch's lifetime -- rf_amd_batch_trim keeps d_lines, d_pages and d_slots and releases only the
// others -- so a set outlives a trim of its members without re-resolving anything.
// The table has `capacity` entries, num_members of them in use (the probes' bound); the others
// are NULL members. A set is its host state (rf_set_plan.h: the count, each slot's seed and
// whether a filter sits in it, the seed rule of the keys forms) plus that table.
struct rf_amd_filter_set : SetState {
  rf_amd_engine* eng = nullptr;
  DevBuf d_groups;
  // what a member update hands the planner and gets back, kept between calls
  std::vector<uint32_t> upd_seed;
  std::vector<uint8_t> upd_kind;  // SetMemberKind of every entry
  SetUpdatePlan upd_plan;
};

static ProbeGroup null_group() {  // NULL_ROUTING_FILTER: finds nothing
  ProbeGroup g;
  memset(&g, 0, sizeof(g));
  g.err = 1;
  return g;
}

// RF_AMD_MEMBER_UNFILTERED (src/trunk.c:6020-6022): the NULL entry that finds value 0 for every key
static ProbeGroup unfiltered_group() {
  ProbeGroup g = null_group();
  g.err |= GROUP_UNFILTERED;
  return g;
}

static uint8_t member_kind(const rf_amd_batch* b) {
  return !b ? SET_NULL : b == RF_AMD_MEMBER_UNFILTERED ? SET_UNFILTERED : SET_FILTER;
}

// a member named by a call: nullptr batch = NULL_ROUTING_FILTER, RF_AMD_MEMBER_UNFILTERED (neither
// is dereferenced), else a built batch of engine e and one of its filters
static int check_member(const rf_amd_engine* e, const rf_amd_batch* b, uint32_t f) {
  if (member_kind(b) != SET_FILTER) return 0;
  if (!b->built || b->eng != e) return fail(RF_AMD_EINVAL, "member on an unbuilt or foreign batch");
  if (f >= b->F) return fail(RF_AMD_EINVAL, "bad filter index");
  return 0;
}

static int filter_set_create(rf_amd_engine* e, rf_amd_batch* const* batches, const uint32_t* filter_index,
                             uint32_t num_members, uint32_t capacity, rf_amd_filter_set** out) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (!out) return fail(RF_AMD_EINVAL, "null out-param");
  *out = nullptr;
  if (num_members && !batches) return fail(RF_AMD_EINVAL, "null member arrays");
  if (capacity < num_members) return fail(RF_AMD_EINVAL, "capacity below num_members");
  HIPCHK(hipSetDevice(e->device));
  auto s = std::make_unique<rf_amd_filter_set>();
  s->eng = e;
  s->init(capacity);
  std::vector<ProbeGroup> groups(capacity, null_group());
  std::vector<uint32_t> ids(num_members);
  // room for any later call of up to `capacity` entries: an update then allocates nothing on
  // the host either
  s->upd_seed.reserve(capacity);
  s->upd_kind.reserve(capacity);
  s->upd_plan.order.reserve(capacity);
  s->upd_plan.cuts.reserve(capacity / SET_UPD_PER_LAUNCH + 2);
  s->upd_seed.assign(num_members, 0u);
  s->upd_kind.assign(num_members, SET_NULL);
  for (uint32_t g = 0; g < num_members; g++) {
    ids[g] = g;
    rf_amd_batch* b = batches[g];
    s->upd_kind[g] = member_kind(b);
    if (s->upd_kind[g] == SET_UNFILTERED) groups[g] = unfiltered_group();
    if (s->upd_kind[g] != SET_FILTER) continue;
    const uint32_t f = filter_index ? filter_index[g] : 0u;
    if (int rc = check_member(e, b, f)) return rc;
    if (int rc = batch_errors(b)) return rc;
    groups[g] = probe_group_of(b, f);
    s->upd_seed[g] = b->cfg.seed;
  }
  // the members as one update of the empty set: its count and seed rule (the entries go up by
  // the copy below, not by launches)
  std::string msg;
  if (int rc = plan_set_update(s.get(), num_members, ids.data(), s->upd_kind.data(), s->upd_seed.data(),
                               &s->upd_plan, &msg))
    return fail(rc, msg);
  if (s->d_groups.alloc(sizeof(ProbeGroup) * capacity, &e->pool)) return RF_AMD_ENOMEM;
  if (capacity) {
    HIPCHK(hipMemcpyAsync(s->d_groups.p, groups.data(), sizeof(ProbeGroup) * capacity, hipMemcpyHostToDevice,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));  // `groups` is pageable; probes may run on any stream
  }
  *out = s.release();
  return 0;
}

extern "C" int rf_amd_filter_set_create(rf_amd_engine* e, rf_amd_batch* const* batches, const uint32_t* filter_index,
                                        uint32_t num_members, rf_amd_filter_set** out) {
  return filter_set_create(e, batches, filter_index, num_members, num_members, out);
}

extern "C" int rf_amd_filter_set_create_cap(rf_amd_engine* e, rf_amd_batch* const* batches,
                                            const uint32_t* filter_index, uint32_t num_members, uint32_t capacity,
                                            rf_amd_filter_set** out) {
  if (out) *out = nullptr;
  if (capacity == 0) return fail(RF_AMD_EINVAL, "capacity 0");
  return filter_set_create(e, batches, filter_index, num_members, capacity, out);
}

extern "C" uint32_t rf_amd_filter_set_capacity(const rf_amd_filter_set* s) { return s ? s->capacity : 0; }

// Members replaced in stream order: every entry is validated and the call planned on the host
// (rf_set_plan.h) before the first launch, then ceil(entries / SET_UPD_PER_LAUNCH) launches of
// k_set_update carry the entries in their arguments. A launch the runtime refuses comes after
// the planner has changed the host state: the set is then undefined (rf_amd.h). The call's host
// scratch lives in the set, so the caller serialises calls on one set. Nothing is waited for and
// nothing allocated on the device: a member's build error is read by the kernel from the batch's
// d_outs (which rf_amd_batch_trim keeps), behind that build on the stream; bits the host has
// read back already (err_ready) travel with the entry.
extern "C" int rf_amd_filter_set_update(rf_amd_filter_set* s, const uint32_t* member_id, rf_amd_batch* const* batches,
                                        const uint32_t* filter_index, uint32_t count, void* stream) {
  if (!s) return fail(RF_AMD_EINVAL, "null filter set");
  if (count == 0) return 0;
  if (!member_id || !batches) return fail(RF_AMD_EINVAL, "null member arrays");
  s->upd_seed.resize(count);
  s->upd_kind.resize(count);
  for (uint32_t i = 0; i < count; i++) {
    const rf_amd_batch* b = batches[i];
    if (int rc = check_member(s->eng, b, filter_index ? filter_index[i] : 0u)) return rc;
    s->upd_kind[i] = member_kind(b);
    s->upd_seed[i] = s->upd_kind[i] == SET_FILTER ? b->cfg.seed : 0u;
  }
  HIPCHK(hipSetDevice(s->eng->device));
  std::string msg;
  if (int rc = plan_set_update(s, count, member_id, s->upd_kind.data(), s->upd_seed.data(), &s->upd_plan, &msg))
    return fail(rc, msg);
  (void)hipGetLastError();
  const SetUpdatePlan& plan = s->upd_plan;
  SetUpdate a{};
  a.groups = s->d_groups.as<ProbeGroup>();
  a.cap = s->capacity;
  for (uint32_t l = 0; l < plan.launches(); l++) {
    a.n = plan.cuts[l + 1] - plan.cuts[l];
    for (uint32_t k = 0; k < a.n; k++) {
      const uint32_t i = plan.order[plan.cuts[l] + k];
      SetUpdEntry& en = a.e[k];
      rf_amd_batch* b = batches[i];
      en.id = member_id[i];
      en.pad = 0;
      if (s->upd_kind[i] != SET_FILTER) {
        en.g = s->upd_kind[i] == SET_UNFILTERED ? unfiltered_group() : null_group();
        en.out = nullptr;
        continue;
      }
      const uint32_t f = filter_index ? filter_index[i] : 0u;
      const uint32_t known = b->err_ready.load(std::memory_order_acquire) ? b->err_host[f] : 0u;
      en.g = probe_group_with(b, f, known);
      en.out = b->d_outs.as<FilterOut>() + f;
    }
    if (int rc = launch_rc("set update", rf_launch_set_update(stream_of(s->eng, stream), &a))) return rc;
  }
  return 0;
}

// synchronises the device (probes on a caller's stream may still read the table), as
// rf_amd_batch_destroy does
extern "C" void rf_amd_filter_set_destroy(rf_amd_filter_set* s) {
  if (!s) return;
  (void)hipSetDevice(s->eng->device);
  (void)hipDeviceSynchronize();
  delete s;
}

// stream-ordered destroy, as rf_amd_batch_destroy_on: every probe and update of the set is
// ordered before the current end of `stream`; the table's block is parked behind an event
// recorded there. Returns without waiting.
extern "C" int rf_amd_filter_set_destroy_on(rf_amd_filter_set* s, void* stream) {
  if (!s) return 0;
  HIPCHK(hipSetDevice(s->eng->device));
  DevBuf* const table = &s->d_groups;
  if (park_behind(s->eng, stream_of(s->eng, stream), &table, 1)) delete s;
  else rf_amd_filter_set_destroy(s);  // fall back to the synchronising destroy
  return 0;
}

extern "C" uint32_t rf_amd_filter_set_num_members(const rf_amd_filter_set* s) { return s ? s->num_members : 0; }

// The fixed form: key i against its K members (d_member == nullptr: all of them), d_member_off
// nullptr. The ragged form: key i against d_member[d_member_off[i] .. d_member_off[i+1]), K
// unused. `ragged` names the form, not d_member_off: a ragged call without offsets is refused
// as one (after its n == 0 return), not as a fixed call with K == 0. `exists`: the existence
// form of the same call, d_found then being the n bytes d_exists (rf_amd_filter_set_exists_*).
static int set_probe(rf_amd_filter_set* s, int kind, const void* in0, const uint64_t* offs, uint32_t key_len,
                     const uint32_t* d_member, uint32_t K, const uint64_t* d_member_off, uint64_t n,
                     void* d_found, void* stream, bool ragged, bool exists = false) {
  if (!s) return fail(RF_AMD_EINVAL, "null filter set");
  if (!ragged) {
    if (K == 0) return fail(RF_AMD_EINVAL, "K == 0");
    if (!d_member && K != s->num_members) return fail(RF_AMD_EINVAL, "all-members form: K must equal num_members");
  }
  if (kind != IN_HASH && !s->one_seed) return fail(RF_AMD_EINVAL, "keys form over members with different seeds");
  if (ragged ? n >= (1ull << 56) : n > ((1ull << 56) - 1) / K)
    return fail(RF_AMD_EINVAL, ragged ? "n >= 2^56" : "n * K >= 2^56");
  if (n == 0) return 0;
  if (!in0 || !d_found || (kind == IN_VAR && !offs) || (ragged && (!d_member || !d_member_off)))
    return fail(RF_AMD_EINVAL, "null probe buffer");
  HIPCHK(hipSetDevice(s->eng->device));
  (void)hipGetLastError();
  if (exists)
    return launch_rc(ragged ? "ragged existence probe" : "existence probe",
                     rf_launch_probe_fanout_exists(stream_of(s->eng, stream), kind, in0, offs, key_len, s->seed,
                                                   s->d_groups.as<ProbeGroup>(), s->num_members, d_member, K,
                                                   d_member_off, n, static_cast<uint8_t*>(d_found)));
  return launch_rc(ragged ? "ragged fan-out probe" : "fan-out probe",
                   rf_launch_probe_fanout(stream_of(s->eng, stream), kind, in0, offs, key_len, s->seed,
                                          s->d_groups.as<ProbeGroup>(), s->num_members, d_member, K, d_member_off, n,
                                          static_cast<uint64_t*>(d_found)));
}

extern "C" int rf_amd_filter_set_probe_keys(rf_amd_filter_set* s, const void* d_keys, uint32_t key_len,
                                            const uint32_t* d_member, uint32_t K, uint64_t n, uint64_t* d_found,
                                            void* stream) {
  if (key_len == 0) return fail(RF_AMD_EINVAL, "key_len 0");
  return set_probe(s, fixed_kind(d_keys, key_len), d_keys, nullptr, key_len, d_member, K, nullptr, n, d_found,
                   stream, false);
}
extern "C" int rf_amd_filter_set_probe_var_keys(rf_amd_filter_set* s, const uint8_t* d_bytes,
                                                const uint64_t* d_offsets, const uint32_t* d_member, uint32_t K,
                                                uint64_t n, uint64_t* d_found, void* stream) {
  return set_probe(s, IN_VAR, d_bytes, d_offsets, 0, d_member, K, nullptr, n, d_found, stream, false);
}
extern "C" int rf_amd_filter_set_probe_hashes(rf_amd_filter_set* s, const uint32_t* d_hashes, const uint32_t* d_member,
                                              uint32_t K, uint64_t n, uint64_t* d_found, void* stream) {
  return set_probe(s, IN_HASH, d_hashes, nullptr, 4, d_member, K, nullptr, n, d_found, stream, false);
}

// the ragged forms
extern "C" int rf_amd_filter_set_probe_keys_ragged(rf_amd_filter_set* s, const void* d_keys, uint32_t key_len,
                                                   const uint32_t* d_member, const uint64_t* d_member_off, uint64_t n,
                                                   uint64_t* d_found, void* stream) {
  if (key_len == 0) return fail(RF_AMD_EINVAL, "key_len 0");
  return set_probe(s, fixed_kind(d_keys, key_len), d_keys, nullptr, key_len, d_member, 0, d_member_off, n, d_found,
                   stream, true);
}
extern "C" int rf_amd_filter_set_probe_var_keys_ragged(rf_amd_filter_set* s, const uint8_t* d_bytes,
                                                       const uint64_t* d_offsets, const uint32_t* d_member,
                                                       const uint64_t* d_member_off, uint64_t n, uint64_t* d_found,
                                                       void* stream) {
  return set_probe(s, IN_VAR, d_bytes, d_offsets, 0, d_member, 0, d_member_off, n, d_found, stream, true);
}
extern "C" int rf_amd_filter_set_probe_hashes_ragged(rf_amd_filter_set* s, const uint32_t* d_hashes,
                                                     const uint32_t* d_member, const uint64_t* d_member_off,
                                                     uint64_t n, uint64_t* d_found, void* stream) {
  return set_probe(s, IN_HASH, d_hashes, nullptr, 4, d_member, 0, d_member_off, n, d_found, stream, true);
}

// the existence forms: the same calls with the n bytes d_exists in d_found's place
extern "C" int rf_amd_filter_set_exists_keys(rf_amd_filter_set* s, const void* d_keys, uint32_t key_len,
                                             const uint32_t* d_member, uint32_t K, uint64_t n, uint8_t* d_exists,
                                             void* stream) {
  if (!s) return fail(RF_AMD_EINVAL, "null filter set");
  if (key_len == 0) return fail(RF_AMD_EINVAL, "key_len 0");
  return set_probe(s, fixed_kind(d_keys, key_len), d_keys, nullptr, key_len, d_member, K, nullptr, n, d_exists,
                   stream, false, true);
}
extern "C" int rf_amd_filter_set_exists_var_keys(rf_amd_filter_set* s, const uint8_t* d_bytes,
                                                 const uint64_t* d_offsets, const uint32_t* d_member, uint32_t K,
                                                 uint64_t n, uint8_t* d_exists, void* stream) {
  return set_probe(s, IN_VAR, d_bytes, d_offsets, 0, d_member, K, nullptr, n, d_exists, stream, false, true);
}
extern "C" int rf_amd_filter_set_exists_hashes(rf_amd_filter_set* s, const uint32_t* d_hashes,
                                               const uint32_t* d_member, uint32_t K, uint64_t n, uint8_t* d_exists,
                                               void* stream) {
  return set_probe(s, IN_HASH, d_hashes, nullptr, 4, d_member, K, nullptr, n, d_exists, stream, false, true);
}
extern "C" int rf_amd_filter_set_exists_keys_ragged(rf_amd_filter_set* s, const void* d_keys, uint32_t key_len,
                                                    const uint32_t* d_member, const uint64_t* d_member_off,
                                                    uint64_t n, uint8_t* d_exists, void* stream) {
  if (!s) return fail(RF_AMD_EINVAL, "null filter set");
  if (key_len == 0) return fail(RF_AMD_EINVAL, "key_len 0");
  return set_probe(s, fixed_kind(d_keys, key_len), d_keys, nullptr, key_len, d_member, 0, d_member_off, n, d_exists,
                   stream, true, true);
}
extern "C" int rf_amd_filter_set_exists_var_keys_ragged(rf_amd_filter_set* s, const uint8_t* d_bytes,
                                                        const uint64_t* d_offsets, const uint32_t* d_member,
                                                        const uint64_t* d_member_off, uint64_t n, uint8_t* d_exists,
                                                        void* stream) {
  return set_probe(s, IN_VAR, d_bytes, d_offsets, 0, d_member, 0, d_member_off, n, d_exists, stream, true, true);
}
extern "C" int rf_amd_filter_set_exists_hashes_ragged(rf_amd_filter_set* s, const uint32_t* d_hashes,
                                                      const uint32_t* d_member, const uint64_t* d_member_off,
                                                      uint64_t n, uint8_t* d_exists, void* stream) {
  return set_probe(s, IN_HASH, d_hashes, nullptr, 4, d_member, 0, d_member_off, n, d_exists, stream, true, true);
}

extern "C" int rf_amd_diag_fanout_max_blocks(uint32_t blocks) {
  rf_fanout_set_max_blocks(blocks);
  rf_range_set_max_blocks(blocks);
  rf_per_key_set_max_blocks(blocks);
  rf_by_branch_set_max_blocks(blocks);
  rf_advance_set_max_blocks(blocks);
  return 0;
}

// 8 bytes of offset and 4 of count per tile of found words, and slack to keep both aligned
extern "C" uint64_t rf_amd_found_compact_scratch_bytes(uint64_t m) {
  return ((12 * rf_found_compact_tiles(m) + 15) & ~15ull) + 16;
}

extern "C" int rf_amd_found_compact(rf_amd_engine* e, const uint64_t* d_found, uint64_t m, uint64_t* d_cand,
                                    uint64_t cap, uint64_t* d_count, void* d_scratch, void* stream) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (!d_count) return fail(RF_AMD_EINVAL, "null count");
  if (m >= (1ull << 56)) return fail(RF_AMD_EINVAL, "m >= 2^56");
  if (m && (!d_found || !d_scratch)) return fail(RF_AMD_EINVAL, "null found words / scratch");
  if (m && cap && !d_cand) return fail(RF_AMD_EINVAL, "null candidate buffer");
  if ((uintptr_t)d_scratch & 7) return fail(RF_AMD_EINVAL, "scratch not 8-byte aligned");
  HIPCHK(hipSetDevice(e->device));
  (void)hipGetLastError();
  return launch_rc("compaction",
                   rf_launch_found_compact(stream_of(e, stream), d_found, m, d_cand, cap, d_count, d_scratch));
}

// ---- key-aware compaction: candidates with member ids and a CSR over the keys -----------------
// The sizing and the argument checks are rf_per_key_plan.h's, the kernels rf_per_key.hip's.
extern "C" uint64_t rf_amd_found_per_key_scratch_bytes(uint64_t n) { return per_key_scratch_bytes(n); }
extern "C" uint32_t rf_amd_diag_per_key_tile(void) { return PER_KEY_TILE; }

static int found_per_key(rf_amd_engine* e, bool ragged, const uint64_t* d_found, const uint32_t* d_member,
                         const uint64_t* d_member_off, uint32_t K, uint64_t n, uint64_t* d_key_off, uint64_t* d_cand,
                         uint64_t* d_cand_key, uint64_t cap, uint64_t* d_count, void* d_scratch, void* stream) {
  if (const char* m = per_key_refusal(ragged, e, d_found, d_member, d_member_off, K, n, d_key_off, d_cand, cap,
                                      d_count, d_scratch))
    return fail(RF_AMD_EINVAL, m);
  HIPCHK(hipSetDevice(e->device));
  (void)hipGetLastError();
  return launch_rc("per-key compaction",
                   rf_launch_found_per_key(stream_of(e, stream), d_found, d_member, d_member_off, K, n, d_key_off,
                                           d_cand, d_cand_key, cap, d_count, d_scratch));
}

extern "C" int rf_amd_found_per_key(rf_amd_engine* e, const uint64_t* d_found, const uint32_t* d_member, uint32_t K,
                                    uint64_t n, uint64_t* d_key_off, uint64_t* d_cand, uint64_t* d_cand_key,
                                    uint64_t cap, uint64_t* d_count, void* d_scratch, void* stream) {
  return found_per_key(e, false, d_found, d_member, nullptr, K, n, d_key_off, d_cand, d_cand_key, cap, d_count,
                       d_scratch, stream);
}
extern "C" int rf_amd_found_per_key_ragged(rf_amd_engine* e, const uint64_t* d_found, const uint32_t* d_member,
                                           const uint64_t* d_member_off, uint64_t n, uint64_t* d_key_off,
                                           uint64_t* d_cand, uint64_t* d_cand_key, uint64_t cap, uint64_t* d_count,
                                           void* d_scratch, void* stream) {
  return found_per_key(e, true, d_found, d_member, d_member_off, 0, n, d_key_off, d_cand, d_cand_key, cap, d_count,
                       d_scratch, stream);
}

// ---- group by branch: the per-key records in the order a batch's consumer walks the B-trees ---
// The sizing and the argument checks are rf_by_branch_plan.h's, the kernels rf_by_branch.hip's.
extern "C" uint64_t rf_amd_found_by_branch_scratch_bytes(uint64_t cap, uint32_t num_members) {
  return by_branch_scratch_bytes(cap, num_members);
}
extern "C" uint32_t rf_amd_diag_by_branch_tile(void) { return BY_BRANCH_TILE; }
extern "C" uint32_t rf_amd_diag_by_branch_passes(uint32_t num_members) {
  return num_members == 0 || num_members > BY_BRANCH_MAX_MEMBERS ? 0 : by_branch_passes(num_members);
}

extern "C" int rf_amd_found_by_branch(rf_amd_engine* e, const uint64_t* d_cand, const uint64_t* d_cand_key,
                                      const uint64_t* d_count, uint64_t cap, uint32_t num_members, uint32_t* d_order,
                                      uint64_t* d_order_key, uint64_t* d_branch, uint64_t* d_branch_off,
                                      uint64_t branch_cap, uint64_t* d_num_branches, void* d_scratch, void* stream) {
  if (const char* m = by_branch_refusal(e, d_cand, d_cand_key, d_count, cap, num_members, d_order, d_order_key,
                                        d_branch, d_branch_off, branch_cap, d_num_branches, d_scratch))
    return fail(RF_AMD_EINVAL, m);
  HIPCHK(hipSetDevice(e->device));
  (void)hipGetLastError();
  return launch_rc("group by branch",
                   rf_launch_found_by_branch(stream_of(e, stream), d_cand, d_cand_key, d_count, cap, num_members,
                                             d_order, d_order_key, d_branch, d_branch_off, branch_cap,
                                             d_num_branches, d_scratch));
}

// ---- stepwise hand-out: each open key's next records, in the form the grouping takes ----------
// The sizing and the argument checks are rf_advance_plan.h's, the kernels rf_advance.hip's.
static_assert(ADVANCE_FIRST == RF_AMD_ADVANCE_FIRST, "the plan's flag is the header's");
extern "C" uint64_t rf_amd_found_advance_scratch_bytes(uint64_t n) { return advance_scratch_bytes(n); }

extern "C" int rf_amd_found_advance(rf_amd_engine* e, const uint64_t* d_key_off, const uint64_t* d_cand,
                                    uint64_t cand_cap, uint64_t n, uint32_t width, uint32_t flags,
                                    const uint8_t* d_done, uint32_t* d_cursor, uint64_t* d_out_cand,
                                    uint64_t* d_out_key, uint64_t out_cap, uint64_t* d_out_count, void* d_scratch,
                                    void* stream) {
  if (const char* m = advance_refusal(e, d_key_off, d_cand, cand_cap, n, width, flags, d_cursor, d_out_cand, out_cap,
                                      d_out_count, d_scratch))
    return fail(RF_AMD_EINVAL, m);
  HIPCHK(hipSetDevice(e->device));
  (void)hipGetLastError();
  return launch_rc("stepwise hand-out",
                   rf_launch_found_advance(stream_of(e, stream), d_key_off, d_cand, cand_cap, n, width,
                                           (flags & ADVANCE_FIRST) != 0, d_done, d_cursor, d_out_cand, d_out_key,
                                           out_cap, d_out_count, d_scratch));
}

// ---- range maps: multi-get keys routed to their member lists --------------------------------
// The map is the planner's image (rf_range_plan.h) in one pool block, immutable; a route call is
// three launches over it and the caller's buffers (rf_range.hip). It holds no reference to any
// set or batch, and nothing downstream reads it: the route output is a copy.
// A map made from segments (rf_range_seg_plan.h) also keeps the segment sections' addresses, the
// capacities for the validation of an update, and the host scratch of an update call. One made
// with room (rf_range_split_plan.h) keeps both copies of the structural sections by address and
// the host state of its edits; dev and seg name the live copy.
struct rf_amd_range_map {
  rf_amd_engine* eng = nullptr;
  uint32_t num_ranges = 0, max_list = 0;
  DevBuf d_image;
  RangeDev dev{};
  bool segmented = false;
  RangeSegDev seg{};
  RangeSegState seg_state;
  RangeSegUpdatePlan upd_plan;
  RangeSegUpdate upd_args{};
  bool roomy = false;
  RangeStructDev copy[2]{};
  RangeSplitState split;
  RangeSplicePlan splice_plan;
  RangeSpliceArgs splice_args{};
};

// the image in one pool block by one copy on the engine stream, which is synchronised: the image
// is pageable, and route calls may run on any stream
static int range_map_upload(rf_amd_range_map* m, rf_amd_engine* e, const RangePlan& plan) {
  m->eng = e;
  m->num_ranges = plan.num_ranges;
  m->max_list = plan.max_list;
  if (m->d_image.alloc(plan.image.size(), &e->pool)) return RF_AMD_ENOMEM;
  HIPCHK(hipMemcpyAsync(m->d_image.p, plan.image.data(), plan.image.size(), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  const uint8_t* base = m->d_image.as<uint8_t>();
  m->dev.num_ranges = plan.num_ranges;
  m->dev.prefix = reinterpret_cast<const uint64_t*>(base + plan.o_prefix);
  m->dev.boff = reinterpret_cast<const uint64_t*>(base + plan.o_boff);
  m->dev.loff = reinterpret_cast<const uint64_t*>(base + plan.o_loff);
  m->dev.list = reinterpret_cast<const uint32_t*>(base + plan.o_list);
  m->dev.bytes = base + plan.o_bytes;
  return 0;
}

extern "C" int rf_amd_range_map_create(rf_amd_engine* e, uint32_t num_ranges, const uint8_t* h_bound_bytes,
                                       const uint64_t* h_bound_off, const uint32_t* h_list,
                                       const uint64_t* h_list_off, rf_amd_range_map** out) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (!out) return fail(RF_AMD_EINVAL, "null out-param");
  *out = nullptr;
  RangePlan plan;
  std::string msg;
  if (int rc = plan_range_map(num_ranges, h_bound_bytes, h_bound_off, h_list, h_list_off, &plan, &msg))
    return fail(rc, msg);
  HIPCHK(hipSetDevice(e->device));
  auto m = std::make_unique<rf_amd_range_map>();
  if (int rc = range_map_upload(m.get(), e, plan)) return rc;
  *out = m.release();
  return 0;
}

extern "C" int rf_amd_range_map_create_segments(rf_amd_engine* e, uint32_t num_ranges, const uint8_t* h_bound_bytes,
                                                const uint64_t* h_bound_off, const uint32_t* h_path,
                                                const uint64_t* h_path_off, uint32_t num_segments,
                                                const uint32_t* h_seg_cap, const uint32_t* h_seg_ids,
                                                const uint64_t* h_seg_off, rf_amd_range_map** out) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (!out) return fail(RF_AMD_EINVAL, "null out-param");
  *out = nullptr;
  RangeSegPlan plan;
  std::string msg;
  if (int rc = plan_range_map_segments(num_ranges, h_bound_bytes, h_bound_off, h_path, h_path_off, num_segments,
                                       h_seg_cap, h_seg_ids, h_seg_off, &plan, &msg))
    return fail(rc, msg);
  HIPCHK(hipSetDevice(e->device));
  auto m = std::make_unique<rf_amd_range_map>();
  m->segmented = true;
  m->seg_state.init(h_seg_cap, num_segments);
  if (int rc = range_map_upload(m.get(), e, plan)) return rc;
  m->seg = range_seg_dev(plan, m->d_image.as<uint8_t>());
  m->upd_args.slots = m->seg.slots;
  m->upd_args.slen = m->seg.slen;
  m->upd_args.sbase = m->seg.sbase;
  m->upd_args.scap = m->seg.scap;
  m->upd_args.num_segments = num_segments;
  *out = m.release();
  return 0;
}

extern "C" int rf_amd_range_map_create_segments_room(rf_amd_engine* e, uint32_t num_ranges,
                                                     const uint8_t* h_bound_bytes, const uint64_t* h_bound_off,
                                                     const uint32_t* h_path, const uint64_t* h_path_off,
                                                     uint32_t num_segments, const uint32_t* h_seg_cap,
                                                     const uint32_t* h_seg_ids, const uint64_t* h_seg_off,
                                                     const rf_amd_range_room* room, rf_amd_range_map** out) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (!out) return fail(RF_AMD_EINVAL, "null out-param");
  *out = nullptr;
  RangeRoomPlan plan;
  std::string msg;
  if (int rc = plan_range_map_segments_room(num_ranges, h_bound_bytes, h_bound_off, h_path, h_path_off, num_segments,
                                            h_seg_cap, h_seg_ids, h_seg_off, room, &plan, &msg))
    return fail(rc, msg);
  HIPCHK(hipSetDevice(e->device));
  auto m = std::make_unique<rf_amd_range_map>();
  m->segmented = m->roomy = true;
  m->seg_state.init(h_seg_cap, num_segments);
  m->split.init(*room, num_ranges, h_bound_bytes, h_bound_off, h_path, h_path_off, h_seg_cap);
  if (int rc = range_map_upload(m.get(), e, plan)) return rc;
  uint8_t* base = m->d_image.as<uint8_t>();
  m->seg = range_seg_dev(plan, base);
  m->copy[0] = range_struct_dev(plan, base, 0);
  m->copy[1] = range_struct_dev(plan, base, 1);
  m->upd_args.slots = m->seg.slots;
  m->upd_args.slen = m->seg.slen;
  m->upd_args.sbase = m->seg.sbase;
  m->upd_args.scap = m->seg.scap;
  m->upd_args.num_segments = num_segments;
  *out = m.release();
  return 0;
}

// Segment lists replaced in stream order: every entry is validated and the call cut into launches
// on the host (rf_range_seg_plan.h) before the first launch; the scatter launches carry the ids
// in their arguments, then the flatten rewrites the flat table the route kernels read. Nothing
// is waited for and nothing allocated on the device. The call's host scratch lives in the map,
// so the caller serialises calls on one map. A launch the runtime refuses leaves the segments
// and the flat table out of step: the map is then good only for destroy (rf_amd.h).
extern "C" int rf_amd_range_map_update_segments(rf_amd_range_map* m, const uint32_t* seg_id, const uint32_t* h_ids,
                                                const uint64_t* h_ids_off, uint32_t count, void* stream) {
  if (!m) return fail(RF_AMD_EINVAL, "null range map");
  if (!m->segmented) return fail(RF_AMD_EINVAL, "a flat range map has no segments");
  if (count == 0) return 0;
  std::string msg;
  if (int rc = plan_range_seg_update(&m->seg_state, count, seg_id, h_ids, h_ids_off, &m->upd_plan, &msg))
    return fail(rc, msg);
  HIPCHK(hipSetDevice(m->eng->device));
  (void)hipGetLastError();
  hipStream_t st = stream_of(m->eng, stream);
  for (uint32_t l = 0; l < m->upd_plan.launches(); l++) {
    range_seg_fill_launch(m->upd_plan, l, h_ids, &m->upd_args);
    if (int rc = launch_rc("segment update", rf_launch_range_seg_scatter(st, &m->upd_args))) return rc;
  }
  return launch_rc("segment flatten", rf_launch_range_seg_flatten(st, &m->seg));
}

// An edit whose plan the host has accepted, in stream order: the splice launches read the copy
// that was live and write the other, which the route launches and the flatten are given from here
// on; then the flatten. The copy that route calls already queued read is not written before the
// next edit. Nothing is waited for and nothing allocated; the call's host scratch lives in the map.
static int range_map_splice(rf_amd_range_map* m, const uint8_t* h_bound_bytes, const uint64_t* h_bound_off,
                            const uint32_t* h_path, const uint64_t* h_path_off, void* stream) {
  HIPCHK(hipSetDevice(m->eng->device));
  (void)hipGetLastError();
  hipStream_t st = stream_of(m->eng, stream);
  const RangeStructDev& to = m->copy[m->split.live];
  m->splice_args.src = m->copy[m->split.live ^ 1u];
  m->splice_args.dst = to;
  m->num_ranges = m->dev.num_ranges = m->seg.num_ranges = m->splice_plan.e.r_new;
  m->dev.prefix = to.prefix;
  m->dev.boff = to.boff;
  m->dev.bytes = to.bytes;
  m->seg.poff = to.poff;
  m->seg.path = to.path;
  for (uint32_t l = 0; l < m->splice_plan.launches(); l++) {
    range_splice_fill_launch(m->splice_plan, l, h_bound_bytes, h_bound_off, h_path, h_path_off, &m->splice_args);
    if (int rc = launch_rc("range splice", rf_launch_range_splice(st, &m->splice_args))) return rc;
  }
  return launch_rc("segment flatten", rf_launch_range_seg_flatten(st, &m->seg));
}

static int range_map_roomy(const rf_amd_range_map* m) {
  if (!m) return fail(RF_AMD_EINVAL, "null range map");
  if (!m->segmented) return fail(RF_AMD_EINVAL, "a flat range map has no paths");
  if (!m->roomy) return fail(RF_AMD_EINVAL, "a range map created without room");
  return 0;
}

extern "C" int rf_amd_range_map_split(rf_amd_range_map* m, uint32_t range, uint32_t pieces,
                                      const uint8_t* h_bound_bytes, const uint64_t* h_bound_off,
                                      const uint32_t* h_path, const uint64_t* h_path_off, void* stream) {
  if (int rc = range_map_roomy(m)) return rc;
  std::string msg;
  if (int rc = plan_range_split(&m->split, m->seg_state, range, pieces, h_bound_bytes, h_bound_off, h_path,
                                h_path_off, &m->splice_plan, &msg))
    return fail(rc, msg);
  return range_map_splice(m, h_bound_bytes, h_bound_off, h_path, h_path_off, stream);
}

extern "C" int rf_amd_range_map_set_paths(rf_amd_range_map* m, uint32_t first, uint32_t count, const uint32_t* h_path,
                                          const uint64_t* h_path_off, void* stream) {
  if (int rc = range_map_roomy(m)) return rc;
  if (count == 0 && first <= m->num_ranges) return 0;
  std::string msg;
  if (int rc = plan_range_set_paths(&m->split, m->seg_state, first, count, h_path, h_path_off, &m->splice_plan, &msg))
    return fail(rc, msg);
  return range_map_splice(m, nullptr, nullptr, h_path, h_path_off, stream);
}

// synchronises the device (route calls on a caller's stream may still read the image), as
// rf_amd_filter_set_destroy does
extern "C" void rf_amd_range_map_destroy(rf_amd_range_map* m) {
  if (!m) return;
  (void)hipSetDevice(m->eng->device);
  (void)hipDeviceSynchronize();
  delete m;
}

// stream-ordered destroy, as rf_amd_filter_set_destroy_on: the image's block is parked behind an
// event recorded on `stream`. Returns without waiting.
extern "C" int rf_amd_range_map_destroy_on(rf_amd_range_map* m, void* stream) {
  if (!m) return 0;
  HIPCHK(hipSetDevice(m->eng->device));
  DevBuf* const image = &m->d_image;
  if (park_behind(m->eng, stream_of(m->eng, stream), &image, 1)) delete m;
  else rf_amd_range_map_destroy(m);  // fall back to the synchronising destroy
  return 0;
}

extern "C" uint32_t rf_amd_range_map_num_ranges(const rf_amd_range_map* m) { return m ? m->num_ranges : 0; }
extern "C" uint32_t rf_amd_range_map_max_list(const rf_amd_range_map* m) { return m ? m->max_list : 0; }
extern "C" uint32_t rf_amd_range_map_num_segments(const rf_amd_range_map* m) {
  return m && m->segmented ? m->seg.num_segments : 0;
}
extern "C" uint32_t rf_amd_diag_range_seg_launch_ids(void) { return RANGE_SEG_LAUNCH_IDS; }
extern "C" uint32_t rf_amd_diag_range_seg_thread_ids(void) { return RANGE_SEG_THREAD_IDS; }
extern "C" uint32_t rf_amd_diag_range_splice_words(void) { return RANGE_SPLICE_WORDS; }
extern "C" uint64_t rf_amd_range_route_scratch_bytes(uint64_t n) { return range_route_scratch_bytes(n); }
extern "C" uint32_t rf_amd_diag_range_lds_ranges(void) { return RANGE_LDS_RANGES; }
extern "C" uint32_t rf_amd_diag_range_tile(void) { return RANGE_TILE; }

static int range_route(rf_amd_range_map* m, int var, const uint8_t* in0, const uint64_t* offs, uint32_t key_len,
                       uint64_t n, uint32_t* d_range, uint64_t* d_member_off, uint32_t* d_member, uint64_t pair_cap,
                       uint64_t* d_total, void* d_scratch, void* stream) {
  if (!m) return fail(RF_AMD_EINVAL, "null range map");
  if (n >= (1ull << 56)) return fail(RF_AMD_EINVAL, "n >= 2^56");
  if (!d_member_off || !d_total) return fail(RF_AMD_EINVAL, "null member offsets / total");
  if (n && (!in0 || (var && !offs) || !d_range || !d_scratch)) return fail(RF_AMD_EINVAL, "null route buffer");
  if (n && pair_cap && !d_member) return fail(RF_AMD_EINVAL, "null member buffer");
  if ((uintptr_t)d_scratch & 7) return fail(RF_AMD_EINVAL, "scratch not 8-byte aligned");
  HIPCHK(hipSetDevice(m->eng->device));
  (void)hipGetLastError();
  return launch_rc("range route",
                   rf_launch_range_route(stream_of(m->eng, stream), var, in0, offs, key_len, n, &m->dev, d_range,
                                         d_member_off, d_member, pair_cap, d_total, d_scratch));
}

extern "C" int rf_amd_range_map_route_keys(rf_amd_range_map* m, const void* d_keys, uint32_t key_len, uint64_t n,
                                           uint32_t* d_range, uint64_t* d_member_off, uint32_t* d_member,
                                           uint64_t pair_cap, uint64_t* d_total, void* d_scratch, void* stream) {
  if (key_len == 0) return fail(RF_AMD_EINVAL, "key_len 0");
  return range_route(m, 0, static_cast<const uint8_t*>(d_keys), nullptr, key_len, n, d_range, d_member_off,
                     d_member, pair_cap, d_total, d_scratch, stream);
}
extern "C" int rf_amd_range_map_route_var_keys(rf_amd_range_map* m, const uint8_t* d_bytes,
                                               const uint64_t* d_offsets, uint64_t n, uint32_t* d_range,
                                               uint64_t* d_member_off, uint32_t* d_member, uint64_t pair_cap,
                                               uint64_t* d_total, void* d_scratch, void* stream) {
  return range_route(m, 1, d_bytes, d_offsets, 0, n, d_range, d_member_off, d_member, pair_cap, d_total,
                     d_scratch, stream);
}

static int do_probe(rf_amd_batch* b, int kind, const void* in0, const uint64_t* offs, uint32_t key_len,
                    const uint32_t* fid, uint64_t n, uint64_t* found, void* stream,
                    const uint64_t* d_runs) {
  if (!b || !b->built) return fail(RF_AMD_EINVAL, "probe on an unbuilt batch");
  if (n && (!in0 || !(fid || d_runs) || !found)) return fail(RF_AMD_EINVAL, "null probe buffer");
  HIPCHK(hipSetDevice(b->eng->device));
  hipStream_t st = stream_of(b->eng, stream);
  (void)hipGetLastError();
  LaunchArgs a = make_args(b, st);
  a.probe_runs = d_runs;
  a.wave_tab = d_runs ? b->d_wave_tab.as<uint32_t>() : nullptr;
  return launch_rc("probe", rf_launch_probe(&a, kind, in0, offs, key_len, fid, n, found));
}

extern "C" int rf_amd_batch_probe_keys(rf_amd_batch* b, const void* d_keys, uint32_t key_len,
                                       const uint32_t* d_filter_id, uint64_t n, uint64_t* d_found, void* stream) {
  if (key_len == 0) return fail(RF_AMD_EINVAL, "key_len 0");
  return do_probe(b, fixed_kind(d_keys, key_len), d_keys, nullptr, key_len, d_filter_id, n, d_found, stream);
}
extern "C" int rf_amd_batch_probe_var_keys(rf_amd_batch* b, const uint8_t* d_bytes, const uint64_t* d_offsets,
                                           const uint32_t* d_filter_id, uint64_t n, uint64_t* d_found,
                                           void* stream) {
  return do_probe(b, IN_VAR, d_bytes, d_offsets, 0, d_filter_id, n, d_found, stream);
}
extern "C" int rf_amd_batch_probe_hashes(rf_amd_batch* b, const uint32_t* d_hashes, const uint32_t* d_filter_id,
                                         uint64_t n, uint64_t* d_found, void* stream) {
  return do_probe(b, IN_HASH, d_hashes, nullptr, 4, d_filter_id, n, d_found, stream);
}

// Probes grouped by filter (filter f's h_counts[f] probes follow filter f-1's): the filter of
// a probe comes from its position, so no per-probe filter id is read. The run bounds are
// uploaded when they change.
static int upload_runs(rf_amd_batch* b, const uint64_t* h_counts, void* stream, uint64_t* n_out) {
  if (!b || !b->built) return fail(RF_AMD_EINVAL, "probe on an unbuilt batch");
  if (!h_counts) return fail(RF_AMD_EINVAL, "null counts");
  std::vector<uint64_t> runs(b->F + 1, 0);
  for (uint32_t f = 0; f < b->F; f++) runs[f + 1] = runs[f] + h_counts[f];
  const uint64_t n = runs[b->F];
  *n_out = n;
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(b->eng->device));
  if (runs != b->runs_host) {
    if (!b->d_runs.p && b->d_runs.alloc(8ull * (b->F + 1), &b->eng->pool)) return RF_AMD_ENOMEM;
    hipStream_t st = stream_of(b->eng, stream);
    HIPCHK(hipStreamSynchronize(st));  // earlier probes may still read the old bounds
    const uint64_t nw = (n + 63) / 64;
    if (b->d_wave_tab.n < 4 * nw && b->d_wave_tab.alloc(4 * nw, &b->eng->pool)) return RF_AMD_ENOMEM;
    HIPCHK(hipMemcpyAsync(b->d_runs.p, runs.data(), 8ull * (b->F + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    if (rf_launch_wave_tab(st, b->d_runs.as<uint64_t>(), b->F, n, b->d_wave_tab.as<uint32_t>()))
      return fail(RF_AMD_EINVAL, "wave table launch failed");
    b->runs_host = runs;
  }
  return 0;
}

static int probe_runs(rf_amd_batch* b, int kind, const void* in0, const uint64_t* offs, uint32_t key_len,
                      const uint64_t* h_counts, uint64_t* d_found, void* stream) {
  uint64_t n = 0;
  if (int rc = upload_runs(b, h_counts, stream, &n)) return rc;
  if (n == 0) return 0;
  if (kind == IN_VAR && !offs) return fail(RF_AMD_EINVAL, "null probe buffer");
  return do_probe(b, kind, in0, offs, key_len, nullptr, n, d_found, stream, b->d_runs.as<uint64_t>());
}

// bench.py's measured probe floor: k_probe_floor over the same runs (rf_amd_diag.h)
extern "C" int rf_amd_debug_probe_floor(rf_amd_batch* b, const void* d_in, uint32_t key_len, const uint64_t* h_counts,
                                        uint64_t* d_out, void* stream) {
  if (key_len != 24 && key_len != 4) return fail(RF_AMD_EINVAL, "probe floor: 24-byte keys or 4-byte hashes");
  if (!d_in || !d_out) return fail(RF_AMD_EINVAL, "null probe buffer");
  if (key_len == 24 && ((uintptr_t)d_in & 15)) return fail(RF_AMD_EINVAL, "probe floor: keys 16-byte aligned");
  uint64_t n = 0;
  if (int rc = upload_runs(b, h_counts, stream, &n)) return rc;
  if (n == 0) return 0;
  hipStream_t st = stream_of(b->eng, stream);
  (void)hipGetLastError();
  LaunchArgs a = make_args(b, st);
  a.probe_runs = b->d_runs.as<uint64_t>();
  a.wave_tab = b->d_wave_tab.as<uint32_t>();
  return launch_rc("probe floor", rf_launch_probe_floor(&a, key_len == 24 ? IN_KEYS24 : IN_HASH, d_in, n, d_out));
}

extern "C" int rf_amd_batch_probe_keys_runs(rf_amd_batch* b, const void* d_keys, uint32_t key_len,
                                            const uint64_t* h_counts, uint64_t* d_found, void* stream) {
  if (key_len == 0) return fail(RF_AMD_EINVAL, "key_len 0");
  return probe_runs(b, fixed_kind(d_keys, key_len), d_keys, nullptr, key_len, h_counts, d_found, stream);
}
extern "C" int rf_amd_batch_probe_var_keys_runs(rf_amd_batch* b, const uint8_t* d_bytes, const uint64_t* d_offsets,
                                                const uint64_t* h_counts, uint64_t* d_found, void* stream) {
  return probe_runs(b, IN_VAR, d_bytes, d_offsets, 0, h_counts, d_found, stream);
}
extern "C" int rf_amd_batch_probe_hashes_runs(rf_amd_batch* b, const uint32_t* d_hashes, const uint64_t* h_counts,
                                              uint64_t* d_found, void* stream) {
  return probe_runs(b, IN_HASH, d_hashes, nullptr, 4, h_counts, d_found, stream);
}

extern "C" int rf_amd_debug_phase_buffer(void* d_buf, uint32_t kernel) {
#ifdef RF_PHASE_STAMPS
  return rf_debug_set_phase_buffer(static_cast<uint64_t*>(d_buf), kernel) ? fail(RF_AMD_EINVAL, "phase buffer") : 0;
#else
  (void)kernel;
  return d_buf ? fail(RF_AMD_EINVAL, "phase stamps exist only in the diagnostics library") : 0;
#endif
}

extern "C" int rf_amd_debug_read_lines(rf_amd_batch* b, uint8_t* h_lines, uint64_t bytes, uint64_t* num_lines) {
  if (!b || !b->built) return fail(RF_AMD_EINVAL, "unbuilt batch");
  if (num_lines) *num_lines = b->NL;
  if (!h_lines) return 0;
  if (bytes < 64ull * b->NL) return fail(RF_AMD_EINVAL, "lines buffer too small");
  HIPCHK(hipSetDevice(b->eng->device));
  if (int rc = wait_built(b)) return rc;
  HIPCHK(hipMemcpyAsync(h_lines, b->d_lines.p, 64ull * b->NL, hipMemcpyDeviceToHost, b->eng->stream));
  HIPCHK(hipStreamSynchronize(b->eng->stream));
  return 0;
}

extern "C" int rf_amd_debug_rebuild_lines(rf_amd_batch* b) {
  if (!b || !b->built) return fail(RF_AMD_EINVAL, "unbuilt batch");
  HIPCHK(hipSetDevice(b->eng->device));
  if (int rc = wait_built(b)) return rc;
  (void)hipGetLastError();
  LaunchArgs a = make_args(b, b->eng->stream);
  a.plines_force = 1;  // every filter, also those whose lines K6 cut
  if (int rc = launch_rc("probe-line", rf_launch_plines(&a))) return rc;
  HIPCHK(hipStreamSynchronize(b->eng->stream));
  return 0;
}

extern "C" int rf_amd_batch_set_timing(rf_amd_batch* b, int enable) {
  if (!b) return fail(RF_AMD_EINVAL, "null batch");
  HIPCHK(hipSetDevice(b->eng->device));
  for (auto ev : b->events) (void)hipEventDestroy(ev);
  b->events.clear();
  b->ev_sets = b->ev_set = 0;
  b->ev_mask = enable < 0 ? EV_MASK_PROBE : EV_MASK_ALL;
  if (enable < 0) enable = -enable;
  if (enable > 0) {
    b->events.resize((size_t)NUM_EVENTS * enable);
    for (auto& ev : b->events) HIPCHK(hipEventCreate(&ev));
    b->ev_sets = (uint32_t)enable;
  }
  return 0;
}
extern "C" int rf_amd_batch_timings_back(rf_amd_batch* b, uint32_t back, float* ms, uint32_t n) {
  if (!b || b->events.empty() || !ms || n < RF_AMD_NUM_TIMINGS) return fail(RF_AMD_EINVAL, "timing not enabled");
  if (back >= b->ev_sets) return fail(RF_AMD_EINVAL, "timing set out of range");
  HIPCHK(hipSetDevice(b->eng->device));
  const hipEvent_t* ev = b->events.data() + (size_t)((b->ev_set + b->ev_sets - back) % b->ev_sets) * NUM_EVENTS;
  static const int pairs[RF_AMD_NUM_TIMINGS][2] = {
      {EV_B_START, EV_B_HASH},    {EV_B_HASH, EV_B_SCAN},     {EV_B_SCAN, EV_B_SCATTER},
      {EV_B_SCATTER, EV_B_SORT},  {EV_B_SORT, EV_B_SORT_BIG}, {EV_B_SORT_BIG, EV_B_LAYOUT},
      {EV_B_LAYOUT, EV_B_ASSEMBLE}, {EV_B_START, EV_B_ASSEMBLE}, {EV_P_START, EV_P_END}};
  for (uint32_t i = 0; i < RF_AMD_NUM_TIMINGS; i++) {
    ms[i] = -1.f;
    if (!(b->ev_mask >> pairs[i][0] & 1u) || !(b->ev_mask >> pairs[i][1] & 1u)) continue;  // not recorded
    if (hipEventSynchronize(ev[pairs[i][1]]) != hipSuccess) continue;
    float t = 0;
    if (hipEventElapsedTime(&t, ev[pairs[i][0]], ev[pairs[i][1]]) == hipSuccess) ms[i] = t;
  }
  (void)hipGetLastError();  // a stage not run yet (e.g. no probe) must not poison later launches
  return 0;
}
extern "C" int rf_amd_batch_timings(rf_amd_batch* b, float* ms, uint32_t n) {
  return rf_amd_batch_timings_back(b, 0, ms, n);
}

extern "C" int rf_amd_batch_info(rf_amd_batch* b, uint32_t f, rf_amd_filter_info* out) {
  if (!b || f >= b->F || !out) return fail(RF_AMD_EINVAL, "bad batch/filter");
  HIPCHK(hipSetDevice(b->eng->device));
  FilterOut o;
  if (int rc = wait_built(b)) return rc;
  hipStream_t st = b->eng->stream;
  HIPCHK(hipMemcpyAsync(&o, b->d_outs.as<FilterOut>() + f, sizeof(o), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const FilterPlan& p = b->plans[f];
  out->num_fingerprints = p.num_fp;
  out->num_unique = o.num_unique;
  out->value_size = p.vs;
  out->num_indices = p.num_indices;
  out->num_pages = o.num_pages;
  out->error = o.error;
  return 0;
}

// every filter's info with one copy (rf_amd_batch_info per filter synchronises F times)
extern "C" int rf_amd_batch_infos(rf_amd_batch* b, rf_amd_filter_info* out, void* stream) {
  if (!b || !out) return fail(RF_AMD_EINVAL, "bad batch");
  HIPCHK(hipSetDevice(b->eng->device));
  std::vector<FilterOut> o(b->F);
  if (stream) {  // the build was issued on `stream`: wait for it alone
    HIPCHK(hipMemcpyAsync(o.data(), b->d_outs.p, sizeof(FilterOut) * b->F, hipMemcpyDeviceToHost,
                          (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  } else {  // wherever the build ran: its event, then a copy on the engine stream
    if (int rc = wait_built(b)) return rc;
    HIPCHK(hipMemcpyAsync(o.data(), b->d_outs.p, sizeof(FilterOut) * b->F, hipMemcpyDeviceToHost, b->eng->stream));
    HIPCHK(hipStreamSynchronize(b->eng->stream));
  }
  {
    std::lock_guard<std::mutex> lk(b->err_mu);
    b->err_host.resize(b->F);
    for (uint32_t f = 0; f < b->F; f++) b->err_host[f] = o[f].error;
    b->err_ready.store(true, std::memory_order_release);
  }
  for (uint32_t f = 0; f < b->F; f++) {
    const FilterPlan& p = b->plans[f];
    out[f].num_fingerprints = p.num_fp;
    out[f].num_unique = o[f].num_unique;
    out[f].value_size = p.vs;
    out[f].num_indices = p.num_indices;
    out[f].num_pages = o[f].num_pages;
    out[f].error = o[f].error;
  }
  return 0;
}

extern "C" int rf_amd_batch_read_image(rf_amd_batch* b, uint32_t f, uint8_t* h_pages, uint64_t pages_bytes,
                                       uint64_t* h_slots, uint32_t num_slots) {
  rf_amd_filter_info info;
  if (int rc = rf_amd_batch_info(b, f, &info)) return rc;
  if (info.error) return fail(RF_AMD_EINVAL, "filter build reported error bits");
  const FilterPlan& p = b->plans[f];
  const uint64_t need = (uint64_t)info.num_pages * b->cfg.page_size;
  hipStream_t st = b->eng->stream;  // after rf_amd_batch_info waited for the build
  if (h_pages) {
    if (pages_bytes < need) return fail(RF_AMD_EINVAL, "pages buffer too small");
    HIPCHK(hipMemcpyAsync(h_pages, b->d_pages.as<uint8_t>() + (uint64_t)p.page_base * b->cfg.page_size, need,
                          hipMemcpyDeviceToHost, st));
  }
  if (h_slots) {
    if (num_slots < p.num_indices) return fail(RF_AMD_EINVAL, "slots buffer too small");
    HIPCHK(hipMemcpyAsync(h_slots, b->d_slots.as<uint64_t>() + p.idx_base, 8ull * p.num_indices,
                          hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int rf_amd_batch_read_image_async(rf_amd_batch* b, uint32_t f, void* h_pages, uint64_t pages_bytes,
                                             void* h_slots, uint32_t num_slots, void* stream) {
  if (!b || f >= b->F) return fail(RF_AMD_EINVAL, "bad batch/filter");
  const FilterPlan& p = b->plans[f];
  if (pages_bytes > (uint64_t)p.page_cap * b->cfg.page_size || num_slots > p.num_indices)
    return fail(RF_AMD_EINVAL, "copy larger than the filter's reservation");
  HIPCHK(hipSetDevice(b->eng->device));
  hipStream_t st = stream_of(b->eng, stream);
  if (h_pages && pages_bytes)
    HIPCHK(hipMemcpyAsync(h_pages, b->d_pages.as<uint8_t>() + (uint64_t)p.page_base * b->cfg.page_size,
                          pages_bytes, hipMemcpyDeviceToHost, st));
  if (h_slots && num_slots)
    HIPCHK(hipMemcpyAsync(h_slots, b->d_slots.as<uint64_t>() + p.idx_base, 8ull * num_slots,
                          hipMemcpyDeviceToHost, st));
  return 0;
}

extern "C" int rf_amd_batch_image_ptrs(rf_amd_batch* b, uint32_t f, void** d_pages, void** d_slots) {
  if (!b || f >= b->F) return fail(RF_AMD_EINVAL, "bad batch/filter");
  const FilterPlan& p = b->plans[f];
  if (d_pages) *d_pages = b->d_pages.as<uint8_t>() + (uint64_t)p.page_base * b->cfg.page_size;
  if (d_slots) *d_slots = b->d_slots.as<uint64_t>() + p.idx_base;
  return 0;
}

// ---- image batches: images (host or device) imported as a built, probe-only batch --------
// Filter f's pages are the num_pages[f] * page_size bytes after those of filters < f in
// `pages`, its index slots (relocatable, filter-relative) the num_indices[f] u64 after
// those of filters < f in `slots`. Probe lines are cut from the images by k_plines.
// batch_import, steps 3b and 4: uploads, the probe lines' kernel, and the wait for them. On
// failure work may still be queued (reading outs / idx_filter, the caller's host vectors).
static int import_enqueue(rf_amd_batch* b, const std::vector<FilterOut>& outs, const std::vector<uint32_t>& idx_filter,
                          const void* pages, const uint64_t* slots, hipMemcpyKind kind) {
  const uint32_t F = b->F;
  const size_t page_bytes = (size_t)b->PS * b->cfg.page_size;
  hipStream_t st = b->eng->stream;
  HIPCHK(hipMemcpyAsync(b->d_outs.p, outs.data(), sizeof(FilterOut) * F, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(b->d_pages.as<uint8_t>() + page_bytes, 0, 256, st));
  HIPCHK(hipMemcpyAsync(b->d_pages.p, pages, page_bytes, kind, st));
  HIPCHK(hipMemcpyAsync(b->d_slots.p, slots, 8ull * b->I, kind, st));
  HIPCHK(hipMemcpyAsync(b->d_idx_filter.p, idx_filter.data(), 4ull * b->I, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->d_plans.p, b->plans.data(), sizeof(FilterPlan) * F, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->d_pplans.p, b->pplans.data(), 16ull * F, hipMemcpyHostToDevice, st));
  {
    LaunchArgs a = make_args(b, st);
    note_dense_lines(b);
    if (int lrc = launch_rc("probe-line", rf_launch_plines(&a))) return lrc;
  }
  HIPCHK(hipStreamSynchronize(st));
  return note_built(b, st);
}

// Four steps, as batch_create: check and plan (rf_batch_plan.h), allocate, upload, launch and
// synchronise.
static int batch_import(rf_amd_engine* e, const rf_amd_config* cfg, uint32_t F, const rf_amd_filter_info* infos,
                        const void* pages, const uint64_t* slots, hipMemcpyKind kind, rf_amd_batch** out) {
  if (int rc = check_cfg(cfg)) return rc;
  if (F == 0 || !infos || !pages || !slots) return fail(RF_AMD_EINVAL, "bad image");
  auto b = std::make_unique<rf_amd_batch>();
  std::string msg;
  if (int rc = plan_import(cfg, F, infos, plan_knobs_env(), b.get(), &msg)) return fail(rc, msg);
  b->eng = e;
  b->cfg = *cfg;

  HIPCHK(hipSetDevice(e->device));
  DevPool* pool = &e->pool;
  int rc = b->d_plans.alloc(sizeof(FilterPlan) * F, pool);
  rc |= b->d_pplans.alloc(16ull * F, pool);
  rc |= b->d_pages.alloc((size_t)b->PS * cfg->page_size + 256, pool);
  rc |= b->d_slots.alloc(8ull * b->I, pool);
  rc |= b->d_lines.alloc(64ull * b->NL + 64, pool);
  rc |= b->d_idx_filter.alloc(4ull * b->I, pool);
  rc |= b->d_outs.alloc(sizeof(FilterOut) * F, pool);
  if (rc) return fail(RF_AMD_ENOMEM, "device allocation failed");

  std::vector<FilterOut> outs(F);
  std::vector<uint32_t> idx_filter;
  idx_filter.reserve(b->I);
  for (uint32_t f = 0; f < F; f++) {
    outs[f] = FilterOut{infos[f].num_unique, infos[f].num_pages, 0u, 0u};
    idx_filter.insert(idx_filter.end(), b->plans[f].num_indices, f);
  }
  if (int erc = import_enqueue(b.get(), outs, idx_filter, pages, slots, kind)) {
    (void)hipStreamSynchronize(e->stream);  // queued copies may still read the vectors above
    return erc;
  }
  b->err_host.assign(F, 0u);  // imports carry no error bits (checked by the planner)
  b->err_ready.store(true, std::memory_order_release);
  b->built = true;
  *out = b.release();
  return 0;
}

static int batch_from_image(rf_amd_engine* e, const rf_amd_config* cfg, const rf_amd_image* img,
                            rf_amd_batch** out) {
  if (!img || !img->pages || !img->slots || img->info.num_fingerprints == 0)
    return fail(RF_AMD_EINVAL, "bad image");
  return batch_import(e, cfg, 1, &img->info, img->pages, img->slots, hipMemcpyHostToDevice, out);
}

extern "C" int rf_amd_batch_export(rf_amd_batch* b, void* d_pages, uint64_t pages_bytes, uint64_t* d_slots,
                                   uint64_t num_slots, void* stream) {
  if (!b || !b->built) return fail(RF_AMD_EINVAL, "export of an unbuilt batch");
  uint64_t po = 0, so = 0;
  std::vector<rf_amd_filter_info> inf(b->F);
  for (uint32_t f = 0; f < b->F; f++) {
    if (int rc = rf_amd_batch_info(b, f, &inf[f])) return rc;
    if (inf[f].error) return fail(RF_AMD_EINVAL, "filter build reported error bits");
    po += (uint64_t)inf[f].num_pages * b->cfg.page_size;
    so += inf[f].num_indices;
  }
  if (!d_pages || !d_slots || pages_bytes < po || num_slots < so) return fail(RF_AMD_EINVAL, "export buffers too small");
  hipStream_t st = stream_of(b->eng, stream);
  po = so = 0;
  for (uint32_t f = 0; f < b->F; f++) {
    const FilterPlan& p = b->plans[f];
    const uint64_t pb = (uint64_t)inf[f].num_pages * b->cfg.page_size;
    HIPCHK(hipMemcpyAsync(static_cast<uint8_t*>(d_pages) + po,
                          b->d_pages.as<uint8_t>() + (uint64_t)p.page_base * b->cfg.page_size, pb,
                          hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(d_slots + so, b->d_slots.as<uint64_t>() + p.idx_base, 8ull * p.num_indices,
                          hipMemcpyDeviceToDevice, st));
    po += pb;
    so += p.num_indices;
  }
  return 0;
}

extern "C" int rf_amd_batch_import(rf_amd_engine* e, const rf_amd_config* cfg, uint32_t num_filters,
                                   const rf_amd_filter_info* infos, const void* pages, const uint64_t* slots,
                                   int device_resident, rf_amd_batch** out) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (!out) return fail(RF_AMD_EINVAL, "null out-param");
  *out = nullptr;
  return batch_import(e, cfg, num_filters, infos, pages, slots,
                      device_resident ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, out);
}

// rf_amd_filter_add (num_runs == 0: the one run new_fp_arrs[0], num_new_fp[0], values[0], which
// may be empty) and rf_amd_filter_add_runs
static int filter_add_runs(rf_amd_engine* e, const rf_amd_config* cfg, const rf_amd_image* old_filter,
                           rf_amd_image* filter, const uint32_t* const* new_fp_arrs, const uint64_t* num_new_fp,
                           const uint16_t* values, uint32_t num_runs) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (!filter) return fail(RF_AMD_EINVAL, "null filter out-param");
  memset(filter, 0, sizeof(*filter));
  const uint32_t k = num_runs ? num_runs : 1u;
  std::vector<uint32_t> lens(k);
  uint64_t total = 0;
  for (uint32_t j = 0; j < k; j++) {
    if (num_new_fp[j] && !new_fp_arrs[j]) return fail(RF_AMD_EINVAL, "null fingerprint array");
    if (num_new_fp[j] > 0xffffffffull) return fail(RF_AMD_EINVAL, "too many fingerprints");
    lens[j] = (uint32_t)num_new_fp[j];
    total += num_new_fp[j];
  }
  rf_amd_batch* ob = nullptr;
  const bool has_old = old_filter && old_filter->pages && old_filter->info.num_fingerprints;
  if (has_old)
    if (int rc = batch_from_image(e, cfg, old_filter, &ob)) return rc;
  rf_amd_batch* b = nullptr;
  uint32_t zero = 0;
  int rc = num_runs ? rf_amd_batch_create_runs(e, cfg, 1, &num_runs, lens.data(), values, has_old ? &ob : nullptr,
                                               has_old ? &zero : nullptr, &b)
                    : rf_amd_batch_create(e, cfg, 1, lens.data(), values, has_old ? &ob : nullptr,
                                          has_old ? &zero : nullptr, &b);
  if (rc) {
    rf_amd_batch_destroy(ob);
    return rc;
  }
  DevBuf d_h;
  if ((rc = d_h.alloc(4ull * total + 16)) == 0) {
    uint64_t at = 0;
    for (uint32_t j = 0; j < k && !rc; j++) {
      if (lens[j] && hipMemcpyAsync(d_h.as<uint32_t>() + at, new_fp_arrs[j], 4ull * lens[j], hipMemcpyHostToDevice,
                                    e->stream) != hipSuccess)
        rc = fail(RF_AMD_EINVAL, "H2D failed");
      at += lens[j];
    }
  }
  if (!rc) rc = rf_amd_batch_build_hashes(b, d_h.as<uint32_t>(), nullptr);
  rf_amd_filter_info info{};
  if (!rc) rc = rf_amd_batch_info(b, 0, &info);
  if (!rc && info.error) rc = fail(RF_AMD_EINVAL, "filter exceeds the on-disk format (error bits set)");
  if (!rc) {
    filter->info = info;
    filter->pages = (uint8_t*)calloc((size_t)info.num_pages * cfg->page_size + 16, 1);
    filter->slots = (uint64_t*)calloc(info.num_indices, 8);
    if (!filter->pages || !filter->slots) rc = fail(RF_AMD_ENOMEM, "host allocation failed");
  }
  if (!rc) rc = rf_amd_batch_read_image(b, 0, filter->pages, (uint64_t)info.num_pages * cfg->page_size,
                                        filter->slots, info.num_indices);
  if (rc) rf_amd_image_free(filter);
  rf_amd_batch_destroy(b);
  rf_amd_batch_destroy(ob);
  return rc;
}

extern "C" int rf_amd_filter_add(rf_amd_engine* e, const rf_amd_config* cfg, const rf_amd_image* old_filter,
                                 rf_amd_image* filter, const uint32_t* new_fp_arr, uint64_t num_new_fp,
                                 uint16_t value) {
  return filter_add_runs(e, cfg, old_filter, filter, &new_fp_arr, &num_new_fp, &value, 0);
}

extern "C" int rf_amd_filter_add_runs(rf_amd_engine* e, const rf_amd_config* cfg, const rf_amd_image* old_filter,
                                      rf_amd_image* filter, const uint32_t* const* new_fp_arrs,
                                      const uint64_t* num_new_fp, const uint16_t* values, uint32_t num_runs) {
  if (!num_runs || !new_fp_arrs || !num_new_fp || !values) return fail(RF_AMD_EINVAL, "null / empty runs");
  return filter_add_runs(e, cfg, old_filter, filter, new_fp_arrs, num_new_fp, values, num_runs);
}

extern "C" int rf_amd_filter_lookup_hashes(rf_amd_engine* e, const rf_amd_config* cfg, const rf_amd_image* filter,
                                           const uint32_t* hashes, uint64_t n, uint64_t* found_values) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (!filter || !filter->pages) {  // NULL filter finds nothing (src/routing_filter.c:1003-1006)
    if (found_values) memset(found_values, 0, 8 * n);
    return 0;
  }
  if (n == 0) return 0;
  rf_amd_batch* b = nullptr;
  if (int rc = batch_from_image(e, cfg, filter, &b)) return rc;
  DevBuf d_h, d_f, d_id;
  int rc = d_h.alloc(4 * n) | d_f.alloc(8 * n) | d_id.alloc(4 * n);
  if (!rc) {
    hipStream_t st = e->stream;
    if (hipMemcpyAsync(d_h.p, hashes, 4 * n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(d_id.p, 0, 4 * n, st) != hipSuccess)
      rc = fail(RF_AMD_EINVAL, "H2D failed");
    if (!rc) rc = rf_amd_batch_probe_hashes(b, d_h.as<uint32_t>(), d_id.as<uint32_t>(), n, d_f.as<uint64_t>(), st);
    if (!rc && (hipMemcpyAsync(found_values, d_f.p, 8 * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess))
      rc = fail(RF_AMD_EINVAL, "D2H failed");
  }
  rf_amd_batch_destroy(b);
  return rc;
}

extern "C" int rf_amd_filter_lookup_keys(rf_amd_engine* e, const rf_amd_config* cfg, const rf_amd_image* filter,
                                         const void* keys, uint32_t key_len, uint64_t n, uint64_t* found_values) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (!filter || !filter->pages) {
    if (found_values) memset(found_values, 0, 8 * n);
    return 0;
  }
  if (n == 0) return 0;
  if (!keys || key_len == 0) return fail(RF_AMD_EINVAL, "null keys");
  rf_amd_batch* b = nullptr;
  if (int rc = batch_from_image(e, cfg, filter, &b)) return rc;
  DevBuf d_k, d_f, d_id;
  int rc = d_k.alloc((size_t)key_len * n + 16) | d_f.alloc(8 * n) | d_id.alloc(4 * n);
  if (!rc) {
    hipStream_t st = e->stream;
    if (hipMemcpyAsync(d_k.p, keys, (size_t)key_len * n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(d_id.p, 0, 4 * n, st) != hipSuccess)
      rc = fail(RF_AMD_EINVAL, "H2D failed");
    if (!rc) rc = rf_amd_batch_probe_keys(b, d_k.p, key_len, d_id.as<uint32_t>(), n, d_f.as<uint64_t>(), st);
    if (!rc && (hipMemcpyAsync(found_values, d_f.p, 8 * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess))
      rc = fail(RF_AMD_EINVAL, "D2H failed");
  }
  rf_amd_batch_destroy(b);
  return rc;
}

// only the byte range the keys occupy goes to the device, with the offsets rebased to it
extern "C" int rf_amd_filter_lookup_var_keys(rf_amd_engine* e, const rf_amd_config* cfg, const rf_amd_image* filter,
                                             const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                                             uint64_t* found_values) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (!filter || !filter->pages) {
    if (found_values) memset(found_values, 0, 8 * n);
    return 0;
  }
  if (n == 0) return 0;
  if (!offsets || !found_values) return fail(RF_AMD_EINVAL, "null keys");
  const uint64_t base = offsets[0], total = offsets[n] - base;
  if (offsets[n] < base) return fail(RF_AMD_EINVAL, "offsets decrease");
  if (total && !bytes) return fail(RF_AMD_EINVAL, "null keys");
  rf_amd_batch* b = nullptr;
  if (int rc = batch_from_image(e, cfg, filter, &b)) return rc;
  std::vector<uint64_t> rel(offsets, offsets + n + 1);
  for (auto& o : rel) o -= base;
  DevBuf d_k, d_o, d_f, d_id;
  int rc = d_k.alloc(total + 16) | d_o.alloc(8 * (n + 1)) | d_f.alloc(8 * n) | d_id.alloc(4 * n);
  if (!rc) {
    hipStream_t st = e->stream;
    if ((total && hipMemcpyAsync(d_k.p, bytes + base, total, hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipMemcpyAsync(d_o.p, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(d_id.p, 0, 4 * n, st) != hipSuccess)
      rc = fail(RF_AMD_EINVAL, "H2D failed");
    if (!rc)
      rc = rf_amd_batch_probe_var_keys(b, d_k.as<uint8_t>(), d_o.as<uint64_t>(), d_id.as<uint32_t>(), n,
                                       d_f.as<uint64_t>(), st);
    if (!rc && (hipMemcpyAsync(found_values, d_f.p, 8 * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess))
      rc = fail(RF_AMD_EINVAL, "D2H failed");
  }
  rf_amd_batch_destroy(b);
  return rc;
}

extern "C" void rf_amd_image_free(rf_amd_image* img) {
  if (!img) return;
  free(img->pages);
  free(img->slots);
  img->pages = nullptr;
  img->slots = nullptr;
}

extern "C" uint64_t rf_amd_max_fingerprints(const rf_amd_config* cfg) {
  return max_fingerprints(*cfg);
}

// src/routing_filter.c:1119-1139 as the reference's release build evaluates it (-O3
// -ffast-math, Makefile:89,123-124: GCC reassociates the sum into two fused multiply-adds and
// truncates through 64 bits). The order decides the result where the exact value is an
// integer (num_unique = 1: exactly 1 there, 0 in source order); oracle/rf_oracle.c holds the
// same restatement, pinned against the reference for fingerprint sizes 8-32.
extern "C" uint32_t rf_amd_estimate_unique_keys_from_count(const rf_amd_config* cfg, uint64_t num_unique) {
#pragma clang fp contract(off)
  const double U = (double)(1ull << cfg->fingerprint_size);
  const double s = U - (double)num_unique;
  const double U2 = U * U, s2 = s * s;
  const double lU = log(U), ls = log(s);
  const double a = fma(1.0 / U - 1.0 / s, 0.5, (1.0 / s2 - 1.0 / U2) * (1.0 / 12.0));
  const double b = fma(1.0 / (U2 * U2) - 1.0 / (s2 * s2), 1.0 / 120.0, lU);
  return (uint32_t)(int64_t)(U * ((a + b) - ls));
}

extern "C" uint64_t rf_amd_space_use_bytes(const rf_amd_config* cfg, uint32_t num_pages) {
  const uint64_t extent = (uint64_t)cfg->page_size * cfg->pages_per_extent;
  return cfg->page_size + extent * (1 + (num_pages + cfg->pages_per_extent - 1) / cfg->pages_per_extent);
}

// ---- routing_filter_estimate_unique_fp (src/routing_filter.c:702-848) --------------------
constexpr uint64_t EST_MAX_FILTERS = 32;  // MAX_FILTERS, src/routing_filter.h:25

// fl: the filters to decode (pages/slots already device pointers, idx_first unset);
// total_num_fp: the reference's uint32 sum of num_fingerprints over ALL filters (:719-722)
static int estimate_run(rf_amd_engine* e, hipStream_t st, const rf_amd_config* cfg, std::vector<EstFilter>& fl,
                        uint32_t total_num_fp, uint32_t* num_unique_fp) {
  uint32_t total_idx = 0;
  for (auto& f : fl) {
    f.idx_first = total_idx;
    total_idx += f.num_idx;
  }
  const uint32_t ubits = cfg->fingerprint_size > 4 ? cfg->fingerprint_size - 4 : 0;  // fps < 2^(fp_size-4)
  uint64_t words = ((1ull << ubits) + 31) / 32;
  words = (words + 3) & ~3ull;
  DevBuf d_fl, d_bm, d_cnt;
  if (d_fl.alloc(sizeof(EstFilter) * (fl.size() + 1)) || d_bm.alloc(4 * words) || d_cnt.alloc(16))
    return fail(RF_AMD_ENOMEM, "device allocation failed");
  if (!fl.empty())
    HIPCHK(hipMemcpyAsync(d_fl.p, fl.data(), sizeof(EstFilter) * fl.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d_bm.p, 0, 4 * words, st));
  HIPCHK(hipMemsetAsync(d_cnt.p, 0, 16, st));
  if (rf_launch_estimate(st, d_fl.as<EstFilter>(), (uint32_t)fl.size(), total_idx, cfg->log_index_size,
                         d_bm.as<uint32_t>(), words, d_cnt.as<uint32_t>()))
    return fail(RF_AMD_EINVAL, "estimate kernel launch failed");
  uint32_t cnt[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(cnt, d_cnt.p, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  (void)e;
  // the reference unpacks every decoded entry into a total_num_fp / 12 buffer and asserts
  // it fits (:776-780); the running count only grows, so this is the same condition
  if (cnt[0] > total_num_fp / 12)
    return fail(RF_AMD_EINVAL, "decoded fingerprints exceed num_fingerprints / 12 (reference asserts, :776)");
  *num_unique_fp = cnt[1] * 16;
  return 0;
}

static uint32_t est_lnb(const rf_amd_config* cfg, uint32_t num_fp) {
  uint32_t lnb = num_fp ? 31 - __builtin_clz(num_fp) : 0;
  return lnb < cfg->log_index_size ? cfg->log_index_size : lnb;
}

extern "C" int rf_amd_estimate_unique_fp(rf_amd_engine* e, const rf_amd_config* cfg, const rf_amd_image* filters,
                                         uint64_t num_filters, uint32_t* num_unique_fp) {
  if (!num_unique_fp) return fail(RF_AMD_EINVAL, "num_unique_fp must not be NULL");  // :710-714
  *num_unique_fp = 0;
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (int rc = check_cfg(cfg)) return rc;
  if (num_filters > EST_MAX_FILTERS) return fail(RF_AMD_EINVAL, "more than MAX_FILTERS filters (:717)");
  if (num_filters && !filters) return fail(RF_AMD_EINVAL, "null filters");
  HIPCHK(hipSetDevice(e->device));
  hipStream_t st = e->stream;
  uint32_t total_num_fp = 0;
  std::vector<EstFilter> fl;
  std::vector<DevBuf> bufs(2 * num_filters);
  for (uint64_t i = 0; i < num_filters; i++) {
    const rf_amd_image& im = filters[i];
    total_num_fp += im.info.num_fingerprints;
    if (!im.pages || !im.slots) continue;  // filter.addr == 0 (:739-742)
    const uint32_t lnb = est_lnb(cfg, im.info.num_fingerprints);
    if (lnb > cfg->fingerprint_size || lnb - cfg->log_index_size > 14)
      return fail(RF_AMD_EINVAL, "image geometry out of range");
    const uint32_t num_indices = 1u << (lnb - cfg->log_index_size);
    if (num_indices < 16) continue;  // "the filter is too small forget it" (:755)
    if (cfg->fingerprint_size + im.info.value_size > 32) return fail(RF_AMD_EINVAL, "fp_size + value_size > 32");
    const uint32_t nidx = num_indices / 16;
    uint64_t last_page = 0;  // upload only the pages the decoded indices live on
    for (uint32_t k = 0; k < nidx; k++) last_page = std::max<uint64_t>(last_page, im.slots[k] / cfg->page_size);
    if (last_page >= im.info.num_pages) return fail(RF_AMD_EINVAL, "index slot outside the image");
    const uint64_t pbytes = (last_page + 1) * cfg->page_size;
    DevBuf& dp = bufs[2 * i];
    DevBuf& ds = bufs[2 * i + 1];
    if (dp.alloc(pbytes + 256) || ds.alloc(8ull * nidx)) return fail(RF_AMD_ENOMEM, "device allocation failed");
    HIPCHK(hipMemsetAsync(dp.as<uint8_t>() + pbytes, 0, 256, st));
    HIPCHK(hipMemcpyAsync(dp.p, im.pages, pbytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ds.p, im.slots, 8ull * nidx, hipMemcpyHostToDevice, st));
    const uint32_t rem = cfg->fingerprint_size - lnb;
    fl.push_back(EstFilter{dp.as<uint8_t>(), ds.as<uint64_t>(), im.info.value_size, rem + im.info.value_size, nidx, 0});
  }
  return estimate_run(e, st, cfg, fl, total_num_fp, num_unique_fp);
}

extern "C" int rf_amd_batch_estimate_unique_fp(rf_amd_batch* const* batches, const uint32_t* filter_index,
                                               uint64_t num_filters, uint32_t* num_unique_fp) {
  if (!num_unique_fp) return fail(RF_AMD_EINVAL, "num_unique_fp must not be NULL");
  *num_unique_fp = 0;
  if (num_filters > EST_MAX_FILTERS) return fail(RF_AMD_EINVAL, "more than MAX_FILTERS filters (:717)");
  if (num_filters == 0) return 0;
  if (!batches || !filter_index) return fail(RF_AMD_EINVAL, "null batch list");
  rf_amd_engine* e = nullptr;
  const rf_amd_config* cfg = nullptr;
  uint32_t total_num_fp = 0;
  std::vector<EstFilter> fl;
  for (uint64_t i = 0; i < num_filters; i++) {
    rf_amd_batch* b = batches[i];
    if (!b) continue;  // NULL_ROUTING_FILTER
    const uint32_t f = filter_index[i];
    if (f >= b->F || !b->built) return fail(RF_AMD_EINVAL, "bad batch/filter (not built)");
    if (!e) {
      e = b->eng;
      cfg = &b->cfg;
    } else if (b->eng != e || memcmp(&b->cfg, cfg, sizeof(*cfg)) != 0) {
      return fail(RF_AMD_EINVAL, "filters of one estimate must share an engine and a routing config");
    }
    const FilterPlan& p = b->plans[f];
    total_num_fp += p.num_fp;
    if (p.num_indices < 16) continue;
    fl.push_back(EstFilter{b->d_pages.as<uint8_t>() + (uint64_t)p.page_base * b->cfg.page_size,
                           b->d_slots.as<uint64_t>() + p.idx_base, p.vs, p.rvs, p.num_indices / 16, 0});
  }
  if (!e) return 0;
  HIPCHK(hipSetDevice(e->device));
  // the images must be complete (and error-free) before they are decoded
  for (uint64_t i = 0; i < num_filters; i++) {
    if (!batches[i]) continue;
    rf_amd_filter_info info;
    if (int rc = rf_amd_batch_info(batches[i], filter_index[i], &info)) return rc;
    if (info.error) return fail(RF_AMD_EINVAL, "filter build reported error bits");
  }
  return estimate_run(e, e->stream, cfg, fl, total_num_fp, num_unique_fp);
}

extern "C" uint32_t rf_amd_estimate_unique_keys(const rf_amd_filter_info* filter, const rf_amd_config* cfg) {
  return rf_amd_estimate_unique_keys_from_count(cfg, filter->num_unique);  // .c:1141-1146
}

// ---- asynchronous batched lookup (routing_filter_lookup_async, src/routing_filter.h:130-155,
// .c:895-972) ---------------------------------------------------------------------------
// The reference's coroutine yields while a filter page is read and calls `callback` when it
// can be resumed; here one call stages a whole batch of lookups (H2D, probe, D2H) on a
// stream and the callback fires from a HIP host function once the results are in h_found.
struct rf_amd_lookup_async_state {
  rf_amd_batch* b = nullptr;
  hipStream_t st = nullptr;
  uint64_t n = 0;
  uint64_t* h_found = nullptr;
  void* h_stage = nullptr;  // pinned: keys in, found values out
  size_t stage_bytes = 0;
  DevBuf d_keys, d_fid, d_found;
  hipEvent_t done_ev = nullptr;
  rf_amd_callback_fn cb = nullptr;
  void* cb_arg = nullptr;
  volatile int done = 0;
  ~rf_amd_lookup_async_state() {
    if (done_ev) (void)hipEventSynchronize(done_ev);
    if (done_ev) (void)hipEventDestroy(done_ev);
    if (h_stage) (void)hipHostFree(h_stage);
  }
};

static void lookup_async_finish(void* arg) {  // HIP host function: no HIP calls in here
  auto* s = static_cast<rf_amd_lookup_async_state*>(arg);
  memcpy(s->h_found, s->h_stage, 8 * s->n);
  __atomic_store_n(&s->done, 1, __ATOMIC_RELEASE);
  if (s->cb) s->cb(s->cb_arg);
}

extern "C" int rf_amd_lookup_async(rf_amd_batch* b, const void* h_keys, uint32_t key_len,
                                   const uint32_t* h_filter_id, uint64_t n, uint64_t* h_found,
                                   rf_amd_callback_fn callback, void* callback_arg, void* stream,
                                   rf_amd_lookup_async_state** out) {
  if (!out) return fail(RF_AMD_EINVAL, "null state out-param");
  *out = nullptr;
  if (!b || !b->built) return fail(RF_AMD_EINVAL, "batch not built");
  if (n && (!h_keys || !h_found || key_len == 0)) return fail(RF_AMD_EINVAL, "null keys / results");
  HIPCHK(hipSetDevice(b->eng->device));
  auto* s = new rf_amd_lookup_async_state();
  s->b = b;
  s->st = stream_of(b->eng, stream);
  s->n = n;
  s->h_found = h_found;
  s->cb = callback;
  s->cb_arg = callback_arg;
  const size_t kbytes = (size_t)key_len * n;
  s->stage_bytes = std::max<size_t>(std::max<size_t>(kbytes, 8 * n), 16);
  int rc = 0;
  if (hipHostMalloc(&s->h_stage, s->stage_bytes, hipHostMallocDefault) != hipSuccess) {
    s->h_stage = nullptr;
    rc = fail(RF_AMD_ENOMEM, "pinned staging allocation failed");
  }
  if (!rc) rc = s->d_keys.alloc(kbytes + 16) | s->d_fid.alloc(4 * n + 16) | s->d_found.alloc(8 * n + 16);
  if (!rc && hipEventCreateWithFlags(&s->done_ev, hipEventDisableTiming) != hipSuccess)
    rc = fail(RF_AMD_EINVAL, "event creation failed");
  if (rc) {
    delete s;
    return rc;
  }
  if (n) {
    memcpy(s->h_stage, h_keys, kbytes);
    if (hipMemcpyAsync(s->d_keys.p, s->h_stage, kbytes, hipMemcpyHostToDevice, s->st) != hipSuccess ||
        (h_filter_id ? hipMemcpyAsync(s->d_fid.p, h_filter_id, 4 * n, hipMemcpyHostToDevice, s->st)
                     : hipMemsetAsync(s->d_fid.p, 0, 4 * n, s->st)) != hipSuccess)
      rc = fail(RF_AMD_EINVAL, "H2D failed");
    if (!rc) rc = rf_amd_batch_probe_keys(b, s->d_keys.p, key_len, s->d_fid.as<uint32_t>(), n,
                                          s->d_found.as<uint64_t>(), s->st);
    // the keys' staging copy has been consumed once the probe ran: reuse it for the results
    if (!rc && hipMemcpyAsync(s->h_stage, s->d_found.p, 8 * n, hipMemcpyDeviceToHost, s->st) != hipSuccess)
      rc = fail(RF_AMD_EINVAL, "D2H failed");
  }
  if (!rc && hipLaunchHostFunc(s->st, lookup_async_finish, s) != hipSuccess)
    rc = fail(RF_AMD_EINVAL, "host function launch failed");
  if (!rc && hipEventRecord(s->done_ev, s->st) != hipSuccess) rc = fail(RF_AMD_EINVAL, "event record failed");
  if (rc) {
    (void)hipStreamSynchronize(s->st);
    delete s;
    return rc;
  }
  *out = s;
  return 0;
}

extern "C" int rf_amd_lookup_async_poll(rf_amd_lookup_async_state* s) {
  if (!s) return RF_AMD_ASYNC_DONE;
  return __atomic_load_n(&s->done, __ATOMIC_ACQUIRE) ? RF_AMD_ASYNC_DONE : RF_AMD_ASYNC_RUNNING;
}

extern "C" int rf_amd_lookup_async_wait(rf_amd_lookup_async_state* s) {
  if (!s) return 0;
  HIPCHK(hipEventSynchronize(s->done_ev));
  while (!__atomic_load_n(&s->done, __ATOMIC_ACQUIRE)) {
  }
  return 0;
}

extern "C" void rf_amd_lookup_async_free(rf_amd_lookup_async_state* s) {
  if (!s) return;
  (void)rf_amd_lookup_async_wait(s);
  delete s;
}

// ---- batch hashing (data_key_hash, btree_pack's fingerprint loop) -------------------------
extern "C" int rf_amd_hash_keys(rf_amd_engine* e, const rf_amd_config* cfg, const void* d_keys, uint32_t key_len,
                                uint64_t n, uint32_t* d_hashes, void* stream) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (int rc = check_cfg(cfg)) return rc;
  if (n && (!d_keys || !d_hashes || key_len == 0)) return fail(RF_AMD_EINVAL, "null keys / output");
  HIPCHK(hipSetDevice(e->device));
  if (rf_launch_hash(stream_of(e, stream), fixed_kind(d_keys, key_len), d_keys, nullptr, key_len, cfg->seed, n,
                     d_hashes))
    return fail(RF_AMD_EINVAL, "hash kernel launch failed");
  return 0;
}

extern "C" int rf_amd_hash_var_keys(rf_amd_engine* e, const rf_amd_config* cfg, const uint8_t* d_bytes,
                                    const uint64_t* d_offsets, uint64_t n, uint32_t* d_hashes, void* stream) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (int rc = check_cfg(cfg)) return rc;
  if (n && (!d_bytes || !d_offsets || !d_hashes)) return fail(RF_AMD_EINVAL, "null keys / output");
  HIPCHK(hipSetDevice(e->device));
  if (rf_launch_hash(stream_of(e, stream), IN_VAR, d_bytes, d_offsets, 0, cfg->seed, n, d_hashes))
    return fail(RF_AMD_EINVAL, "hash kernel launch failed");
  return 0;
}

// ---- routed probes across ranks --------------------------------------------
extern "C" uint64_t rf_amd_route_scratch_bytes(uint64_t n, uint32_t world) {
  return 4 * rf_route_scratch_words(n, world) + 8 + 8 * (uint64_t)RF_AMD_ROUTE_MAX_WORLD;
}

extern "C" int rf_amd_route_probes(rf_amd_engine* e, const uint32_t* d_hashes, const uint32_t* d_filter_id,
                                   uint64_t n, const uint32_t* d_route, uint32_t num_filters, uint32_t world,
                                   uint64_t* d_pairs, uint32_t* d_perm, void* d_scratch, uint64_t* h_counts,
                                   void* stream) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (world == 0 || world > RF_AMD_ROUTE_MAX_WORLD) return fail(RF_AMD_EINVAL, "world out of range");
  if (!h_counts) return fail(RF_AMD_EINVAL, "null counts");
  for (uint32_t d = 0; d < world; d++) h_counts[d] = 0;
  if (n == 0) return 0;
  if (n >= (1ull << 32)) return fail(RF_AMD_EINVAL, "more than 2^32 - 1 probes");
  if (!d_hashes || !d_filter_id || !d_route || !d_pairs || !d_perm || !d_scratch)
    return fail(RF_AMD_EINVAL, "null route buffer");
  HIPCHK(hipSetDevice(e->device));
  hipStream_t st = stream_of(e, stream);
  uint32_t* scratch = static_cast<uint32_t*>(d_scratch);
  const uint64_t words = rf_route_scratch_words(n, world);
  uint64_t* d_tot = reinterpret_cast<uint64_t*>(scratch + ((words + 1) & ~1ull));
  if (rf_launch_route(st, d_hashes, d_filter_id, n, d_route, num_filters, world, d_pairs, d_perm, scratch, d_tot))
    return fail(RF_AMD_EINVAL, "route kernel launch failed");
  uint32_t err = 0;
  HIPCHK(hipMemcpyAsync(h_counts, d_tot, 8 * world, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&err, scratch + words - 4, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (err & 1u) return fail(RF_AMD_EINVAL, "probe filter id out of range");
  if (err & 2u) return fail(RF_AMD_EINVAL, "route table names a rank >= world");
  return 0;
}

extern "C" int rf_amd_unroute_found(rf_amd_engine* e, const uint64_t* d_back, const uint32_t* d_perm, uint64_t n,
                                    uint64_t* d_found, void* stream) {
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (n && (!d_back || !d_perm || !d_found)) return fail(RF_AMD_EINVAL, "null unroute buffer");
  HIPCHK(hipSetDevice(e->device));
  if (rf_launch_unroute(stream_of(e, stream), d_back, d_perm, n, d_found))
    return fail(RF_AMD_EINVAL, "unroute kernel launch failed");
  return 0;
}

extern "C" int rf_amd_batch_probe_pairs(rf_amd_batch* b, const uint64_t* d_pairs, uint64_t n, uint64_t* d_found,
                                        void* stream) {
  return do_probe(b, IN_PAIR, d_pairs, nullptr, 8, reinterpret_cast<const uint32_t*>(d_pairs), n, d_found, stream);
}

// ---- routing_filter_verify (src/routing_filter.c:1163-1183) ------------------------------
extern "C" int rf_amd_filter_verify(rf_amd_engine* e, const rf_amd_config* cfg, const rf_amd_image* filter,
                                    const void* keys, uint32_t key_len, uint64_t n, uint16_t value,
                                    uint64_t* num_missing) {
  if (num_missing) *num_missing = 0;
  if (!e) return fail(RF_AMD_ENODEV, "no engine");
  if (value >= 64) return fail(RF_AMD_EINVAL, "value >= 64");
  if (n == 0) return 0;
  if (!keys || key_len == 0) return fail(RF_AMD_EINVAL, "null keys");
  if (!filter || !filter->pages) {  // a NULL filter finds nothing: every key is missing
    if (num_missing) *num_missing = n;
    return fail(RF_AMD_EINVAL, "verify: key not found in a NULL filter");
  }
  rf_amd_batch* b = nullptr;
  if (int rc = batch_from_image(e, cfg, filter, &b)) return rc;
  DevBuf d_k, d_f, d_id, d_m;
  int rc = d_k.alloc((size_t)key_len * n + 16) | d_f.alloc(8 * n) | d_id.alloc(4 * n) | d_m.alloc(8);
  unsigned long long missing = 0;
  if (!rc) {
    hipStream_t st = e->stream;
    if (hipMemcpyAsync(d_k.p, keys, (size_t)key_len * n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(d_id.p, 0, 4 * n, st) != hipSuccess || hipMemsetAsync(d_m.p, 0, 8, st) != hipSuccess)
      rc = fail(RF_AMD_EINVAL, "H2D failed");
    if (!rc) rc = rf_amd_batch_probe_keys(b, d_k.p, key_len, d_id.as<uint32_t>(), n, d_f.as<uint64_t>(), st);
    if (!rc && rf_launch_count_missing(st, d_f.as<uint64_t>(), n, value, d_m.as<unsigned long long>()))
      rc = fail(RF_AMD_EINVAL, "verify kernel launch failed");
    if (!rc && (hipMemcpyAsync(&missing, d_m.p, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess))
      rc = fail(RF_AMD_EINVAL, "D2H failed");
  }
  rf_amd_batch_destroy(b);
  if (rc) return rc;
  if (num_missing) *num_missing = missing;
  // the reference asserts routing_filter_is_value_found for every key (:1177)
  return missing ? fail(RF_AMD_EINVAL, "verify: " + std::to_string(missing) + " keys not found") : 0;
}

// ---- routing_filter_print (src/routing_filter.c:1185-1286): debug text, host only ----------
static int print_filter(const rf_amd_config* cfg, const rf_amd_image* filter, uint64_t filter_addr,
                        const uint64_t* abs_slots, void* out_file);

extern "C" int rf_amd_filter_print(const rf_amd_config* cfg, const rf_amd_image* filter, void* out_file) {
  return print_filter(cfg, filter, 0, nullptr, out_file);
}

extern "C" int rf_amd_filter_print_abs(const rf_amd_config* cfg, const rf_amd_image* filter, uint64_t filter_addr,
                                       const uint64_t* abs_slots, void* out_file) {
  if (!abs_slots) return fail(RF_AMD_EINVAL, "null absolute slots");
  return print_filter(cfg, filter, filter_addr, abs_slots, out_file);
}

static int print_filter(const rf_amd_config* cfg, const rf_amd_image* filter, uint64_t filter_addr,
                        const uint64_t* abs_slots, void* out_file) {
  if (int rc = check_cfg(cfg)) return rc;
  if (!filter || !filter->pages || !filter->slots) return fail(RF_AMD_EINVAL, "null filter");
  FILE* fo = out_file ? (FILE*)out_file : stdout;
  const uint32_t lis = cfg->log_index_size, index_size = 1u << lis;
  const uint32_t lnb = est_lnb(cfg, filter->info.num_fingerprints);
  const uint32_t num_indices = 1u << (lnb - lis);
  const uint32_t rem = cfg->fingerprint_size - lnb, vs = filter->info.value_size, rvs = rem + vs;
  const uint8_t* pg = filter->pages;
  auto bit = [&](uint64_t bp) { return (pg[bp >> 3] >> (bp & 7)) & 1u; };
  fprintf(fo, "********************************************************************************\n");
  fprintf(fo, "***   filter INDEX\n");
  fprintf(fo, "***   filter_addr: %lu\n", (unsigned long)filter_addr);
  fprintf(fo, "--------------------------------------------------------------------------------\n");
  for (uint32_t i = 0; i < num_indices; i++)
    fprintf(fo, "index 0x%x: %lu\n", i, (unsigned long)(abs_slots ? abs_slots[i] : filter->slots[i]));
  for (uint32_t i = 0; i < num_indices; i++) {
    const uint64_t h = filter->slots[i];
    const uint32_t c = (uint32_t)pg[h] | ((uint32_t)pg[h + 1] << 8);
    fprintf(fo, "----------------------------------------\n");
    fprintf(fo, "--- Index 0x%x\n", i);
    fprintf(fo, "--- Encoding: %u\n", c);
    const uint64_t eb = (h + 2) * 8;
    for (uint32_t k = 0; k < c + index_size; k++) {
      if (k != 0 && k % 16 == 0) fprintf(fo, " | ");
      fputc(bit(eb + k) ? '1' : '0', fo);
    }
    fputc('\n', fo);
    fprintf(fo, "--- Remainders\n");
    // print_remainders' header_length uses (c + index_size - 1) / 8 + 1 encoding bytes, not
    // the block's + 4 (:1234-1236 vs :207-211): the reference prints from that offset, so do we
    const uint64_t hl = (c + index_size - 1) / 8 + 1 + 2;
    const uint64_t rb = (h + hl) * 8;
    // bucket bounds by walking the unary encoding (routing_get_bucket_bounds, :230-279)
    uint32_t pos = 0, start = 0;
    for (uint32_t bo = 0; bo < index_size; bo++) {
      uint32_t cnt = 0;
      while (pos < c + index_size && !bit(eb + pos)) { pos++; cnt++; }
      pos++;  // the bucket's terminating 1
      fprintf(fo, "0x%x remainders:", bo);
      for (uint32_t j = start; j < start + cnt; j++) {
        uint32_t rv = 0;
        for (uint32_t t = 0; t < rvs; t++) rv |= bit(rb + (uint64_t)j * rvs + t) << t;
        fprintf(fo, " 0x%x:%u", vs >= 32 ? 0u : rv >> vs, rv & (uint32_t)((1ull << vs) - 1));
      }
      fputc('\n', fo);
      start += cnt;
    }
  }
  fflush(fo);
  return 0;
}
