// rf_launch.h -- every function that rf_kernels.hip defines and rf_engine.cpp calls, declared
// once. Both files include it, so the compiler sees each declaration next to its definition:
// extern "C" names carry no types, and a parameter changed on one side alone would still link.
#pragma once
#include <stdint.h>

#include "rf_plan.h"
#include "rf_range_plan.h"
#include "rf_range_seg_plan.h"
#include "rf_range_split_plan.h"
#include "rf_per_key_plan.h"
#include "rf_by_branch_plan.h"
#include "rf_advance_plan.h"

extern "C" {

// ---- build --------------------------------------------------------------------------------
// K1-K6 on a.stream for one batch (a chained batch when a.tile_value is set)
int rf_launch_build(const rf::LaunchArgs* a);
// zero the coarse-bucket counters, the output words and the overflow / spill / page-list flags
int rf_launch_build_init(void* stream, uint32_t* cb_count, uint32_t* cb_cursor, uint32_t num_cb,
                         uint32_t* outs_words, uint32_t num_out_words, uint32_t* overflow, uint32_t* spill,
                         uint32_t* plist);
// K0: decode the old filters of an incremental add into entries
int rf_launch_old_decode(const rf::LaunchArgs* a);
// probe lines of a batch, cut from its image
int rf_launch_plines(const rf::LaunchArgs* a);
// fof[i] = the filter of element i under the prefix sums pre[0..nf]; start[i] (optional) =
// (i - pre[fof[i]]) * mul
int rf_launch_seg_fill(void* stream, const uint32_t* pre, uint32_t nf, uint32_t n, uint32_t* fof, uint32_t* start,
                       uint32_t mul);
// the probe's wave table over the run bounds runs[0..nf]: tab[w] = (filter of probe 64 w) << 7 |
// the wave's leading probes in that filter's run
int rf_launch_wave_tab(void* stream, const uint64_t* runs, uint32_t nf, uint64_t n, uint32_t* tab);
// copy pages and index slots of an image to the addresses of a page table
int rf_launch_place(void* stream, const uint8_t* img, const uint64_t* slots, uint32_t first_page, uint32_t count,
                    uint32_t num_pages, uint32_t num_indices, uint32_t page_size, const uint64_t* table,
                    uint32_t addrs_per_page);
// builds whose K4 ran as the bitmap kernel, counted where K4 is launched
uint64_t rf_k4_bitmap_builds(void);
// builds whose partition wrote 16-bit in-bucket keys for that kernel (k_hash_scatter, P16)
uint64_t rf_part16_builds(void);
// whether rf_launch_build launches this build packed (K4 writes index-block bodies instead of
// sorted entries unless the partition spills: the batch then has no entries for a later add to
// read in place), and how many builds were
int rf_build_packs(const rf::LaunchArgs* a);
uint64_t rf_k4_packed_builds(void);
// diagnostics build: the buffer the build kernels write their phase clock stamps to
int rf_debug_set_phase_buffer(uint64_t* d_buf, uint32_t kid);

// ---- probes -------------------------------------------------------------------------------
// k_probe, one lane per probe; offs: the n + 1 byte offsets of IN_VAR keys
int rf_launch_probe(const rf::LaunchArgs* a, int kind, const void* in0, const uint64_t* offs, uint32_t key_len,
                    const uint32_t* filter_id, uint64_t n, uint64_t* found);
// bench.py's measured probe floor: k_probe_floor over the same runs (rf_amd_diag.h)
int rf_launch_probe_floor(const rf::LaunchArgs* a, int kind, const void* in0, uint64_t n, uint64_t* found);
// host-buffer lookups: n hashes, each against the group of its position
int rf_launch_probe_groups(void* stream, const uint32_t* in, const rf::ProbeGroup* groups, uint32_t ng, uint64_t n,
                           uint64_t* found, uint32_t* counter, uint32_t* done_flag, uint32_t seq);
// one wave for a lookup of at most a wave of hashes
int rf_launch_probe_small(void* stream, const rf::SmallProbe* a);
// the persistent lookup-server wave over the request ring
int rf_launch_lookup_server(void* stream, const rf::SrvReq* ring, rf::SrvRes* res, rf::SrvCtl* ctl, uint64_t head,
                            uint64_t gen, uint64_t idle_ticks, uint64_t life_ticks);

// ---- multi-get ----------------------------------------------------------------------------
// offs: the n + 1 byte offsets of IN_VAR keys (in0 = their bytes), unused by the other kinds.
// moff == nullptr: the fixed form, key i against its K members (member == nullptr: all K == ng).
// Else the ragged form: key i against member[moff[i] .. moff[i+1]) (n + 1 pair offsets), found[p]
// for member[p]; K unused.
int rf_launch_probe_fanout(void* stream, int kind, const void* in0, const uint64_t* offs, uint32_t key_len,
                           uint32_t seed, const rf::ProbeGroup* groups, uint32_t ng, const uint32_t* member,
                           uint32_t K, const uint64_t* moff, uint64_t n, uint64_t* found);
// the same walk as an existence lookup (the kernels' EXISTS instantiations): exists[i] = the OR of
// RF_AMD_EXISTS_* over key i's pairs, every one of the n bytes written, no found word
int rf_launch_probe_fanout_exists(void* stream, int kind, const void* in0, const uint64_t* offs, uint32_t key_len,
                                  uint32_t seed, const rf::ProbeGroup* groups, uint32_t ng, const uint32_t* member,
                                  uint32_t K, const uint64_t* moff, uint64_t n, uint8_t* exists);
// k_set_update: a->n <= SET_UPD_PER_LAUNCH entries into the table a->groups, one launch
int rf_launch_set_update(void* stream, const rf::SetUpdate* a);
// diagnostics (rf_amd_diag_fanout_max_blocks): a cap on both fan-out grids; 0 = none
void rf_fanout_set_max_blocks(uint32_t blocks);
uint64_t rf_found_compact_tiles(uint64_t m);
// scratch: ntiles 64-bit offsets, then ntiles 32-bit sums
int rf_launch_found_compact(void* stream, const uint64_t* found, uint64_t m, uint64_t* cand, uint64_t cap,
                            uint64_t* count, void* scratch);

// ---- range maps (rf_range.hip) --------------------------------------------------------------
// k_range_find, k_range_scan, k_range_emit: n keys (var: keys[offs[i] .. offs[i+1]), else
// key_len bytes each) to range[n], member_off[n + 1], member[< pair_cap] and *total; scratch:
// range_route_scratch_bytes(n) bytes, 8-byte aligned
int rf_launch_range_route(void* stream, int var, const uint8_t* keys, const uint64_t* offs, uint32_t key_len,
                          uint64_t n, const rf::RangeDev* m, uint32_t* range, uint64_t* member_off,
                          uint32_t* member, uint64_t pair_cap, uint64_t* total, void* scratch);
// k_range_seg_scatter: one launch of a segment update, a->npieces pieces and their ids in the
// arguments (rf_range_seg_plan.h)
int rf_launch_range_seg_scatter(void* stream, const rf::RangeSegUpdate* a);
// k_range_seg_len, k_range_scan, k_range_seg_emit: loff[0..R] and list rewritten from the
// segments' current lists
int rf_launch_range_seg_flatten(void* stream, const rf::RangeSegDev* d);
// k_range_splice: one launch of a split or set_paths, from the structural copy a->src into
// a->dst (rf_range_split_plan.h); the first launch of an edit (a->bulk) copies what it keeps
int rf_launch_range_splice(void* stream, const rf::RangeSpliceArgs* a);
// diagnostics (rf_amd_diag_fanout_max_blocks): a cap on the route and flatten kernels' grids; 0 =
// none
void rf_range_set_max_blocks(uint32_t blocks);
// k_range_scan alone, one workgroup: the exclusive scan of ntiles 32-bit tile sums into 64-bit
// offsets off[ntiles], the total to *total and to *total_too (ntiles == 0: both 0)
void rf_launch_range_scan(void* stream, const uint32_t* cnt, uint64_t ntiles, uint64_t* off, uint64_t* total,
                          uint64_t* total_too);

// ---- key-aware compaction (rf_per_key.hip) ---------------------------------------------------
// k_per_key_count, k_range_scan, k_per_key_emit: the found words of n keys' pairs (moff: the
// n + 1 pair offsets of the ragged form; nullptr: K pairs per key, member == nullptr: id = slot)
// to key_off[n + 1], cand[< cap], cand_key[< cap] (nullptr: not written) and *count; scratch:
// per_key_scratch_bytes(n) bytes, 8-byte aligned (rf_per_key_plan.h)
int rf_launch_found_per_key(void* stream, const uint64_t* found, const uint32_t* member, const uint64_t* moff,
                            uint32_t K, uint64_t n, uint64_t* key_off, uint64_t* cand, uint64_t* cand_key,
                            uint64_t cap, uint64_t* count, void* scratch);
// diagnostics (rf_amd_diag_fanout_max_blocks): a cap on both kernels' grids; 0 = none
void rf_per_key_set_max_blocks(uint32_t blocks);

// ---- group by branch (rf_by_branch.hip) -------------------------------------------------------
// by_branch_launches(num_members) launches: the first min(*count, cap) records of cand to
// order[< cap] (their positions, stable by sort key), order_key[t] = cand_key[order[t]] (both
// nullptr: not written), branch[< branch_cap], branch_off[<= branch_cap] and *num_branches;
// scratch: by_branch_scratch_bytes(cap, num_members) bytes, 8-byte aligned (rf_by_branch_plan.h)
int rf_launch_found_by_branch(void* stream, const uint64_t* cand, const uint64_t* cand_key, const uint64_t* count,
                              uint64_t cap, uint32_t num_members, uint32_t* order, uint64_t* order_key,
                              uint64_t* branch, uint64_t* branch_off, uint64_t branch_cap, uint64_t* num_branches,
                              void* scratch);
// diagnostics (rf_amd_diag_fanout_max_blocks): a cap on the tile kernels' grids; 0 = none
void rf_by_branch_set_max_blocks(uint32_t blocks);

// ---- stepwise hand-out (rf_advance.hip) -------------------------------------------------------
// k_advance_count, k_range_scan, k_advance_emit: for each of the n keys that is not done (done ==
// nullptr: none is) the next min(width, ...) records of cand[key_off[i] + cursor[i] ..) below
// min(key_off[i + 1], cand_cap) (advance_take, rf_advance_plan.h; first: every cursor counts as 0)
// to out_cand[< out_cap] and out_key[< out_cap] (nullptr: not written), the true total to
// *out_count, cursor[i] += the records written; scratch: advance_scratch_bytes(n) bytes, 8-byte
// aligned
int rf_launch_found_advance(void* stream, const uint64_t* key_off, const uint64_t* cand, uint64_t cand_cap,
                            uint64_t n, uint32_t width, int first, const uint8_t* done, uint32_t* cursor,
                            uint64_t* out_cand, uint64_t* out_key, uint64_t out_cap, uint64_t* out_count,
                            void* scratch);
// diagnostics (rf_amd_diag_fanout_max_blocks): a cap on both kernels' grids; 0 = none
void rf_advance_set_max_blocks(uint32_t blocks);

// ---- estimate, hashing, routing, verify ---------------------------------------------------
// bitmap (zeroed by the caller, bitmap_words a multiple of 4) -> counters[0] = entries
// decoded, counters[1] = distinct fingerprints
int rf_launch_estimate(void* stream, const rf::EstFilter* fl, uint32_t num_filters, uint32_t total_idx, uint32_t lis,
                       uint32_t* bitmap, uint64_t bitmap_words, uint32_t* counters);
// out[i] = XXH32 of key i
int rf_launch_hash(void* stream, int kind, const void* in0, const uint64_t* offs, uint32_t key_len, uint32_t seed,
                   uint64_t n, uint32_t* out);
uint64_t rf_route_scratch_words(uint64_t n, uint32_t world);
// scratch: rf_route_scratch_words(n, world) u32 words; totals: world u64 (device)
int rf_launch_route(void* stream, const uint32_t* hashes, const uint32_t* gfid, uint64_t n, const uint32_t* route,
                    uint32_t num_g, uint32_t world, uint64_t* pairs, uint32_t* perm, uint32_t* scratch,
                    uint64_t* totals);
// found[perm[j]] = back[j]
int rf_launch_unroute(void* stream, const uint64_t* back, const uint32_t* perm, uint64_t n, uint64_t* found);
// *missing += the found words without bit `value`
int rf_launch_count_missing(void* stream, const uint64_t* found, uint64_t n, uint32_t value,
                            unsigned long long* missing);

}  // extern "C"
