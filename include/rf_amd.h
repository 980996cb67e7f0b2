/*
 * rf_amd.h -- C ABI of the MI355X routing-filter engine.
 *
 * Drop-in boundary for SplinterDB's routing filter (reference: vmware/splinterdb,
 * src/routing_filter.h). Plain C types only: device pointers are `void *` / typed
 * pointers into HIP device memory, streams are `hipStream_t` passed as `void *`.
 * Errors follow platform_status (src/platform_linux/platform_status.h): 0 = STATUS_OK,
 * ENOMEM = STATUS_NO_MEMORY, EINVAL = STATUS_BAD_PARAM, ENODEV = no HIP device.
 *
 * Filter images are bit-exact with the reference's page bytes (src/routing_filter.c
 * :599-633 layout, src/PackedArray.c packing). Index slots are RELOCATABLE:
 * slot = data_page_no * page_size + byte_offset; the integration shim
 * adds the mini_alloc'd page address, restoring the reference's absolute slot
 * (src/routing_filter.c:620).
 */
#ifndef RF_AMD_H
#define RF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_AMD_OK        0
#define RF_AMD_ENOMEM    12
#define RF_AMD_ENODEV    19
#define RF_AMD_EINVAL    22
#define RF_AMD_ENOSPC    28  /* a well-formed edit that exceeds a range map's room */

/* per-filter error bits reported in rf_amd_filter_info.error */
#define RF_AMD_ERR_INDEX_OVERFLOW 1u /* > 4096 entries in one index (ref: fp_buffer overflow, :596) */
#define RF_AMD_ERR_BLOCK_TOO_BIG  2u /* one index block > page (ref: writes past page, :603-610) */
#define RF_AMD_ERR_PAGE_CAP       4u /* internal page bound exceeded (never expected)           */
#define RF_AMD_ERR_GEOMETRY       8u /* invalid geometry                                         */

/* mirrors routing_config (src/routing_filter.h:32-40); key_hash is always XXH32 */
typedef struct rf_amd_config {
   uint32_t fingerprint_size; /* 26 (splinterdb.c:147-152, tests/config.c:29) */
   uint32_t log_index_size;   /* 9 library default, 8 tests                   */
   uint32_t seed;             /* 42                                           */
   uint32_t page_size;        /* 4096                                         */
   uint32_t pages_per_extent; /* 32                                           */
} rf_amd_config;

/* mirrors the routing_filter descriptor (src/routing_filter.h:66-72) + image geometry */
typedef struct rf_amd_filter_info {
   uint32_t num_fingerprints;
   uint32_t num_unique;
   uint32_t value_size;
   uint32_t num_indices;
   uint32_t num_pages; /* data pages in the image */
   uint32_t error;     /* RF_AMD_ERR_* bits, 0 on success */
} rf_amd_filter_info;

typedef struct rf_amd_engine rf_amd_engine;
typedef struct rf_amd_batch  rf_amd_batch;

/* ---- engine ------------------------------------------------------------------------ */
int         rf_amd_engine_create(int device, rf_amd_engine **out);
void        rf_amd_engine_destroy(rf_amd_engine *e);
const char *rf_amd_last_error(void);

/* ---- batched device-resident build (the throughput path) ----------------------------
 * A batch = F independent filters, filter f built from the f-th run of `num_new[f]`
 * inputs (runs concatenated in filter order), tagged with value[f]. This coalesces the
 * concurrent routing_filter_add calls SplinterDB issues from its TASK_TYPE_NORMAL
 * workers (src/trunk.c:3821-3835) into one launch sequence. `old` (may be NULL) gives,
 * per filter, a previously built filter (batch, index) whose entries are merged in
 * (routing_filter_add's old_filter, src/routing_filter.c:355-368, 496-544); pass
 * old_batch[f] = NULL for a fresh filter.
 * A filter built on a rejected old filter (one whose rf_amd_filter_info.error is set) is itself
 * rejected: its error holds the old filter's bits besides its own, it finds nothing, and its
 * build reads neither the old filter's slots nor its pages (a rejected filter has none). The
 * rule is applied on the device, in stream order, so create does not wait for the old filter's
 * build and returns OK; the bits show in rf_amd_batch_info after the build. It holds for
 * rf_amd_batch_create_runs and for a trimmed old batch alike.
 */
int rf_amd_batch_create(rf_amd_engine *e, const rf_amd_config *cfg, uint32_t num_filters,
                        const uint32_t *num_new, const uint16_t *value,
                        rf_amd_batch *const *old_batch, const uint32_t *old_index,
                        rf_amd_batch **out);
/* A chained batch: filter f is the end of a chain of num_runs[f] routing_filter_add calls
 * (maplet_compaction_task's loop over a pivot's bundle compactions, src/trunk.c:3815-3868,
 * which keeps only the last filter), built in one build. Run j of filter f has run_len[] inputs
 * tagged run_value[] (both arrays hold every filter's runs, filter-major, run-minor); the
 * inputs of a build call are concatenated in the same order. The result -- pages, slots and
 * descriptor, num_unique included -- is what the reference leaves after adding run 0 onto
 * old_filter (or onto no filter), run 1 onto that, and so on; value_size is the last run's.
 * The build, probe, info, image, trim and estimate calls work on the batch as on any other,
 * and it may be the old filter of a later batch.
 * EINVAL: a filter's values not strictly increasing, a first value narrower than the old
 * filter's value_size, a zero-length run, more than rf_amd_max_fingerprints fingerprints (old
 * filter's included), fingerprint_size + value_size of the last value over 32.
 * Precondition (not checkable): every value is greater than every value already in the old
 * filter, as the trunk guarantees (value = base_num_branches + i). */
int rf_amd_batch_create_runs(rf_amd_engine *e, const rf_amd_config *cfg, uint32_t num_filters,
                             const uint32_t *num_runs,   /* per filter, >= 1                  */
                             const uint32_t *run_len,    /* all runs, filter-major, run-minor */
                             const uint16_t *run_value,  /* same order                        */
                             rf_amd_batch *const *old_batch, const uint32_t *old_index,
                             rf_amd_batch **out);
/* synchronises the device, then releases the batch's memory (routing_filter_dec_ref's
 * release of a superseded filter, src/routing_filter.c:1101-1109) */
void rf_amd_batch_destroy(rf_amd_batch *b);
/* stream-ordered destroy: the caller has ordered every use of b before the current end of
 * `stream` (NULL = engine's); the memory becomes reusable once the stream passes that point.
 * Does not wait. */
int rf_amd_batch_destroy_on(rf_amd_batch *b, void *stream);

/* inputs are DEVICE pointers; all calls are asynchronous on `stream` (NULL = engine's) */
int rf_amd_batch_build_keys(rf_amd_batch *b, const void *d_keys, uint32_t key_len,
                            void *stream);
int rf_amd_batch_build_var_keys(rf_amd_batch *b, const uint8_t *d_bytes,
                                const uint64_t *d_offsets, void *stream);
int rf_amd_batch_build_hashes(rf_amd_batch *b, const uint32_t *d_hashes, void *stream);

/* probes: probe i looks up key i in filter d_filter_id[i]; result = routing_filter_lookup's
 * found_values bit-vector (src/routing_filter.c:985-1073) */
int rf_amd_batch_probe_keys(rf_amd_batch *b, const void *d_keys, uint32_t key_len,
                            const uint32_t *d_filter_id, uint64_t n, uint64_t *d_found,
                            void *stream);
int rf_amd_batch_probe_var_keys(rf_amd_batch *b, const uint8_t *d_bytes,
                                const uint64_t *d_offsets, const uint32_t *d_filter_id,
                                uint64_t n, uint64_t *d_found, void *stream);
int rf_amd_batch_probe_hashes(rf_amd_batch *b, const uint32_t *d_hashes,
                              const uint32_t *d_filter_id, uint64_t n, uint64_t *d_found,
                              void *stream);
/* probes grouped by filter, in filter order: filter f's h_counts[f] probes follow those of
 * filters < f (one batch of routing_filter_lookup calls per filter). The filter of each
 * probe follows from its position: no per-probe filter id is read. */
int rf_amd_batch_probe_keys_runs(rf_amd_batch *b, const void *d_keys, uint32_t key_len,
                                 const uint64_t *h_counts, uint64_t *d_found, void *stream);
int rf_amd_batch_probe_hashes_runs(rf_amd_batch *b, const uint32_t *d_hashes, const uint64_t *h_counts,
                                   uint64_t *d_found, void *stream);
/* the same for variable-length keys: the sum of h_counts keys, key i being
 * d_bytes[d_offsets[i] .. d_offsets[i+1]) as in rf_amd_batch_probe_var_keys */
int rf_amd_batch_probe_var_keys_runs(rf_amd_batch *b, const uint8_t *d_bytes,
                                     const uint64_t *d_offsets, const uint64_t *h_counts,
                                     uint64_t *d_found, void *stream);

/* Host-buffer forms (synchronous), for callers that hold no device memory, e.g. the
 * routing_filter.h shim (shim/routing_filter_amd.c): build batch b from its keys_total host
 * hashes (staged through the engine's pinned buffer, on the engine stream), and probe n host
 * hashes (filter h_filter_id[i], or filter 0 when NULL; ids >= the batch's filters find
 * nothing) into h_found.
 * Lookups (this and the two calls below) are ONE kernel launch per call on one of the
 * engine's lookup slots (own stream, pinned device-mapped buffers, a completion word the
 * host polls): small calls are read by the kernel straight from pinned host memory, large
 * ones copied in once; results are written by the kernel into pinned host memory. They are
 * thread-safe and concurrent callers run concurrently. Batches must be built (a build issued
 * on the engine stream is waited for). */
int rf_amd_batch_build_hashes_host(rf_amd_batch *b, const uint32_t *h_hashes);
/* the same in two steps, for callers that fill the pinned staging buffer themselves (e.g.
 * each thread of a coalesced add copying its own fingerprints, in parallel): stage_begin
 * takes the engine's staging buffer (filter f's hashes at its run offset, runs in filter
 * order) and returns its host address; stage_build uploads it, builds, waits and releases
 * it; stage_abort releases it without building. */
int  rf_amd_batch_stage_begin(rf_amd_batch *b, uint32_t **h_stage);
int  rf_amd_batch_stage_build(rf_amd_batch *b);
void rf_amd_batch_stage_abort(rf_amd_batch *b);
int rf_amd_batch_probe_hashes_host(rf_amd_batch *b, const uint32_t *h_hashes, const uint32_t *h_filter_id,
                                   uint64_t n, uint64_t *h_found);
/* lookups against many resident filters -- of any batches of the engine -- in ONE launch:
 * probe i looks up h_hashes[i] in filter filter_index[g] (NULL: 0) of batches[g], where
 * g = h_group[i] (NULL: 0); g >= num_groups finds nothing. The form of a flush of queued
 * routing_filter_lookup_async states (src/routing_filter.h:130-155) and of trunk_merge_lookup's
 * per-bundle routing_filter_lookup calls (src/trunk.c:6008-6075; routing_filter.h:87-92)
 * gathered together. Each group is probed with its own batch's routing config, so filters of
 * differently configured kvstores may share a call. */
int rf_amd_probe_filters_host(rf_amd_engine *e, rf_amd_batch *const *batches, const uint32_t *filter_index,
                              uint32_t num_groups, const uint32_t *h_hashes, const uint32_t *h_group,
                              uint64_t n, uint64_t *h_found);
/* the same with the probes grouped: group g probes counts[g] consecutive hashes */
int rf_amd_probe_many_hashes_host(rf_amd_engine *e, rf_amd_batch *const *batches,
                                  const uint32_t *filter_index, const uint64_t *counts,
                                  uint32_t num_groups, const uint32_t *h_hashes, uint64_t *h_found);
/* ---- multi-get: resident filter sets, fan-out probes, candidate lists -------------------
 * The device form of the call above, for a multi-get that probes many keys, each against the
 * maplets along its trunk path (trunk_merge_lookup, src/trunk.c:6008-6075, :6295-6330), from
 * device pointers in one launch.
 * A filter set is a resident table of num_members filters of any batches of engine e: member g
 * is filter filter_index[g] (NULL: 0) of batches[g]; batches[g] == NULL is NULL_ROUTING_FILTER
 * (finds nothing). Each member keeps its own batch's routing config (fingerprint_size and
 * log_index_size may differ between members). Members are validated as rf_amd_probe_filters_host
 * validates groups: an unbuilt batch, a batch of another engine or a bad filter index is EINVAL;
 * a member whose build failed finds nothing. create waits for builds issued on the engine
 * stream and allocates the set's device table (from the engine's pool); no later call on the
 * set allocates or synchronises. The set holds pointers into its members' batches and no
 * references: the batches must outlive the set's last probe (the rule of rf_amd_lookup_submit).
 * rf_amd_batch_trim of a member leaves the set valid (pages, slots and probe lines keep their
 * addresses). destroy synchronises the device, as rf_amd_batch_destroy does. */
typedef struct rf_amd_filter_set rf_amd_filter_set;
/* a bundle without a maplet that holds one branch: every key finds value 0 (found word 1)
 * (trunk_ondisk_bundle_merge_lookup, src/trunk.c:6020-6022: found_values = num_branches == 1 ? 1
 * : 0 without a filter call -- the bundles of memtable incorporations). Accepted wherever a set
 * takes a member: batches[i] of rf_amd_filter_set_create, _create_cap and _update;
 * filter_index[i] is ignored, as it is for NULL. A NULL batch stays the bundle with no branch.
 * Such a member has no seed and takes no part in the seed rule of the keys forms; it counts for
 * num_members. Downstream its word 1 is the record index << 8 | 0 of rf_amd_found_compact and
 * member_id << 8 | 0 of rf_amd_found_per_key*, at the member's place in the key's list. */
#define RF_AMD_MEMBER_UNFILTERED ((rf_amd_batch *)(uintptr_t)1)
int  rf_amd_filter_set_create(rf_amd_engine *e, rf_amd_batch *const *batches,
                              const uint32_t *filter_index, uint32_t num_members,
                              rf_amd_filter_set **out);
void rf_amd_filter_set_destroy(rf_amd_filter_set *s);
uint32_t rf_amd_filter_set_num_members(const rf_amd_filter_set *s);
/* Sets that follow compactions (each maplet compaction replaces one bundle's filter,
 * maplet_compaction_task, src/trunk.c:3815-3868): a set with room to grow, members replaced in
 * stream order, and a stream-ordered destroy, so a resident set lives across compactions without
 * a host wait. The intended sequence, all on one stream: build the new batch,
 * rf_amd_filter_set_update, rf_amd_batch_destroy_on the old batch.
 * create_cap is rf_amd_filter_set_create with room for `capacity` members (EINVAL: capacity <
 * num_members, capacity == 0): members [num_members, capacity) start as NULL_ROUTING_FILTER.
 * rf_amd_filter_set_create makes capacity = num_members.
 * update: member member_id[i] becomes filter filter_index[i] (NULL: 0) of batches[i] (NULL batch:
 * NULL_ROUTING_FILTER, which is how a member is cleared), for i < count. Asynchronous on stream
 * (NULL = the engine's): a probe queued there before the call sees the old members, one queued
 * after it the new ones; the caller orders probes on other streams, as for any device-pointer
 * call. The call waits for nothing -- the new members' builds included -- and allocates nothing
 * on the device (nor on the host, while count <= capacity). Calls on one set -- updates, and
 * updates against probes -- are serialised by the caller: the set keeps the call's host scratch.
 * A member's batch must be built in the sense of the other calls (its build has been issued);
 * the caller orders that build before the update, on the same stream or with an event. The
 * member's build error is read on the device, in stream order, so a member whose build is
 * rejected finds nothing without the host ever having read its bits (bits the host knows
 * already, e.g. of an imported batch, travel with the call). rf_amd_batch_trim keeps what the
 * update reads: a trimmed batch may become a member.
 * Ids lie in [0, capacity); num_members becomes max(num_members, largest id + 1) when the call
 * returns, and later probes use it. Slots never set are NULL members, so a gap finds nothing. A
 * set does not shrink and does not grow beyond its capacity (that takes a new set). An id named
 * twice in one call: the last entry wins. The seed rule of the keys forms follows the membership
 * after the update: putting back a member with the common seed makes them legal again.
 * EINVAL, and then nothing has changed -- neither a member nor num_members nor the seed rule: a
 * NULL set; with count > 0 a NULL member_id or batches; an id >= capacity; a batch that is
 * unbuilt or of another engine; a filter index out of range. Every entry is checked before the
 * first is applied. count == 0 is OK and touches nothing. The one exception: a launch that the
 * HIP runtime itself refuses (a faulted stream; the HIP error is in rf_amd_last_error) also
 * returns EINVAL, after the host state has changed and possibly some of the launches have gone
 * out; the set's members are then undefined and the set is good only for destroy.
 * The set still holds addresses and no references: a replaced batch must outlive the last probe
 * ordered before the update.
 * destroy_on is the stream-ordered destroy, as rf_amd_batch_destroy_on: the caller has ordered
 * every use of s before the current end of `stream`; does not wait. */
int rf_amd_filter_set_create_cap(rf_amd_engine *e, rf_amd_batch *const *batches,
                                 const uint32_t *filter_index, uint32_t num_members,
                                 uint32_t capacity, rf_amd_filter_set **out);
uint32_t rf_amd_filter_set_capacity(const rf_amd_filter_set *s);
int rf_amd_filter_set_update(rf_amd_filter_set *s, const uint32_t *member_id,
                             rf_amd_batch *const *batches, const uint32_t *filter_index,
                             uint32_t count, void *stream);
int rf_amd_filter_set_destroy_on(rf_amd_filter_set *s, void *stream);
/* fan-out probes: key i is looked up in the K members d_member[i*K .. i*K+K) (row-major; an
 * id >= num_members finds nothing). d_member == NULL: K must equal num_members and slot j is
 * member j. d_found[i*K + j] = routing_filter_lookup's found_values of key i in that member.
 * Each key is read and hashed once. Asynchronous on stream (NULL = the engine's); all pointers
 * are device memory; a build still in flight is ordered by the caller as for any
 * device-pointer probe.
 * The keys form takes the key lengths of rf_amd_batch_probe_keys (any key_len > 0) and hashes
 * with the members' seed: EINVAL when the non-NULL members' seeds differ (the hashes form has no
 * such restriction). EINVAL: K == 0, d_member == NULL with K != num_members, n * K >= 2^56, and
 * -- unless n == 0, which is OK and touches nothing -- a NULL input or output. */
int rf_amd_filter_set_probe_keys(rf_amd_filter_set *s, const void *d_keys, uint32_t key_len,
                                 const uint32_t *d_member, uint32_t K, uint64_t n,
                                 uint64_t *d_found, void *stream);
int rf_amd_filter_set_probe_hashes(rf_amd_filter_set *s, const uint32_t *d_hashes,
                                   const uint32_t *d_member, uint32_t K, uint64_t n,
                                   uint64_t *d_found, void *stream);
/* the keys form for variable-length keys (SplinterDB's key slices): key i is
 * d_bytes[d_offsets[i] .. d_offsets[i+1]), d_offsets holding n + 1 non-decreasing byte offsets
 * (unchecked, as in rf_amd_batch_probe_var_keys). d_bytes may have any alignment, d_offsets[0]
 * need not be 0, a zero-length key is legal (XXH32 of nothing). Everything else -- members,
 * d_found, the seed rule, the EINVAL cases (a NULL d_bytes, d_offsets or d_found with n > 0),
 * n == 0, asynchronous without allocation or synchronisation -- is rf_amd_filter_set_probe_keys'. */
int rf_amd_filter_set_probe_var_keys(rf_amd_filter_set *s, const uint8_t *d_bytes,
                                     const uint64_t *d_offsets, const uint32_t *d_member,
                                     uint32_t K, uint64_t n, uint64_t *d_found, void *stream);
/* ragged fan-out probes: per-key member lists of any length, as a trunk path gives them (the
 * live inflight bundles and the pivot bundle of each node differ from key to key), without
 * padding to one K. d_member_off holds n + 1 non-decreasing uint64 offsets (unchecked, like the
 * variable-length keys' offsets); key i is looked up in the members d_member[p] for p in
 * [d_member_off[i], d_member_off[i+1]), and d_found[p] = routing_filter_lookup's found_values
 * of that key in that member: the same index p as in d_member. d_member_off[0] need not be 0: a
 * call over a sub-range of a larger CSR writes into the matching sub-range of a whole d_found,
 * and nothing outside [d_member_off[0], d_member_off[n]) is written. A key with an empty list
 * is legal and writes nothing. One key's list holds AT MOST 65,535 ids (a wave's 64 keys then
 * span fewer than 2^32 pairs); longer lists are not detected. An id >= num_members, a NULL
 * member and a member whose build failed find nothing (word 0). Everything else is
 * rf_amd_filter_set_probe_keys': each key is read and hashed once, any key_len > 0 and any
 * alignment, the seed rule of the keys forms (EINVAL when the non-NULL members' seeds differ;
 * not for the hashes form), asynchronous on stream (NULL = the engine's), no allocation, no
 * synchronisation. n == 0 is OK and touches nothing. EINVAL: a NULL set, key_len == 0, with
 * n > 0 a NULL input, d_member, d_member_off or d_found, and n >= 2^56. There is no all-members
 * form: that case has one K, and the calls above cover it.
 * rf_amd_found_compact takes the result as it is: on d_found + d_member_off[0] with m = the
 * number of pairs (d_member_off[n] - d_member_off[0]); a record's index is then the pair's
 * position relative to d_member_off[0]. */
int rf_amd_filter_set_probe_keys_ragged(rf_amd_filter_set *s, const void *d_keys, uint32_t key_len,
                                        const uint32_t *d_member, const uint64_t *d_member_off,
                                        uint64_t n, uint64_t *d_found, void *stream);
int rf_amd_filter_set_probe_var_keys_ragged(rf_amd_filter_set *s, const uint8_t *d_bytes,
                                            const uint64_t *d_offsets, const uint32_t *d_member,
                                            const uint64_t *d_member_off, uint64_t n,
                                            uint64_t *d_found, void *stream);
int rf_amd_filter_set_probe_hashes_ragged(rf_amd_filter_set *s, const uint32_t *d_hashes,
                                          const uint32_t *d_member, const uint64_t *d_member_off,
                                          uint64_t n, uint64_t *d_found, void *stream);
/* existence multi-get (SPLINTERDB_LOOKUP_MIGHT_EXIST, include/splinterdb/splinterdb.h:241,
 * src/lookup_result.h:149-169): answered by the filters alone, the first found_values != 0
 * ending the lookup (src/trunk.c:6036-6043, :6153-6158). The six probe calls with d_exists (n
 * bytes, any alignment) in the place of d_found: d_exists[i] = the OR of the two bits below over
 * key i's list -- its K members in the fixed forms, d_member[d_member_off[i] ..
 * d_member_off[i+1]) in the ragged ones. 0: no bundle of the list can hold the key. Bit 0 set:
 * the reference's existence lookup would stop at a filter hit, so the answer is "might exist"
 * whatever else the list holds. 2 alone: the caller looks the key up in the list's unfiltered
 * bundles. Every one of the n bytes is written, those of keys with empty lists too (0), and
 * nothing outside [d_exists, d_exists + n); no found word is written. Everything else is the
 * probe calls' contract: the member-id rules (an id >= num_members, a NULL member and a member
 * whose build failed add nothing), the seed rule of the keys forms, d_member == NULL in the
 * fixed forms meaning all members (K == num_members), d_member_off[0] any value, at most 65,535
 * ids per list, asynchronous on stream (NULL = the engine's), one launch, no allocation, no
 * synchronisation, n == 0 OK and touching nothing, and the same EINVAL cases with d_exists in
 * d_found's place. */
#define RF_AMD_EXISTS_FILTER_HIT 1u  /* some filter of the key's list found a value */
#define RF_AMD_EXISTS_UNFILTERED 2u  /* the list holds an unfiltered member: its branch decides */
int rf_amd_filter_set_exists_keys(rf_amd_filter_set *s, const void *d_keys, uint32_t key_len,
                                  const uint32_t *d_member, uint32_t K, uint64_t n,
                                  uint8_t *d_exists, void *stream);
int rf_amd_filter_set_exists_var_keys(rf_amd_filter_set *s, const uint8_t *d_bytes,
                                      const uint64_t *d_offsets, const uint32_t *d_member,
                                      uint32_t K, uint64_t n, uint8_t *d_exists, void *stream);
int rf_amd_filter_set_exists_hashes(rf_amd_filter_set *s, const uint32_t *d_hashes,
                                    const uint32_t *d_member, uint32_t K, uint64_t n,
                                    uint8_t *d_exists, void *stream);
int rf_amd_filter_set_exists_keys_ragged(rf_amd_filter_set *s, const void *d_keys, uint32_t key_len,
                                         const uint32_t *d_member, const uint64_t *d_member_off,
                                         uint64_t n, uint8_t *d_exists, void *stream);
int rf_amd_filter_set_exists_var_keys_ragged(rf_amd_filter_set *s, const uint8_t *d_bytes,
                                             const uint64_t *d_offsets, const uint32_t *d_member,
                                             const uint64_t *d_member_off, uint64_t n,
                                             uint8_t *d_exists, void *stream);
int rf_amd_filter_set_exists_hashes_ragged(rf_amd_filter_set *s, const uint32_t *d_hashes,
                                           const uint32_t *d_member, const uint64_t *d_member_off,
                                           uint64_t n, uint8_t *d_exists, void *stream);
/* the set bits of m found_values words as an ordered candidate list: record =
 * index << 8 | value, index ascending, and within one word value DESCENDING (the order in
 * which routing_filter_get_next_value hands them out, src/routing_filter.h:94-105; with the
 * fan-out's index = key * K + slot these are trunk_merge_lookup's (key, bundle, branch)
 * candidates, src/trunk.c:6057-6060). *d_count = the total number of candidates (all of them,
 * also when > cap); only the first cap records are written and nothing is written past
 * d_cand[cap) (cap == 0: d_cand may be NULL). Works on the output of any probe call; after a
 * ragged probe, on d_found + d_member_off[0] with m = the number of pairs, the index being the
 * pair's position relative to d_member_off[0]. The same
 * input gives the same bytes. Asynchronous on stream (NULL = the engine's), three launches, no
 * allocation: d_scratch (8-byte aligned) holds rf_amd_found_compact_scratch_bytes(m) bytes
 * (callable without a device; non-decreasing in m). m == 0 is OK and sets *d_count = 0.
 * EINVAL: NULL d_count, m >= 2^56, a NULL d_found / d_scratch with m > 0. */
uint64_t rf_amd_found_compact_scratch_bytes(uint64_t m);
int rf_amd_found_compact(rf_amd_engine *e, const uint64_t *d_found, uint64_t m,
                         uint64_t *d_cand, uint64_t cap, uint64_t *d_count,
                         void *d_scratch, void *stream);
/* the key-aware compaction: the step between a fan-out probe and the loop that consumes its
 * candidates (trunk_ondisk_bundle_merge_lookup, src/trunk.c:6057-6087: key by key, bundle by
 * bundle, newest first, bndl->branches[idx] per found value, out at the first definitive hit,
 * :6085). The same words as rf_amd_found_compact, in the same order, but a record names its
 * member instead of its pair, and the records come with a CSR over the keys.
 * Fixed form: the words of rf_amd_filter_set_probe_{keys,var_keys,hashes}; the pair of (key i,
 * slot j) is i * K + j, and its member id is d_member[i * K + j], or the slot j with d_member ==
 * NULL. K need not equal any set's size: the call takes no set. Ragged form: the words of
 * rf_amd_filter_set_probe_*_ragged with the same d_found pointer, the same d_member and the same
 * n + 1 offsets: d_found and d_member are indexed by the absolute pair p, d_member_off[0] need not
 * be 0, and nothing outside [d_member_off[0], d_member_off[n]) is read of either. One key's list
 * holds at most 65,535 ids (the probe's limit; longer lists are not detected).
 * d_key_off receives n + 1 uint64, d_key_off[0] = 0; key i owns the candidates
 * [d_key_off[i], d_key_off[i+1]), and *d_count = d_key_off[n] = the total. Offsets and total are
 * always the true values, also when they exceed cap. d_cand[j] = (uint64_t)member_id << 8 | value
 * for j < min(total, cap); nothing is written at or past d_cand[cap) (cap == 0: d_cand may be
 * NULL). The order is exactly rf_amd_found_compact's over the same words -- pair ascending, value
 * descending within a word (routing_filter_get_next_value, src/routing_filter.h:94-105) -- so
 * record j here and record j there describe the same (pair, value), and a key's candidates are
 * contiguous and in list order: the trunk's newest-first path order. member_id is d_member[pair]
 * as stored, all 32 bits, not validated (an id that finds nothing has word 0 and makes no
 * record). d_cand_key is optional (NULL: not written): d_cand_key[j] = the key index i of record
 * j, under the same cap rule.
 * Asynchronous on stream (NULL = the engine's), three launches whatever n is, no allocation, no
 * synchronisation, no atomics on global memory; the same input gives the same bytes. d_scratch
 * (8-byte aligned) holds rf_amd_found_per_key_scratch_bytes(n) bytes (callable without a device;
 * non-decreasing in n; a multiple of 8). n == 0 is OK: it writes d_key_off[0] = 0 and
 * *d_count = 0 and nothing else. EINVAL: a NULL engine, n >= 2^56, a NULL d_key_off or d_count, a
 * NULL d_cand with cap > 0; in the fixed form K == 0, K > 65,535 and n * K >= 2^56; with n > 0 a
 * NULL d_found or d_scratch, and in the ragged form a NULL d_member or d_member_off. */
uint64_t rf_amd_found_per_key_scratch_bytes(uint64_t n);
int rf_amd_found_per_key(rf_amd_engine *e, const uint64_t *d_found, const uint32_t *d_member, uint32_t K,
                         uint64_t n, uint64_t *d_key_off, uint64_t *d_cand, uint64_t *d_cand_key,
                         uint64_t cap, uint64_t *d_count, void *d_scratch, void *stream);
int rf_amd_found_per_key_ragged(rf_amd_engine *e, const uint64_t *d_found, const uint32_t *d_member,
                                const uint64_t *d_member_off, uint64_t n, uint64_t *d_key_off,
                                uint64_t *d_cand, uint64_t *d_cand_key, uint64_t cap, uint64_t *d_count,
                                void *d_scratch, void *stream);
/* group by branch: the step between rf_amd_found_per_key* and a consumer that looks a whole batch
 * up together. Every record member_id << 8 | value names one B-tree,
 * bundle_of[member]->branches[value]; the records come key by key (the order of the loop of
 * trunk_ondisk_bundle_merge_lookup, src/trunk.c:6057-6087), and this call groups them by branch,
 * stably, so that all keys that go into one tree stand side by side and in batch order, with a
 * table of the branches that occur.
 * d_cand, d_count and cap are what a rf_amd_found_per_key* call wrote and was given; the call
 * works on the first m = min(*d_count, cap) records. *d_count is read on the device: the host
 * never waits for it, and every size it needs comes from cap. The sort key of a record c is
 * ((c >> 8) & (2^mb - 1)) << 6 | (c & 63), mb being the bit width of num_members - 1 (0 for one
 * member): for ids below num_members that is (member, value) ascending. Ids at or above
 * num_members are the caller's error; they are masked, not validated, so the call stays in bounds
 * and the result is still defined.
 * d_order[t], t < m, is the position j in d_cand of the record at grouped position t: a
 * permutation of [0, m), ascending in the sort key and stable, so within one branch the records
 * keep their input order, the batch's key order. d_order_key[t] = d_cand_key[d_order[t]] is
 * optional: both pointers non-NULL, or both NULL and it is not produced. d_branch[u] is the full
 * 64-bit record of the first element of branch run u, d_branch_off[u] the start of that run in
 * d_order, and the entry behind the last written branch is m: d_branch_off holds branch_cap + 1
 * words (with branch_cap == 0 it may be NULL and is then not written). *d_num_branches is the
 * true number of runs, also when it exceeds branch_cap. Nothing is written at or past
 * d_branch[branch_cap), d_branch_off[branch_cap + 1) or d_order[cap). With m == 0 the call writes
 * *d_num_branches = 0 and d_branch_off[0] = 0 and nothing else.
 * Asynchronous on stream (NULL = the engine's), no allocation, no synchronisation, no atomics on
 * global memory, no workgroup waits for another; the same input gives the same bytes. The
 * launches are known from num_members alone: a least-significant-digit radix sort in digits of 8
 * bits, four launches per pass -- the histogram, the two levels of its scan and the scatter -- (1 pass up to 4 members, 2 up to 1,024, 3 up to 2^18, else 4) and
 * three for the run table. d_scratch (8-byte aligned) holds
 * rf_amd_found_by_branch_scratch_bytes(cap, num_members) bytes (callable without a device;
 * non-decreasing in cap; a multiple of 8; never 0).
 * EINVAL: a NULL engine; a NULL d_count or d_num_branches; num_members == 0 or > 2^26 (the sort
 * key fits 32 bits); cap >= 2^32; a NULL d_cand, d_order or d_scratch with cap > 0; a NULL
 * d_branch or d_branch_off with branch_cap > 0; a scratch that is not 8-byte aligned; exactly one
 * of d_cand_key and d_order_key NULL. */
uint64_t rf_amd_found_by_branch_scratch_bytes(uint64_t cap, uint32_t num_members);
int rf_amd_found_by_branch(rf_amd_engine *e, const uint64_t *d_cand, const uint64_t *d_cand_key,
                           const uint64_t *d_count, uint64_t cap, uint32_t num_members,
                           uint32_t *d_order, uint64_t *d_order_key,
                           uint64_t *d_branch, uint64_t *d_branch_off, uint64_t branch_cap,
                           uint64_t *d_num_branches, void *d_scratch, void *stream);
/* the stepwise hand-out: the early exit of the lookup loop for a consumer that walks the B-trees
 * branch by branch. The reference walks a key's candidates newest first and stops at the first
 * definitive message (trunk_ondisk_bundle_merge_lookup, src/trunk.c:6057-6087, out at :6085 on
 * lookup_result_should_continue, src/lookup_result.h:150-156; :6310 and :6328 between bundles and
 * nodes). This call hands out, for every key whose lookup is still open, its next `width`
 * records, in batch order and in exactly the form rf_amd_found_by_branch takes; the consumer
 * alternates advance, group by branch, walk the trees, mark keys done, until a call's
 * *d_out_count is 0. With width 1 it does the branch lookups of the reference's loop and none
 * after a definitive hit.
 * d_key_off (n + 1 words), d_cand and cand_cap are what a rf_amd_found_per_key* call wrote and was
 * given; records at or past cand_cap do not exist. d_cursor[i] (n uint32) is the number of key
 * i's records already handed out; the caller owns it between calls. d_done is optional (NULL:
 * every key is open): n bytes at any alignment, a non-zero byte means key i's lookup is complete;
 * the consumer writes it between calls. flags: RF_AMD_ADVANCE_FIRST -- the cursors count as 0 and
 * are not read; all n are written.
 * For key i ascending: a = d_key_off[i] + d_cursor[i], e = min(d_key_off[i+1], cand_cap); take_i =
 * 0 if the key is done or a >= e, else min(width, e - a, 65,535 * 64) (the last term keeps a
 * tile's 32-bit count from overflowing on offsets the call does not validate). The output is the
 * concatenation over i of d_cand[a .. a + take_i); d_out_key (optional, NULL: not written)
 * receives the key index i of every record, the type and meaning of d_cand_key. *d_out_count =
 * the sum of take_i, the true total, also when it exceeds out_cap. Only positions below out_cap
 * are written: nothing at or past d_out_cand[out_cap) or d_out_key[out_cap). d_cursor[i] advances
 * by the number of key i's records written, so a key cut by out_cap gets the rest in the next
 * call and nothing is lost. A cursor that does not advance keeps its value (0 under FIRST);
 * nothing outside d_cursor[0, n) is written.
 * rf_amd_found_by_branch(e, d_out_cand, d_out_key, d_out_count, out_cap, ...) chains behind it
 * with no host read.
 * Asynchronous on stream (NULL = the engine's), three launches whatever n is, no allocation, no
 * synchronisation, no atomics on global memory, no workgroup waits for another; the same input
 * gives the same bytes. d_scratch (8-byte aligned) holds rf_amd_found_advance_scratch_bytes(n)
 * bytes (callable without a device; non-decreasing in n; a multiple of 8; never 0). n == 0 writes
 * *d_out_count = 0 and nothing else.
 * EINVAL: a NULL engine; n >= 2^56; width == 0; unknown flag bits; a NULL d_out_count; a NULL
 * d_out_cand with out_cap > 0; a scratch that is not 8-byte aligned; with n > 0 a NULL d_key_off,
 * d_cursor or d_scratch, and a NULL d_cand with cand_cap > 0. */
#define RF_AMD_ADVANCE_FIRST 1u   /* cursors count as 0 and are not read; they are written */
uint64_t rf_amd_found_advance_scratch_bytes(uint64_t n);
int rf_amd_found_advance(rf_amd_engine *e, const uint64_t *d_key_off, const uint64_t *d_cand,
                         uint64_t cand_cap, uint64_t n, uint32_t width, uint32_t flags,
                         const uint8_t *d_done, uint32_t *d_cursor,
                         uint64_t *d_out_cand, uint64_t *d_out_key, uint64_t out_cap,
                         uint64_t *d_out_count, void *d_scratch, void *stream);
/* ---- range maps: multi-get keys routed to their member lists on the device ----------------
 * What produces the ragged probe's per-key lists. At each node on its trunk path a key takes
 * the last pivot whose key is <= it (trunk_ondisk_node_find_pivot, src/trunk.c:5886-5932,
 * less_than_or_equal under data_key_compare) and from it the node's live inflight bundles and the
 * pivot bundle (trunk_merge_lookup, src/trunk.c:6275-6330). Flattened over the levels, the pivot
 * keys of all nodes cut the key space into R ranges; every key of one range has the same member
 * list, the concatenation along its path. A range map is that table, resident on the device;
 * a route call is an upper-bound search of each key in it and the expansion of the range's list
 * into the CSR that rf_amd_filter_set_probe_*_ragged reads, so a multi-get runs route, ragged
 * probe, rf_amd_found_compact from raw device keys without the host touching a key.
 * The order is the default data_config's: slice_lex_cmp (src/util.h:67-81), unsigned memcmp over
 * the common length, then the shorter key first. A custom key_compare is not supported.
 *
 * create: R = num_ranges >= 1 ranges cut by R - 1 boundary keys: boundary j is
 * h_bound_bytes[h_bound_off[j] .. h_bound_off[j+1]) (R offsets; NULL allowed when R == 1),
 * strictly ascending under slice_lex_cmp. Range r holds the keys k with
 * boundary[r-1] <= k < boundary[r] (range 0: k < boundary[0]; range R-1: k >= boundary[R-2]),
 * i.e. r = the number of boundaries <= k. Range r's member list is
 * h_list[h_list_off[r] .. h_list_off[r+1]) (R + 1 non-decreasing uint64 offsets, h_list_off[0]
 * any value; ids are member ids of whatever filter set the caller probes, not validated).
 * Validated on the host, EINVAL before anything is allocated: num_ranges == 0, NULL arrays where
 * needed, boundary offsets decreasing, boundaries not strictly ascending (equal ones included),
 * list offsets decreasing, a list longer than 65,535 ids (the ragged probe's limit). The table
 * is then copied into pool memory on the engine stream and that stream synchronised, as
 * rf_amd_filter_set_create does. A map is immutable: a trunk change makes a new map and
 * releases the old one with destroy_on behind the route calls that read it (their output is a
 * copy: nothing downstream reads the map). A map holds no reference to any set or batch.
 * destroy synchronises the device; destroy_on is stream-ordered and does not wait (NULL: OK). */
typedef struct rf_amd_range_map rf_amd_range_map;
int  rf_amd_range_map_create(rf_amd_engine *e, uint32_t num_ranges, const uint8_t *h_bound_bytes,
                             const uint64_t *h_bound_off, const uint32_t *h_list,
                             const uint64_t *h_list_off, rf_amd_range_map **out);
void rf_amd_range_map_destroy(rf_amd_range_map *m);
int  rf_amd_range_map_destroy_on(rf_amd_range_map *m, void *stream);
uint32_t rf_amd_range_map_num_ranges(const rf_amd_range_map *m);
uint32_t rf_amd_range_map_max_list(const rf_amd_range_map *m); /* longest list: n * max_list bounds the pairs */
/* route: d_range[i] = key i's range; d_member_off receives n + 1 offsets, d_member_off[0] = 0,
 * key i owning the pairs [d_member_off[i], d_member_off[i+1]); d_member[p] holds the ids of key
 * i's range list in list order; *d_total = d_member_off[n]. The offsets and *d_total are always
 * the true values, also when they exceed pair_cap; nothing is written at or past
 * d_member[pair_cap) (pair_cap == 0: d_member may be NULL). A caller that sizes pair_cap =
 * n * rf_amd_range_map_max_list(m) never overflows and can queue the ragged probe behind the
 * call without reading anything back. Asynchronous on stream (NULL = the engine's), three
 * launches, no allocation, no synchronisation: d_scratch (8-byte aligned) holds
 * rf_amd_range_route_scratch_bytes(n) bytes (callable without a device; non-decreasing in n). The
 * same input gives the same bytes. Keys form: any key_len > 0, any alignment. Var form: key i is
 * d_bytes[d_offsets[i] .. d_offsets[i+1]); d_offsets[0] need not be 0, zero-length keys are
 * legal, a key may have any length. n == 0 is OK: it writes d_member_off[0] = 0 and
 * *d_total = 0 and nothing else. EINVAL: a NULL map, key_len == 0, n >= 2^56, a NULL
 * d_member_off or d_total, and with n > 0 a NULL input, d_range or d_scratch, or a NULL d_member
 * with pair_cap > 0. */
uint64_t rf_amd_range_route_scratch_bytes(uint64_t n);
int rf_amd_range_map_route_keys(rf_amd_range_map *m, const void *d_keys, uint32_t key_len, uint64_t n,
                                uint32_t *d_range, uint64_t *d_member_off, uint32_t *d_member,
                                uint64_t pair_cap, uint64_t *d_total, void *d_scratch, void *stream);
int rf_amd_range_map_route_var_keys(rf_amd_range_map *m, const uint8_t *d_bytes, const uint64_t *d_offsets,
                                    uint64_t n, uint32_t *d_range, uint64_t *d_member_off,
                                    uint32_t *d_member, uint64_t pair_cap, uint64_t *d_total,
                                    void *d_scratch, void *stream);
/* ---- range maps that follow the trunk: shared segments, stream-ordered updates ----------------
 * The flat table above stores, for every range, its own copy of the root's bundles and of every
 * inner node's above it, so a memtable incorporation, a flush or a maplet compaction of an upper
 * node changes all R lists. A map made from segments stores each contribution once. A segment is
 * what one (node, pivot) contributes to a lookup path: the member ids of that pivot's live
 * inflight bundles from inflight_bundle_start (src/trunk.c:1498-1508, :1958-1959), then its
 * pivot bundle (:6275-6330). The map holds S segments; segment s has a fixed capacity cap[s] and
 * a current list of len[s] <= cap[s] ids. Range r has a path, a sequence of segment ids from the
 * root to the leaf, and its list is the concatenation of the current lists of its path's
 * segments in path order. The route calls, their kernels and their output are those above: the
 * map keeps a flat table of the same layout and rewrites it on the device after every update.
 *
 * create_segments: boundaries as rf_amd_range_map_create. Range r's path is
 * h_path[h_path_off[r] .. h_path_off[r+1]) (R + 1 non-decreasing offsets), segment s has room for
 * h_seg_cap[s] ids and starts as h_seg_ids[h_seg_off[s] .. h_seg_off[s+1]) (S + 1 offsets).
 * Validated on the host, EINVAL before anything is allocated: everything rf_amd_range_map_create
 * refuses about boundaries, path or segment offsets decreasing, a path entry >= num_segments, an
 * initial list longer than its capacity, NULL arrays where needed (h_path with every path empty,
 * h_seg_ids with every list empty and all three segment arrays with num_segments == 0 may be
 * NULL), and a range whose path's capacities sum to more than 65,535: the capacities, not the
 * lengths, so that no later update can break the ragged probe's limit. Legal: an empty path (an
 * empty list), cap == 0, num_segments == 0 with all paths empty, a segment in no path, a segment
 * twice in one path (its list appears twice). The image -- the flat table flattened on the host,
 * with room in its list for every path's capacities, the paths, each segment's base, capacity
 * and length, the segments' id slots and the flatten's tile scratch -- goes into one pool block
 * by one copy on the engine stream, which is then synchronised, as for the flat create. destroy
 * and destroy_on are those above. rf_amd_range_map_max_list of such a map is the largest sum of a
 * path's capacities: a bound for the map's life, so pair_cap = n * max_list never overflows
 * whatever updates arrive. rf_amd_range_map_num_segments: S (0 also for a flat map and NULL).
 *
 * update_segments: segment seg_id[i]'s list becomes h_ids[h_ids_off[i] .. h_ids_off[i+1]) (count
 * + 1 offsets), asynchronously on stream (NULL = the engine's), with the semantics of
 * rf_amd_filter_set_update: a route call queued there before it sees the old lists, one queued
 * after it the new ones. The ids travel in kernel arguments -- the host arrays may be reused on
 * return -- in as many launches as they need, followed by the three launches that rewrite the
 * flat table. The call waits for nothing and allocates nothing on the device; the caller orders
 * other streams against it and serialises calls on one map. An id named twice: the last entry
 * wins. count == 0 on a map made from segments is OK and touches nothing. EINVAL, every entry
 * checked before the first launch and nothing changed on the host or the device: a NULL map, a
 * flat map, NULL arrays with count > 0 (h_ids may be NULL when every list is empty), an id >=
 * num_segments, a list longer than its segment's capacity, decreasing offsets. If the HIP
 * runtime refuses a launch the map is good only for destroy.
 * Boundaries and paths change in place only in a map created with room (below); a map made by
 * rf_amd_range_map_create_segments has none, and a leaf split or a new level makes a new map. */
int rf_amd_range_map_create_segments(rf_amd_engine *e, uint32_t num_ranges,
                                     const uint8_t *h_bound_bytes, const uint64_t *h_bound_off,
                                     const uint32_t *h_path, const uint64_t *h_path_off,
                                     uint32_t num_segments, const uint32_t *h_seg_cap,
                                     const uint32_t *h_seg_ids, const uint64_t *h_seg_off,
                                     rf_amd_range_map **out);
uint32_t rf_amd_range_map_num_segments(const rf_amd_range_map *m);
int rf_amd_range_map_update_segments(rf_amd_range_map *m, const uint32_t *seg_id,
                                     const uint32_t *h_ids, const uint64_t *h_ids_off,
                                     uint32_t count, void *stream);
/* ---- range maps that follow node splits: stream-ordered range and path edits -----------------
 * Every flush into a full leaf ends in leaf_split (src/trunk.c:4789): m - 1 new pivot keys
 * (leaf_split_select_pivots, leaf_split_init, :4710-4736) fall strictly inside one range, the
 * parent replaces the child's pivot by one pivot per new leaf (flush_to_one_child, :5258-5340)
 * -- each starting empty, inflight_bundle_start at the end (:5271-5275) -- and every new leaf
 * receives the old leaf's bundles (trunk_node_receive_bundles). In the map's terms one range
 * becomes m ranges, every later range moves up by m - 1, and each new range gets a path of its
 * own. An index_split (:4977) moves no boundary and replaces the paths of a contiguous run of
 * ranges. Segments in no path are legal, so the caller declares spare segments at create, fills
 * them with update_segments, and the edit only names them.
 *
 * create_segments_room: the arguments of rf_amd_range_map_create_segments and the bounds of the
 * map for its life: room->ranges the most ranges, room->bound_bytes the most boundary bytes,
 * room->path_entries the most path entries, room->list_ids the most ids the flat list may need
 * (the sum over ranges of their paths' capacities), room->max_list the largest capacity sum any
 * path may ever have. rf_amd_range_map_max_list returns room->max_list, so pair_cap = n *
 * max_list holds whatever edits arrive. EINVAL: everything create_segments refuses, a NULL room,
 * a room smaller than the initial table in any field, room->max_list > 65,535. The image holds
 * the boundaries and the paths twice (an edit reads one copy and writes the other), everything
 * else once, all sized by room.
 *
 * split: range `range` becomes pieces >= 1 ranges. The pieces - 1 new boundaries are
 * h_bound_bytes[h_bound_off[j] .. h_bound_off[j+1]) (pieces offsets; both NULL allowed with
 * pieces == 1, which replaces the range's path only), strictly ascending under slice_lex_cmp,
 * strictly above the range's lower boundary and strictly below its upper one (range 0 has no
 * lower, range R - 1 no upper; a zero-length boundary can therefore only become the first of the
 * map). New range i's path is h_path[h_path_off[i] .. h_path_off[i+1]) (pieces + 1 offsets).
 * set_paths: the paths of ranges [first, first + count) are replaced likewise (count + 1
 * offsets); count == 0 on a map with room is OK and touches nothing.
 *
 * Both are asynchronous on stream (NULL = the engine's) with the contract of update_segments:
 * nothing is waited for, nothing allocated on the device, the host arrays are free on return.
 * The new boundaries (with their 8-byte prefixes, computed on the host), offsets and paths
 * travel in kernel arguments, in as many launches as they need, each reading one copy of the
 * boundaries and paths and writing the other; the three launches that rewrite the flat table
 * follow. A route call queued on stream before the call sees the old table and the old range
 * numbering -- the copy it reads stays untouched until the next edit on that stream -- and one
 * queued after it the new. rf_amd_range_map_num_ranges is the new R as soon as the call
 * returns. The caller orders other streams against the call and serialises calls on one map.
 * Every check is made before the first launch and a refused call changes nothing on the host or
 * the device. EINVAL: a NULL map, a flat map or one without room, range >= R or first + count >
 * R, pieces == 0, decreasing offsets, a boundary out of order or out of its range, a path entry
 * >= num_segments, a path whose capacities sum to more than room->max_list, NULL arrays where
 * needed. RF_AMD_ENOSPC: a well-formed call that exceeds room in ranges, boundary bytes, path
 * entries or list ids. If the HIP runtime refuses a launch the map is good only for destroy.
 * Out of scope: merging ranges, and growing past room (both make a new map). */
typedef struct {
  uint32_t ranges;
  uint64_t bound_bytes;
  uint64_t path_entries;
  uint64_t list_ids;
  uint32_t max_list;
} rf_amd_range_room;
int rf_amd_range_map_create_segments_room(rf_amd_engine *e, uint32_t num_ranges,
                                          const uint8_t *h_bound_bytes, const uint64_t *h_bound_off,
                                          const uint32_t *h_path, const uint64_t *h_path_off,
                                          uint32_t num_segments, const uint32_t *h_seg_cap,
                                          const uint32_t *h_seg_ids, const uint64_t *h_seg_off,
                                          const rf_amd_range_room *room, rf_amd_range_map **out);
int rf_amd_range_map_split(rf_amd_range_map *m, uint32_t range, uint32_t pieces,
                           const uint8_t *h_bound_bytes, const uint64_t *h_bound_off,
                           const uint32_t *h_path, const uint64_t *h_path_off, void *stream);
int rf_amd_range_map_set_paths(rf_amd_range_map *m, uint32_t first, uint32_t count,
                               const uint32_t *h_path, const uint64_t *h_path_off, void *stream);
/* The engine's lookup server: single lookups -- routing_filter_lookup (src/routing_filter.h:
 * 87-92) and routing_filter_lookup_async states (:130-155) -- without a kernel launch per
 * call. A persistent wave (started on demand on a queue of its own, exiting after 400 us
 * without requests and after an 800 us lifetime -- so a device-wide synchronisation waits at
 * most that long for it; relaunched while lookups continue) polls a ring of requests in
 * device memory that the host writes through its BAR mapping (RF_AMD_SRV_RING=host: pinned
 * host memory) and
 * answers each with filter filter_index of batch b, in submission order. submit queues the
 * lookup of `hash` and returns its ticket; the batch must stay alive until the result is
 * taken. A NULL tag: the caller takes the result with rf_amd_lookup_wait (blocking). A
 * non-NULL tag: the result is delivered by rf_amd_lookup_reap, which returns up to max
 * answered tagged lookups in ticket order (tags[i], found_values[i]) without blocking (0 if
 * none is ready or another thread is reaping). Thread-safe. */
#define RF_AMD_SERVER_RING 4096 /* requests in flight at most (a submit beyond waits for a slot) */
int rf_amd_lookup_submit(rf_amd_engine *e, rf_amd_batch *b, uint32_t filter_index, uint32_t hash,
                         void *tag, uint64_t *ticket);
int rf_amd_lookup_wait(rf_amd_engine *e, uint64_t ticket, uint64_t *found_values);
uint64_t rf_amd_lookup_reap(rf_amd_engine *e, void **tags, uint64_t *found_values, uint64_t max);
/* the server's first error (0: none; sticky: a launch that failed, a faulted stream). Once it
 * is set, submit and wait return it, and rf_amd_lookup_server_failed hands back (consumes) the
 * tags of tagged lookups that will not be answered, so their owners can complete them with an
 * error instead of waiting */
int rf_amd_lookup_server_error(rf_amd_engine *e);
uint64_t rf_amd_lookup_server_failed(rf_amd_engine *e, void **tags, uint64_t max);
/* idle exit and lifetime (microseconds) of the server waves launched from now on (defaults
 * 400 / 800; RF_AMD_SERVER_IDLE_US / _LIFE_US): a host-controlled keep-alive */
int rf_amd_lookup_server_set_times(rf_amd_engine *e, uint64_t idle_us, uint64_t life_us);
/* device-allocation pool of the engine (batch work buffers are recycled across batches; up
 * to RF_AMD_POOL_MIB MiB stay pooled, by default a quarter of the device memory free at
 * engine creation and at most 16 GiB); trim hands pooled blocks back to the device until at
 * most keep_bytes stay pooled */
int rf_amd_engine_pool_stats(rf_amd_engine *e, uint64_t *pooled_bytes, uint64_t *hits, uint64_t *misses);
int rf_amd_engine_pool_trim(rf_amd_engine *e, uint64_t keep_bytes);
/* the most device memory the pool keeps parked for reuse (default: RF_AMD_POOL_MIB, else a
 * quarter of the free memory at creation, at most 16 GiB); trims to it now */
int rf_amd_engine_set_pool_limit(rf_amd_engine *e, uint64_t bytes);
/* the engine's stream (NULL-stream arguments, host-buffer builds and imports run there) and
 * its synchronisation (only that stream, not the device) */
void *rf_amd_engine_stream(rf_amd_engine *e);
int   rf_amd_engine_sync(rf_amd_engine *e);
/* pinned host memory: a read-back target that the DMA engines write at full PCIe rate (a
 * copy into pageable memory goes through the driver's staging buffers) */
int  rf_amd_host_alloc(rf_amd_engine *e, uint64_t bytes, void **out);
void rf_amd_host_free(rf_amd_engine *e, void *p);
/* a completion point after the work queued on the engine stream so far (e.g. one filter's
 * image read-back); fence_wait blocks until it has passed and releases it (once) */
int rf_amd_engine_fence(rf_amd_engine *e, uint64_t *fence);
/* host memory the kernels may write directly (e.g. a page cache's buffer, registered once):
 * rf_amd_batch_place_image stores images there without a staging copy */
int rf_amd_host_register(rf_amd_engine *e, void *p, uint64_t bytes);
int rf_amd_host_unregister(rf_amd_engine *e, void *p);
/* filter f's image straight into host pages (replaces the reference's page fill,
 * src/routing_filter.c:603-633): `table` (rf_amd_host_alloc'd) holds the destination of each
 * of the num_pages image pages (inside registered memory), then each page's disk address,
 * then the destinations of the ceil(num_indices / addrs_per_page) index pages. One call writes
 * pages [first_page, first_page + count) and, with_index, the absolute index slots; the
 * destinations it uses are translated in place (so the ranges of successive calls on one
 * table are disjoint). A refused call (EINVAL: a destination outside the registered ranges,
 * pages outside the filter, addrs_per_page 0 or over page_size / 8, f out of range) writes
 * nothing and leaves the table unchanged. Stream-ordered (NULL: the engine stream): wait with
 * rf_amd_engine_fence before using the pages */
int rf_amd_batch_place_image(rf_amd_batch *b, uint32_t f, uint64_t *table, uint32_t num_pages,
                             uint32_t first_page, uint32_t count, int with_index, uint32_t addrs_per_page,
                             void *stream);
int rf_amd_engine_fence_wait(rf_amd_engine *e, uint64_t fence);
/* Residency control for callers that keep many built batches (the shim's registry):
 * device_bytes = the device memory the batch holds; trim drops its build work buffers,
 * keeping pages, slots, probe lines and plans (lookups, image reads, estimates and use as an
 * old filter through an image decode keep working; incremental adds lose the in-place read
 * of its sorted entries). Stream-ordered on `stream` (NULL = engine's), like destroy_on. */
uint64_t rf_amd_batch_device_bytes(const rf_amd_batch *b);
int      rf_amd_batch_trim(rf_amd_batch *b, void *stream);

/* synchronising accessors */
int rf_amd_batch_info(rf_amd_batch *b, uint32_t f, rf_amd_filter_info *out);
/* all rf_amd_batch_num_filters(b) infos at once: one synchronisation, with `stream` (the
 * build's stream) or, if NULL, the whole device */
int rf_amd_batch_infos(rf_amd_batch *b, rf_amd_filter_info *out, void *stream);
/* copy filter f's image to host: num_pages*page_size bytes and num_indices slots */
int rf_amd_batch_read_image(rf_amd_batch *b, uint32_t f, uint8_t *h_pages,
                            uint64_t pages_bytes, uint64_t *h_slots, uint32_t num_slots);
/* asynchronous D2H of filter f's first pages_bytes of pages and num_slots slots on
 * `stream` (e.g. into hipHostRegister'ed clockcache page buffers); the caller knows the
 * sizes from a previous rf_amd_batch_info or sizes by the reservation */
int rf_amd_batch_read_image_async(rf_amd_batch *b, uint32_t f, void *h_pages, uint64_t pages_bytes,
                                  void *h_slots, uint32_t num_slots, void *stream);
/* device pointers of filter f's image (pages, slots) for zero-copy consumers */
int rf_amd_batch_image_ptrs(rf_amd_batch *b, uint32_t f, void **d_pages, void **d_slots);
uint32_t rf_amd_batch_num_filters(const rf_amd_batch *b);

/* per-stage timing with HIP events recorded on the launch stream. Stages of the last
 * build: 0 partition (fresh builds: fused hash + coarse-bucket partition; incremental: hash
 * + histogram), 1 count/scan (fresh: spill fallback only), 2 scatter (fresh: spill fallback
 * only), 3 bucket sort, 4 big-bucket sort, 5 layout, 6 page assembly + probe lines, 7 whole
 * build; 8 = last probe kernel.
 * Milliseconds, -1 if a stage did not run. */
#define RF_AMD_NUM_TIMINGS 9
/* enable = number of event sets kept (0 = off): each build starts the next set of a ring,
 * so the stages of the last `enable` build+probe rounds can be read without synchronising
 * between them (rf_amd_batch_timings_back: back = 0 is the latest round). A negative
 * enable keeps -enable sets but records only the probe's start and end (every build stage
 * reads back as -1): 2 event records per round instead of 10. */
int rf_amd_batch_set_timing(rf_amd_batch *b, int enable);
int rf_amd_batch_timings_back(rf_amd_batch *b, uint32_t back, float *ms, uint32_t n);
int rf_amd_batch_timings(rf_amd_batch *b, float *ms, uint32_t n);

/* XXH32(key, cfg->seed) of n device-resident keys into d_hashes (data_key_hash as
 * btree_pack computes a compaction's fingerprints, src/btree.c:4020-4024); asynchronous */
int rf_amd_hash_keys(rf_amd_engine *e, const rf_amd_config *cfg, const void *d_keys, uint32_t key_len,
                     uint64_t n, uint32_t *d_hashes, void *stream);
int rf_amd_hash_var_keys(rf_amd_engine *e, const rf_amd_config *cfg, const uint8_t *d_bytes,
                         const uint64_t *d_offsets, uint64_t n, uint32_t *d_hashes, void *stream);

/* Import filter images as a built, probe-only batch (e.g. images all-gathered from the
 * other ranks when probes are replicated rather than routed). Filter f's
 * pages are the infos[f].num_pages * page_size bytes after those of filters < f in
 * `pages`; its relocatable index slots the infos[f].num_indices u64 after those of
 * filters < f in `slots`. device_resident: the buffers are HIP device memory (else host).
 * The batch copies them; probe lines are cut on the device. */
int rf_amd_batch_export(rf_amd_batch *b, void *d_pages, uint64_t pages_bytes, uint64_t *d_slots,
                        uint64_t num_slots, void *stream); /* all filters, packed as import reads them */
int rf_amd_batch_import(rf_amd_engine *e, const rf_amd_config *cfg, uint32_t num_filters,
                        const rf_amd_filter_info *infos, const void *pages, const uint64_t *slots,
                        int device_resident, rf_amd_batch **out);

/* ---- routed probes across ranks (multi-GPU serving) --------------------
 * Each rank owns the filters of a contiguous key range (one filter per trunk pivot,
 * src/trunk.c:4133-4170); a probe may arrive on any rank. rf_amd_route_probes partitions
 * n probes (hash, global filter id) stably by owning rank, d_route[g] = local_id << 8 |
 * rank, into d_pairs = (local_id << 32 | hash) grouped by rank (h_counts[r] pairs for
 * rank r) plus d_perm (pair j came from probe d_perm[j]); it synchronises on the stream
 * to return h_counts. One all-to-all of d_pairs (RCCL, by the caller) hands every rank
 * its probes; rf_amd_batch_probe_pairs probes them against the owner's batch; the
 * reverse all-to-all returns found_values in pair order, and rf_amd_unroute_found
 * scatters them back (d_found[d_perm[j]] = d_back[j]). d_scratch holds
 * rf_amd_route_scratch_bytes(n, world) bytes. Bad filter ids / ranks: EINVAL. */
#define RF_AMD_ROUTE_MAX_WORLD 16
uint64_t rf_amd_route_scratch_bytes(uint64_t n, uint32_t world);
int rf_amd_route_probes(rf_amd_engine *e, const uint32_t *d_hashes, const uint32_t *d_filter_id, uint64_t n,
                        const uint32_t *d_route, uint32_t num_filters, uint32_t world, uint64_t *d_pairs,
                        uint32_t *d_perm, void *d_scratch, uint64_t *h_counts, void *stream);
int rf_amd_batch_probe_pairs(rf_amd_batch *b, const uint64_t *d_pairs, uint64_t n, uint64_t *d_found,
                             void *stream);
int rf_amd_unroute_found(rf_amd_engine *e, const uint64_t *d_back, const uint32_t *d_perm, uint64_t n,
                         uint64_t *d_found, void *stream);

/* ---- drop-in single-filter calls on HOST buffers ------------------------------------
 * rf_amd_filter_add replaces routing_filter_add (src/routing_filter.h:78-85): hashes
 * (32-bit XXH32 of the keys, as btree_pack produces them, src/btree.c:4020-4024) in,
 * relocatable image out. `old_pages/old_slots/old_info` describe old_filter (NULL for
 * NULL_ROUTING_FILTER). Unlike the reference, new_fp_arr is not modified.
 * The image buffers are allocated with malloc and freed with rf_amd_image_free.
 */
typedef struct rf_amd_image {
   rf_amd_filter_info info;
   uint8_t           *pages; /* info.num_pages * page_size bytes */
   uint64_t          *slots; /* info.num_indices slots           */
} rf_amd_image;

int  rf_amd_filter_add(rf_amd_engine *e, const rf_amd_config *cfg, const rf_amd_image *old_filter,
                       rf_amd_image *filter, const uint32_t *new_fp_arr, uint64_t num_new_fp,
                       uint16_t value);
/* num_runs chained routing_filter_add calls in one build (rf_amd_batch_create_runs): run j
 * adds new_fp_arrs[j][0 .. num_new_fp[j]) with values[j] (strictly increasing) onto the
 * result of run j - 1, run 0 onto old_filter; `filter` is the last filter of the chain */
int  rf_amd_filter_add_runs(rf_amd_engine *e, const rf_amd_config *cfg, const rf_amd_image *old_filter,
                            rf_amd_image *filter, const uint32_t *const *new_fp_arrs,
                            const uint64_t *num_new_fp, const uint16_t *values, uint32_t num_runs);
/* replaces routing_filter_lookup (src/routing_filter.h:87-92) for a batch of hashed keys */
int  rf_amd_filter_lookup_hashes(rf_amd_engine *e, const rf_amd_config *cfg,
                                 const rf_amd_image *filter, const uint32_t *hashes, uint64_t n,
                                 uint64_t *found_values);
/* keys-in form: hashes each fixed-length key (XXH32, cfg->seed) on the GPU, as
 * routing_filter_lookup does with data_key_hash (src/routing_filter.c:1011) */
int  rf_amd_filter_lookup_keys(rf_amd_engine *e, const rf_amd_config *cfg,
                               const rf_amd_image *filter, const void *keys, uint32_t key_len,
                               uint64_t n, uint64_t *found_values);
/* the same for variable-length keys in host memory: key i is bytes[offsets[i] .. offsets[i+1]),
 * offsets holding n + 1 non-decreasing byte offsets. Only the byte range the keys occupy,
 * offsets[n] - offsets[0] bytes, is copied to the device, so offsets[0] may be large. */
int  rf_amd_filter_lookup_var_keys(rf_amd_engine *e, const rf_amd_config *cfg,
                                   const rf_amd_image *filter, const uint8_t *bytes,
                                   const uint64_t *offsets, uint64_t n, uint64_t *found_values);
void rf_amd_image_free(rf_amd_image *img);

/* ---- routing_filter_estimate_unique_fp (src/routing_filter.h:169-175, .c:702-848) ------
 * Distinct fingerprints among the first 1/16 of the indices of up to 32 filters, times 16
 * (leaf-split sizing, src/trunk.c:4506). Filters with pages == NULL (filter.addr == 0) or
 * fewer than 16 indices contribute nothing, as in the reference. EINVAL: NULL out-param
 * (STATUS_BAD_PARAM, :710-714), more than MAX_FILTERS = 32 filters, or more decoded entries
 * than num_fingerprints / 12 (the reference asserts, :776-780). */
int rf_amd_estimate_unique_fp(rf_amd_engine *e, const rf_amd_config *cfg, const rf_amd_image *filters,
                              uint64_t num_filters, uint32_t *num_unique_fp);
/* same over device-resident filters: filter i = (batches[i], filter_index[i]); a NULL
 * batches[i] is NULL_ROUTING_FILTER. All batches share one engine and routing config. */
int rf_amd_batch_estimate_unique_fp(rf_amd_batch *const *batches, const uint32_t *filter_index,
                                    uint64_t num_filters, uint32_t *num_unique_fp);
/* routing_filter_estimate_unique_keys (src/routing_filter.h:165-167, .c:1141-1146) */
uint32_t rf_amd_estimate_unique_keys(const rf_amd_filter_info *filter, const rf_amd_config *cfg);

/* ---- asynchronous lookups (routing_filter_lookup_async, src/routing_filter.h:130-155,
 * .c:895-972) ---------------------------------------------------------------------------
 * The reference's lookup coroutine returns ASYNC_STATUS_RUNNING while it waits for a page
 * and calls callback(callback_arg) when it can be resumed. Here one call starts a whole
 * batch of lookups against a built (device-resident) batch: host keys are staged through
 * pinned memory to HBM, probed, and the found_values bit-vectors copied back into h_found,
 * all on `stream` (NULL = the engine's). When h_found is complete, callback(callback_arg)
 * runs on a HIP runtime thread (it must not call HIP). h_filter_id == NULL probes filter 0.
 * poll returns RF_AMD_ASYNC_RUNNING / RF_AMD_ASYNC_DONE (async_status order); free waits for
 * completion first. The keys buffer may be reused as soon as rf_amd_lookup_async returns. */
#define RF_AMD_ASYNC_RUNNING 0
#define RF_AMD_ASYNC_DONE    1
typedef void (*rf_amd_callback_fn)(void *arg);
typedef struct rf_amd_lookup_async_state rf_amd_lookup_async_state;
int  rf_amd_lookup_async(rf_amd_batch *b, const void *h_keys, uint32_t key_len,
                         const uint32_t *h_filter_id, uint64_t n, uint64_t *h_found,
                         rf_amd_callback_fn callback, void *callback_arg, void *stream,
                         rf_amd_lookup_async_state **state);
int  rf_amd_lookup_async_poll(rf_amd_lookup_async_state *state);
int  rf_amd_lookup_async_wait(rf_amd_lookup_async_state *state);
void rf_amd_lookup_async_free(rf_amd_lookup_async_state *state);

/* ---- debug functions (src/routing_filter.h:185-192) ------------------------------------
 * rf_amd_filter_verify replaces routing_filter_verify (.c:1163-1183): every key must find
 * `value`; returns EINVAL (the reference asserts) with *num_missing keys that did not.
 * rf_amd_filter_print replaces routing_filter_print (.c:1260-1286), same text (slots are
 * relocatable), to out_file (a FILE *, NULL = stdout). */
int rf_amd_filter_verify(rf_amd_engine *e, const rf_amd_config *cfg, const rf_amd_image *filter,
                         const void *keys, uint32_t key_len, uint64_t n, uint16_t value,
                         uint64_t *num_missing);
int rf_amd_filter_print(const rf_amd_config *cfg, const rf_amd_image *filter, void *out_file);
/* the same text with the reference's absolute addresses: the filter's index extent address
 * and each index slot as stored on the index pages (src/routing_filter.c:1201-1226) */
int rf_amd_filter_print_abs(const rf_amd_config *cfg, const rf_amd_image *filter, uint64_t filter_addr,
                            const uint64_t *abs_slots, void *out_file);

/* host-side helpers mirroring routing_filter.h (no GPU work) */
uint64_t rf_amd_max_fingerprints(const rf_amd_config *cfg);              /* .h:120-127  */
uint32_t rf_amd_estimate_unique_keys_from_count(const rf_amd_config *cfg,
                                                uint64_t num_unique);     /* .c:1119-1139 */
uint64_t rf_amd_space_use_bytes(const rf_amd_config *cfg, uint32_t num_pages); /* .c:1149 */

#ifdef __cplusplus
}
#endif
#endif
