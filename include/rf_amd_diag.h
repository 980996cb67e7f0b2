/*
 * rf_amd_diag.h -- diagnostics of the MI355X routing-filter engine (librf_amd.so).
 *
 * Not part of the drop-in's product interface (include/rf_amd.h): hooks the parity tests and
 * the measurement tools use to look inside the engine. None of these has a counterpart in
 * the reference's src/routing_filter.h.
 */
#ifndef RF_AMD_DIAG_H
#define RF_AMD_DIAG_H

#include "rf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the batch's device-only probe lines (64 B each). read_lines copies them to host
 * (h_lines == NULL: only *num_lines is set); rebuild_lines re-cuts them from the filter
 * images with the image-upload kernel (k_plines), so a test can check that the build's
 * lines and the image's lines are byte-identical. */
int rf_amd_debug_read_lines(rf_amd_batch *b, uint8_t *h_lines, uint64_t bytes, uint64_t *num_lines);
int rf_amd_debug_rebuild_lines(rf_amd_batch *b);

/* the probe's memory floor, measured (bench.py `roofline.floor_ms`): one launch of a kernel
 * with k_probe's fast-path memory traffic and wave order over the same runs as
 * rf_amd_batch_probe_{keys,hashes}_runs (key_len 24: 16-byte-aligned keys; 4: hashes) --
 * key staging, one 64-B line gather per probe from its filter, one 8-byte store -- with the
 * hash and the decode replaced by a few integer operations. d_out receives no lookup results. */
int rf_amd_debug_probe_floor(rf_amd_batch *b, const void *d_in, uint32_t key_len, const uint64_t *h_counts,
                             uint64_t *d_out, void *stream);

/* diagnostics library only (librf_amd_stamps.so): a device buffer of 16 u64 per workgroup
 * (NULL = off); the instrumented kernel chosen by `kernel` (1 = bucket sort, 2 = fused
 * partition, 3 = page assembly, 4 = layout) stamps the shader clock at each of its phases
 * into it (tools/phase_times.py). The product library accepts only NULL. */
int rf_amd_debug_phase_buffer(void *d_buf, uint32_t kernel);

/* where the host-buffer lookup round trips (rf_amd_probe_filters_host and the forms built on
 * it) spent their time so far: out[0] calls, out[1] ns before the launch (lookup slot,
 * buffers, ordering after builds, argument packing), out[2] ns in the launch call, out[3] ns
 * waiting for the kernel's completion word and copying the results out. reset != 0 zeroes
 * the counters after reading them. */
int rf_amd_diag_lookup_stats(uint64_t *out, int reset);

/* which way those round trips went, counted where the call decides: out[0] small (hashes and
 * filter descriptors in the kernel arguments), out[1] mapped (the kernel reads the slot's pinned
 * buffer), out[2] copy (one H2D copy first); out[3] those that waited by synchronising the
 * stream (RF_AMD_PROBE_WAIT=sync) instead of polling the completion word. A call with no probes
 * or no groups decides nothing and is not counted. reset != 0 zeroes the counters after reading
 * them. */
int rf_amd_diag_lookup_paths(uint64_t *out, int reset);

/* the lookup server so far: out[0] tickets issued, out[1] server launches, out[2] the first
 * ticket the last exited server did not serve */
int rf_amd_lookup_server_stats(rf_amd_engine *e, uint64_t *out);

/* where the engine's lookup server keeps its request ring: 1 device memory written through the
 * BAR, 0 pinned host memory (RF_AMD_SRV_RING=host, or a box whose BAR mapping failed the
 * check), -1 no server yet */
int rf_amd_diag_lookup_ring(rf_amd_engine *e);

/* stops the engine's lookup server (its wave exits; relaunched waves exit at once) and, gap_us
 * microseconds later, marks it dead with error `err`, exactly as a failed launch or a faulted
 * server stream does: tickets published in the gap are never answered (tests of the error
 * path: every submitted tag must come back through rf_amd_lookup_reap or
 * rf_amd_lookup_server_failed) */
int rf_amd_diag_lookup_server_kill(rf_amd_engine *e, int err, uint32_t gap_us);

/* how many builds of this process ran K4 as the bitmap kernel (k_cb_bitmap: fresh single-run
 * batches whose every filter has an in-bucket key of at most 16 bits, unless
 * RF_AMD_K4_BITMAP=0) instead of the bucket sort: a test reads it before and after a build to
 * see which of the two the build took */
uint64_t rf_amd_diag_k4_bitmap_builds(void);

/* how many filters of this process had their probe lines cut in the dense format (any number of
 * buckets per line; the planner takes it for a filter whose line table outgrows one XCD's L2,
 * RF_AMD_LINES_DENSE=1 for every filter that has a dense geometry, RF_AMD_LINES_DENSE=0 for
 * none), counted per filter at every build and import: a test reads it before and after to see
 * which format its filters took */
uint64_t rf_amd_diag_dense_line_filters(void);

/* how many builds of this process partitioned their keys as 16-bit in-bucket keys, the format
 * the bitmap kernel reads when the partition did not spill, instead of 32-bit entries. The host
 * decides both at once, so the two counters advance together; a build that takes the bucket
 * sort leaves both unchanged */
uint64_t rf_amd_diag_part16_builds(void);

/* how many builds of this process were launched packed: bitmap builds whose every filter has a
 * remainder-and-value field of at most 5 bits and probe lines cut by the assembly kernel, unless
 * RF_AMD_K4_PACK=0. K4 of such a build writes each index block's body instead of the sorted
 * entries, and K6 places the bodies in their pages; a build whose partition spills falls back,
 * on the device, to the sorted entries and is still counted. A batch built this way keeps no
 * entries: an incremental add onto it decodes its image, as for an imported batch */
uint64_t rf_amd_diag_k4_packed_builds(void);

/* process-wide cap on the grid of the fan-out probe (rf_amd_filter_set_probe_*), in workgroups
 * of 256 keys; 0 restores the default, a grid that covers n. With a cap below n / 256 every
 * wave takes several 64-key chunks, so a test of a few thousand keys runs the kernel's
 * grid-stride loop, which otherwise starts only above 2^31 workgroups. Always returns 0.
 * The route kernels of a range map (rf_amd_range_map_route_*) honour the same cap, in workgroups
 * of one tile of rf_amd_diag_range_tile() keys: capped at 1 or 2, a call over three tiles runs
 * every one of their loops more than once per workgroup. */
int rf_amd_diag_fanout_max_blocks(uint32_t blocks);

/* range maps: the keys of one scan tile of a route call (the unit of its scratch and of its
 * grid-stride loops), and the largest num_ranges whose boundary prefixes the search keeps in LDS
 * -- a map with more ranges is searched through L2 by another instance of the kernel, so a test
 * takes one map on each side of it. Both are constants of the build. */
uint32_t rf_amd_diag_range_tile(void);
uint32_t rf_amd_diag_range_lds_ranges(void);
/* the ids one launch of rf_amd_range_map_update_segments carries when it holds one list: a list
 * of one id more is cut into two pieces over two launches. The flatten of an update honours
 * rf_amd_diag_fanout_max_blocks like the route kernels, in tiles of rf_amd_diag_range_tile()
 * ranges. */
uint32_t rf_amd_diag_range_seg_launch_ids(void);
/* the flatten expands a range's list of at most this many ids by one thread and a longer one by
 * a wave: a test takes lists of exactly this length and of one id more */
uint32_t rf_amd_diag_range_seg_thread_ids(void);
/* the 32-bit words of new elements one launch of rf_amd_range_map_split / _set_paths carries: four
 * per new boundary (its prefix and offset), one per four boundary bytes, two per new range (its
 * path's offset) and one per path entry, kinds in that order, each kind rounded up on its own. An
 * edit of one word more takes two launches. The splice honours rf_amd_diag_fanout_max_blocks. */
uint32_t rf_amd_diag_range_splice_words(void);
/* the keys of one tile of rf_amd_found_per_key / _ragged (the unit of their scratch and of their
 * grid-stride loops, which honour rf_amd_diag_fanout_max_blocks like the route kernels);
 * rf_amd_found_advance walks its keys in the same tiles and honours the same cap */
uint32_t rf_amd_diag_per_key_tile(void);
/* the records of one tile of rf_amd_found_by_branch (the unit of its scratch and of its
 * grid-stride loops, which honour rf_amd_diag_fanout_max_blocks too), and the digit passes of its
 * sort for num_members (0 for a num_members the call refuses): a test takes one num_members on
 * each side of every value at which the count changes */
uint32_t rf_amd_diag_by_branch_tile(void);
uint32_t rf_amd_diag_by_branch_passes(uint32_t num_members);

/* the source id the library was built from (16 hex digits of SHA-256 over the engine's
 * sources and headers, splinterdb_amd/build.py source_id): the Python loader refuses a
 * library whose id differs from the tree's (a stale prebuilt .so) */
const char *rf_amd_build_id(void);

#ifdef __cplusplus
}
#endif
#endif
