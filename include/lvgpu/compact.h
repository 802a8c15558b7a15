/*
 * lvgpu compaction filter -- the step that makes the scan -> sort -> build
 * chain a compaction.  C ABI.
 *
 * lv_sst_scan_device turns K table images into one op table (table.h),
 * lv_memtable_build_device sorts it (memtable.h) and lv_sst_build_device writes
 * it out again.  Upstream's DoCompactionWork (db_impl.cc) walks the merged
 * input in internal-key order and drops, before it adds an entry to the output
 * table, every version hidden behind a newer one that all live snapshots can
 * see, and every deletion marker that has nothing beneath it to hide.
 * lv_compact_filter_device is that decision for every entry of a sorted
 * memtable quadruple at once: it writes a second order array that holds the
 * kept entries only, and the totals that go with it.  The result is again a
 * memtable quadruple, which lv_sst_build_device and lv_memtable_get_device take
 * as it is.  lv_compact_output_device (below) writes the kept entries as a run
 * of output tables, and lv_memtable_range_device (memtable.h) reads ranges
 * over either quadruple as DBIter would.  Range reads over a version go
 * through scans and a memtable build for now; reading ranges straight from
 * table images, reverse iteration (Prev, SeekToLast), the merging iterator as
 * a streaming object and version edits are not part of this.
 *
 * The contract: upstream's loop.  The input is (d_payload, payload_bytes,
 * d_ops, d_order, *d_mt_totals), what lv_memtable_build_device or
 * lv_sst_scan_device (with d_order) wrote; n = d_mt_totals->entries, read on
 * the device in stream order, never on the host.  S = smallest_snapshot is a
 * host value below LV_MT_MAX_SEQUENCE.  Walk e_i = d_ops[d_order[i]],
 * i = 0 .. n - 1, with the state has_cur = false, cur (a user key) and
 * last_seq = LV_MT_MAX_SEQUENCE; type = tag & 0xff, seq = tag >> 8:
 *
 *   type > 1 (upstream's ParseInternalKey fails; a scan passes such tags
 *   through): KEEP the entry, has_cur = false, last_seq = MAX; it counts in
 *   `unparsed`.
 *   Otherwise:
 *     if !has_cur or ukey(e_i) != cur (bytewise, lengths included):
 *       cur = ukey(e_i), has_cur = true, last_seq = MAX;
 *     rule A: if last_seq <= S, DROP the entry (dropped_hidden): a newer entry
 *       of this user key is visible to every snapshot;
 *     rule B: else if type == 0 and seq <= S and base_level(ukey), DROP the
 *       entry (dropped_deletions): a deletion with nothing beneath it;
 *     last_seq = seq, whether or not the entry was dropped.
 *
 * S < MAX, so the reset value never satisfies rule A: the first entry of a
 * user key is never dropped as hidden.  The loop runs over the order as given
 * and does not check that it is sorted; an unsorted order yields whatever the
 * loop yields.
 *
 * The same, entry by entry.  The decision depends on e_i and its predecessor
 * p = e_{i-1} alone.  Let prev_seq = seq(p) if p exists, type(p) <= 1 and
 * ukey(p) == ukey(e_i), and MAX otherwise.  When the loop reaches e_i with
 * type(e_i) <= 1, last_seq is prev_seq: if p is missing or type(p) > 1,
 * has_cur is false and last_seq is reset to MAX; otherwise cur is ukey(p) (p
 * either set it or matched it) and last_seq is seq(p), which the comparison
 * with ukey(e_i) keeps or resets to MAX.  So rule A is prev_seq <= S.  The
 * device computes this form, one lane per entry; lv_compact_filter_host runs
 * the loop above with its state, so that the two check each other.
 *
 * Base level.  Without LV_COMPACT_BASE_LEVEL n_ranges must be 0, base_level is
 * false everywhere and rule B never fires.  With it, base_level(k) holds iff
 * no range r < n_ranges has lo_r <= k <= hi_r (bytewise): upstream's
 * IsBaseLevelForKey over the files of the deeper levels.  Range r is
 * d_ranges[r], its keys d_range_keys[lo_off, lo_off + lo_len) and
 * [hi_off, hi_off + hi_len).  The ranges are walked linearly, as upstream
 * walks the files, and only for entries that rule B would otherwise drop.
 * With the flag and n_ranges == 0 every key is base level.
 *
 * Outputs.  d_order_out[0, kept) receives the op indices of the kept entries
 * in input order; nothing at or beyond kept is written.  *d_mt_totals_out is
 * an lv_mt_totals: entries = kept, user_keys counted over the kept entries as
 * the memtable build counts it (adjacent kept entries whose user keys differ,
 * plus one for the first), status 0.  (d_payload, d_ops, d_order_out,
 * *d_mt_totals_out) is then a memtable quadruple.  *d_totals is always
 * written; entries_in = d_mt_totals->entries and kept + dropped_hidden +
 * dropped_deletions = entries_in when status is 0.
 *
 * Statuses are bits, decided before any byte of d_order_out is written.  On
 * any of them d_order_out is untouched, *d_mt_totals_out = {0, 0,
 * LV_MT_BUILD_UPSTREAM} (as the scan writes it) and every count but entries_in
 * is 0.
 *   UPSTREAM   d_mt_totals->status != 0.  Nothing else is examined.
 *   BAD_RANGE  a range's lo or hi extent lies outside
 *              d_range_keys[0, range_keys_bytes), or its lo > hi.  The entries
 *              are then not examined.
 *   BAD_INPUT  entries > op_cap; or, with neither bit above, some
 *              d_order[i] >= op_cap (i < entries) or some entry's key extent
 *              lies outside d_payload[0, payload_bytes).  Every entry is
 *              compared or kept, so every entry's key extent counts; values
 *              are not read.  All in u64 arithmetic that cannot wrap, and no
 *              byte outside d_payload is read: an entry is compared only once
 *              both extents are known to be inside.
 *
 * Arguments, checked on the host before any device call (LV_ERR_INVALID,
 * lv_last_error): NULL pointers (d_payload only with payload_bytes == 0; d_ops,
 * d_order and d_order_out only with op_cap == 0; d_ranges only with
 * n_ranges == 0; d_range_keys only with range_keys_bytes == 0), d_ops 16-byte
 * aligned, d_order and d_order_out 4-byte aligned, the three totals and
 * d_ranges 8-byte aligned, d_workspace 16-byte aligned and >=
 * lv_compact_filter_workspace_bytes(op_cap) bytes (not shared with a call that
 * may run concurrently), unknown flag bits, op_cap <= 2^32 - 2,
 * n_ranges <= LV_COMPACT_MAX_RANGES, n_ranges != 0 without
 * LV_COMPACT_BASE_LEVEL, smallest_snapshot >= LV_MT_MAX_SEQUENCE, and
 * d_order_out[0, op_cap) must not overlap d_order[0, op_cap), d_ops[0, op_cap)
 * or d_payload[0, payload_bytes).  Without a usable GPU a well-formed call
 * fails with the runtime's error: there is no host fallback.
 *
 * Stream-ordered, no host synchronisation, staging or stream queries.  The
 * launch sequence depends only on op_cap: a one-thread init that also
 * validates the n_ranges ranges, the flag kernel (one lane per entry, a scan
 * tile per workgroup), the carries (one wave), the scatter, the count of the
 * kept entries' user keys and a one-thread finish, a linear chain of kernel
 * launches.  Launches whose work lies beyond the device-side count return at
 * once.  No workgroup waits on another inside a launch.  It may be captured
 * into a HIP graph once the device has been initialised.
 */
#ifndef LVGPU_COMPACT_H
#define LVGPU_COMPACT_H

#include <stddef.h>
#include <stdint.h>

#include "memtable.h"
#include "version.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LV_COMPACT_BASE_LEVEL 1u     /* flags: rule B is on; base_level(k) = no range holds k */
#define LV_COMPACT_MAX_RANGES 4096u

#define LV_COMPACT_UPSTREAM  1u      /* d_mt_totals->status != 0 */
#define LV_COMPACT_BAD_INPUT 2u      /* entries > op_cap, an order index >= op_cap, a key extent outside d_payload */
#define LV_COMPACT_BAD_RANGE 4u      /* a range's extent outside d_range_keys, or lo > hi */

typedef struct lv_compact_range {    /* 24 bytes; offsets into d_range_keys */
    uint64_t lo_off, hi_off;
    uint32_t lo_len, hi_len;
} lv_compact_range;

typedef struct lv_compact_totals {   /* device memory, 8-B aligned, always written */
    uint64_t entries_in, kept, dropped_hidden, dropped_deletions, unparsed, user_keys, reserved, status;
} lv_compact_totals;

size_t lv_compact_filter_workspace_bytes(size_t op_cap);
int lv_compact_filter_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops,
                             const uint32_t *d_order, const lv_mt_totals *d_mt_totals, size_t op_cap,
                             uint64_t smallest_snapshot, const lv_compact_range *d_ranges, size_t n_ranges,
                             const uint8_t *d_range_keys, size_t range_keys_bytes, uint32_t *d_order_out,
                             lv_mt_totals *d_mt_totals_out, lv_compact_totals *d_totals, uint32_t flags,
                             void *d_workspace, size_t workspace_bytes, void *stream);

/* The host twin (pure, no GPU): the serial loop above over host memory, with
 * has_cur, cur and last_seq as its state.  The same statuses and outputs.
 * Returns 0, or LV_ERR_INVALID for what the device call refuses (pointers,
 * flags, op_cap, n_ranges, smallest_snapshot; alignment and overlap are not
 * checked). */
int lv_compact_filter_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops, const uint32_t *order,
                           const lv_mt_totals *mt_totals, size_t op_cap, uint64_t smallest_snapshot,
                           const lv_compact_range *ranges, size_t n_ranges, const uint8_t *range_keys,
                           size_t range_keys_bytes, uint32_t *order_out, lv_mt_totals *mt_totals_out,
                           lv_compact_totals *totals, uint32_t flags);

/* ---- lv_compact_output_device: a compaction's output as a run of tables ------
 *
 * Upstream's DoCompactionWork adds the kept entries to a TableBuilder and closes
 * the output file as soon as builder->FileSize() >= MaxOutputFileSize() (2 MiB
 * by default), opening the next one with the next entry.  This call writes
 * every output table of a compaction into one arena in HBM, 16-byte aligned
 * one behind the other, together with the lv_sst_table, lv_sst_bloom and
 * lv_version_file record of each, which lv_version_open_device and
 * lv_version_get_device take as they are (version.h).  The only host-side fact
 * a caller then needs is the file count, which lv_version_open_device takes as
 * a host value.
 *
 * The serial contract (lv_compact_output_host runs exactly this).  The input is
 * the memtable quadruple as lv_sst_build_bloom_device takes it.  Walk
 * e_i = d_ops[d_order[i]], i < d_mt_totals->entries:
 *   1. if no file is open, open file k with a fresh TableBuilder (with bloom, a
 *      fresh FilterBlockBuilder too);
 *   2. add(e_i) by the rules of table.h;
 *   3. if the file's flushed bytes, the sum of raw + 5 over its data blocks
 *      written so far (upstream's FileSize()), are >= max_file_bytes: finish
 *      the file (TableBuilder::finish) and close it;
 *   4. at the end, finish an open file.
 * max_file_bytes >= 1.  A cut falls directly behind an add that flushed a
 * block, so every file holds at least one entry, there is no empty last file
 * and files <= data_blocks.
 *
 * The slice rule.  The image of file k is byte for byte what
 * lv_sst_build_bloom_host (without bloom: lv_sst_build_host) writes for the
 * order slice d_order[first_entry, first_entry + entries), its handle pairs
 * included: d_handles holds the pairs of file k from pair index first_handle =
 * sum over j < k of (data_blocks_j + extra), the data blocks, then the filter
 * block if there is one, then metaindex and index: extra = 3 with a filter and
 * 2 without.  Offsets are relative to the file, so
 * lv_sst_verify_blocks_device(d_arena + file_off, file_bytes, d_handles + 2
 * first_handle, data_blocks + extra, ...) takes them as they are.  The caller
 * provides room for block_cap + 3 files_cap pairs.  File k lies at file_off[k] =
 * align16(file_off[k-1] + file_bytes[k-1]), file_off[0] = 0; the up to 15 bytes
 * between two files are never written.
 *
 * Records, each defined by an existing twin over image k:
 *   d_files[k]   {first_entry, entries, file_off, file_bytes, data_blocks,
 *                first_handle, filter_keys (= entries with bloom, else 0), 0}.
 *   d_tables[k]  what lv_sst_open_host writes.
 *   d_blooms[k]  (d_blooms may be NULL) what lv_sst_bloom_open_host writes;
 *                without bloom that is present = 0 and the why the open gives.
 *   d_version_files[k]  (may be NULL: then no bound keys are written and
 *                bound_bytes is 0) what lv_version_file_host writes for number =
 *                first_number + k, the given level, file_off = images_off +
 *                file_off[k], where images_off is the position of d_arena in the
 *                caller's d_images buffer, and file_cap = file_bytes.  Both
 *                bound keys, the internal keys of the file's first and last
 *                entry, are appended behind *d_bound_used, smallest then
 *                largest, file after file, and the cursor is advanced once by
 *                bound_bytes.
 * level must lie in [1, 6]: output files are in key order, which is those
 * levels' order (level 0 is the flush's job).  The call does not judge whether
 * neighbours are strictly ordered; lv_version_open_device does (an exact
 * duplicate astride a cut is its UNSORTED).
 *
 * Statuses are bits, decided once before any byte of any output but *d_totals
 * is written.  On any of them the arena, the handles, every record array and
 * the bound keys are untouched and the cursor is not advanced; *d_totals
 * reports the true entries, files, data_blocks, arena_bytes, handle_pairs
 * (= data_blocks + extra files) and bound_bytes, so one retry suffices, except
 * under NO_TABLE, where everything but status is 0.
 *   NO_TABLE     as LV_SST_BUILD_NO_TABLE (table.h).
 *   HANDLE_OVER  data_blocks > block_cap.
 *   ARENA_OVER   arena_bytes > arena_cap.
 *   BLOCK_LARGE  table.h's meaning, for any file's data, index or filter block.
 *   FILES_OVER   files > files_cap.
 *   BOUND_OVER   with d_version_files: *d_bound_used > bound_keys_cap or
 *                bound_bytes do not fit behind it.
 * An empty memtable gives files = 0, status 0 and writes nothing.  With status 0
 * nothing at or beyond arena_bytes is written.  All sizes and positions are u64.
 *
 * lv_compact_output_arena_bound returns an arena_cap that always suffices when
 * the ops' extents are disjoint (saturating at 2^64 - 1; 0 for op_cap == 0 or
 * bad bloom options): lv_sst_build_bloom_file_bound's derivation (table.h) with
 * the per-file terms taken n = op_cap times, there being at most n files.
 * Without a filter the per-file terms are the metaindex block 13, the footer
 * 48, the index's count and trailer 9, and 15 bytes of alignment: 2
 * payload_bytes + 75 n + 85 n.  With one, add the filters n bpk / 8 + 9 n, the
 * windows' offsets (payload_bytes + 36 n) / 512 over all files plus per file
 * one more offset 4 and the rounding 1, the filter block's fixed part 10 and
 * the metaindex entry 57: + 72 n.
 *
 * Worked example (tests/golden/compact_output_example.json).  Entries
 * ("k", seq 1, "v") and ("m", seq 2, "w"), block_size 1 (every entry a block),
 * restart_interval 16, no filter, max_file_bytes 1: two files.  File 0 is
 * arena[0, 114), byte for byte table.h's one-entry example: its index key is
 * short_successor("k" ...), the key itself.  File 1 is arena[128, 242), the
 * same with "m", tag 2 and "w"; arena[114, 128) is never written.  d_handles =
 * {0,21} {26,8} {39,22} {0,21} {26,8} {39,22}; first_handle = 0 and 3;
 * bound keys "k" 01 01 00.. | "k" 01 01 00.. | "m" 01 02 00.. | "m" 01 02 00..
 * (36 bytes).  The one-file build of the same two entries has "l" + MAXTAG as
 * its first index key (shortest_separator(k, m)), so a build that cuts the
 * index wrongly fails this example.
 *
 * Arguments, checked on the host before any device call (LV_ERR_INVALID,
 * lv_last_error): lv_sst_build_bloom_device's NULL and alignment rules (bloom
 * may be NULL: no filter; d_arena 16-byte aligned, NULL only with arena_cap ==
 * 0; d_files and d_tables NULL only with files_cap == 0; d_bound_used, and
 * d_bound_keys unless bound_keys_cap == 0, needed with d_version_files; every
 * record array and d_bound_used 8-byte aligned), max_file_bytes != 0, level in
 * [1, 6], files_cap <= LV_VERSION_MAX_FILES, first_number + files_cap must not
 * wrap, flags == 0, d_workspace 16-byte aligned and >=
 * lv_compact_output_workspace_bytes(op_cap, block_cap, files_cap) bytes, and no
 * output range may overlap an input range or another output range.  Without a
 * usable GPU a well-formed call fails with the runtime's error.
 *
 * Stream-ordered: a linear chain of kernel launches, no host synchronisation,
 * staging, stream query or memset; the launch sequence and every grid depend
 * only on op_cap, block_cap, files_cap, arena_cap, restart_interval and whether
 * bloom is given; capturable into a HIP graph once the device has been
 * initialised.  The block starts of the run are those of the one-file build
 * (a block starts with an empty builder, and so does a file), so the call
 * begins with lv_sst_build_device's chain; the file starts are a second greedy
 * chain over blocks, fnext(b) a bounded binary search over the scan of raw + 5
 * and the true starts marked by the same pointer doubling.  No workgroup waits
 * on another, launches beyond the device-side counts return at once, and no
 * lane loops over a count of entries, blocks or files. */
typedef struct lv_compact_output_file {   /* 64 bytes, one per output file */
    uint64_t first_entry, entries, file_off, file_bytes, data_blocks, first_handle, filter_keys, reserved;
} lv_compact_output_file;
typedef struct lv_compact_output_totals { /* device memory, 8-B aligned, always written */
    uint64_t entries, files, data_blocks, arena_bytes, handle_pairs, bound_bytes, reserved, status;
} lv_compact_output_totals;
#define LV_COMPACT_OUT_NO_TABLE     1u
#define LV_COMPACT_OUT_HANDLE_OVER  2u   /* data_blocks > block_cap */
#define LV_COMPACT_OUT_ARENA_OVER   4u   /* arena_bytes > arena_cap */
#define LV_COMPACT_OUT_BLOCK_LARGE  8u
#define LV_COMPACT_OUT_FILES_OVER  16u   /* files > files_cap */
#define LV_COMPACT_OUT_BOUND_OVER  32u   /* the bound keys do not fit behind the cursor */

size_t lv_compact_output_workspace_bytes(size_t op_cap, size_t block_cap, size_t files_cap);
uint64_t lv_compact_output_arena_bound(uint64_t payload_bytes, uint64_t op_cap, const lv_sst_build_options *opt,
                                       const lv_sst_bloom_options *bloom);
int lv_compact_output_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops,
                             const uint32_t *d_order, const lv_mt_totals *d_mt_totals, size_t op_cap,
                             const lv_sst_build_options *opt, const lv_sst_bloom_options *bloom, uint64_t max_file_bytes,
                             uint64_t first_number, uint32_t level, uint64_t images_off, uint8_t *d_arena,
                             uint64_t arena_cap, uint64_t *d_handles, size_t block_cap, lv_compact_output_file *d_files,
                             lv_sst_table *d_tables, lv_sst_bloom *d_blooms, lv_version_file *d_version_files,
                             size_t files_cap, uint8_t *d_bound_keys, uint64_t bound_keys_cap, uint64_t *d_bound_used,
                             lv_compact_output_totals *d_totals, uint32_t flags, void *d_workspace,
                             size_t workspace_bytes, void *stream);
/* The host twin (pure, no GPU): the serial loop above over host memory with a
 * real builder per file; the records are read back from the images by
 * lv_sst_open_host, lv_sst_bloom_open_host and lv_version_file_host.  The same
 * statuses and outputs.  arena == NULL with arena_cap == 0 is a sizing pass:
 * only *totals is written, and the capacities are not judged.  Returns 0, or
 * LV_ERR_INVALID for what the device call refuses (alignment and overlap are
 * not checked). */
int lv_compact_output_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops, const uint32_t *order,
                           const lv_mt_totals *mt_totals, size_t op_cap, const lv_sst_build_options *opt,
                           const lv_sst_bloom_options *bloom, uint64_t max_file_bytes, uint64_t first_number,
                           uint32_t level, uint64_t images_off, uint8_t *arena, uint64_t arena_cap, uint64_t *handles,
                           size_t block_cap, lv_compact_output_file *files, lv_sst_table *tables, lv_sst_bloom *blooms,
                           lv_version_file *version_files, size_t files_cap, uint8_t *bound_keys,
                           uint64_t bound_keys_cap, uint64_t *bound_used, lv_compact_output_totals *totals);

#ifdef __cplusplus
}
#endif

#endif /* LVGPU_COMPACT_H */
