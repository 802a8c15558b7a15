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
 * as it is.  The merging iterator as a streaming object, several output files
 * and version edits are not part of this.
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

#ifdef __cplusplus
}
#endif

#endif /* LVGPU_COMPACT_H */
