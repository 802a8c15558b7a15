/*
 * lvgpu memtable order -- the consumer of the WriteBatch op table.  C ABI.
 *
 * WriteBatchInternal::insert_into (write_batch.rs:148-154) hands every op of a
 * batch to MemTable::add (memtable.rs:75-103).  The memtable exists to be
 * walked in internal-key order (its iterator, memtable.rs:146-180) and to
 * answer MemTable::get (memtable.rs:105-143).  lv_memtable_build_device sorts
 * the op table lv_write_batch_decode_device left in HBM (write_batch.h) into
 * that order, on the device; lv_memtable_get_device answers a batch of point
 * lookups over the result and lv_memtable_range_device a batch of range reads
 * (DBIter's Seek and Next at a snapshot).  The skiplist, the arena, reference counting and
 * add as a mutation are not part of this: the table is built once from an op
 * table and then read.
 *
 * The order.  Entries are ordered by InternalKeyComparator::compare
 * (dbformat.rs:153-170) applied to internal keys (user key || tag), which is
 * what that comparator is written for:
 *
 *   1. user key ascending: bytewise, unsigned bytes, a key that is a proper
 *      prefix of another comes first (BytewiseComparator);
 *   2. then tag descending as a full unsigned 64-bit value: newer sequences
 *      first, and at one sequence VALUE (1) before DELETION (0);
 *   3. then, for entries equal in both, the LATER op in log order first.  The
 *      comparator never returns Equal (it returns Greater on a tie) and
 *      SkipList::insert (skiplist.rs:85-107, :155-185) places a new key before
 *      the first node that is not less than it, so the reference puts a
 *      later-inserted exact duplicate in front.  This makes the order a strict
 *      total order: there is one correct output and stability does not arise.
 *
 * A deliberate difference from the reference.  The reference's own MemTable
 * does NOT produce this order.  MemTable::new gives the skiplist the
 * InternalKeyComparator, but what MemTable::add inserts is the whole encoded
 * entry, varint(klen + 8) || key || tag || varint(vlen) || value.  The
 * comparator therefore takes the entry minus its last 8 bytes for the user key
 * and the last 8 bytes of the value for the tag.  That is why
 * write_batch.rs:293-296 expects "Put(b, vb)@201Put(b, vb)@202" with the TODO
 * "the order is different from cpp", and it would also put key "b" before key
 * "aa", because the length byte is compared first.  That order depends on
 * value bytes and is useless for lookup.  This header implements the
 * comparator's contract, which is C++ LevelDB's order; tests/memtable_cases.py
 * restates the reference's entry compare as a model and tests/test_memtable.py
 * pins both facts.
 */
#ifndef LVGPU_MEMTABLE_H
#define LVGPU_MEMTABLE_H

#include <stddef.h>
#include <stdint.h>

#include "write_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LV_MT_MAX_SEQUENCE ((1ull << 56) - 1)          /* dbformat.rs:35 */

/* Rules 1 and 2 over two internal keys given as (user key, tag): -1 if a comes
 * first, +1 if b comes first, 0 only when key bytes and tag are both equal.
 * Host, pure, no GPU.  A NULL key pointer is allowed with length 0. */
int lv_internal_key_compare(const uint8_t *a, size_t a_len, uint64_t a_tag,
                            const uint8_t *b, size_t b_len, uint64_t b_tag);

/* ---- Build: the op table to memtable order ---------------------------------
 *
 * Inputs.  Op i is d_ops[i], i < *d_n_ops, with key and value extents into
 * d_payload[0, payload_bytes): exactly what lv_write_batch_decode_device
 * wrote.  d_n_ops and d_upstream_status may point at &wb_totals->ops and
 * &wb_totals->status of that call; both are read on the device in stream
 * order, never on the host.  d_upstream_status may be NULL.  Every emitted op
 * is an entry, those of records whose status is not LV_WB_OK included: the
 * reference handed them on before it returned its error.  d_payload may have
 * any byte alignment and keys may start at any byte.
 *
 * Outputs.  d_order[i] is the op index of the i-th entry in memtable order,
 * i < entries (op_cap elements are the caller's).  *d_totals is always
 * written: entries, user_keys = the number of distinct user keys (adjacent
 * entries whose user keys differ, plus one for the first), status =
 * LV_MT_BUILD_* bits.  On any status bit d_order is not written and
 * user_keys is 0:
 *   UPSTREAM  *d_upstream_status != 0: the upstream call wrote no table;
 *             entries = 0.
 *   OP_OVER   *d_n_ops > op_cap: entries = *d_n_ops.
 *   BAD_OP    some op's key or value extent is outside
 *             d_payload[0, payload_bytes), checked in u64 arithmetic that
 *             cannot wrap; entries = *d_n_ops.  No byte outside d_payload is
 *             read: a tile that holds such an op compares nothing, and every
 *             later kernel of the call reads the status and exits.
 *
 * Arguments, checked on the host before any device call (LV_ERR_INVALID,
 * lv_last_error): NULL pointers (d_payload only with payload_bytes == 0, d_ops
 * and d_order only with op_cap == 0; d_upstream_status may always be NULL),
 * d_ops 16-byte aligned, d_order 4-byte aligned, d_totals and d_n_ops 8-byte
 * aligned, d_workspace 16-byte aligned and >=
 * lv_memtable_build_workspace_bytes(op_cap) bytes (not shared with a call that
 * may run concurrently), flags == 0 (none is defined), op_cap <= 2^32 - 2
 * (indices are 32-bit), and d_order[0, op_cap) must not overlap
 * d_ops[0, op_cap) or d_payload[0, payload_bytes).  Without a usable GPU a
 * well-formed call fails with the runtime's error: there is no host fallback.
 *
 * Stream-ordered, no host synchronisation, staging or stream queries.  The
 * launch sequence depends only on op_cap: a one-thread init, the tile sort,
 * ceil(log2(ceil(op_cap / tile))) merge passes, the order kernel and the
 * totals kernel, a linear chain of kernel launches.  Launches whose work lies
 * beyond *d_n_ops return at once.  No workgroup waits on another inside a
 * launch.  It may be captured into a HIP graph once the device has been
 * initialised. */
typedef struct lv_mt_totals {     /* device memory, 8-B aligned, always written */
    uint64_t entries, user_keys, status;
} lv_mt_totals;
#define LV_MT_BUILD_UPSTREAM 1u   /* *d_upstream_status != 0: no table, entries = 0 */
#define LV_MT_BUILD_OP_OVER  2u   /* *d_n_ops > op_cap: entries = *d_n_ops, nothing else written */
#define LV_MT_BUILD_BAD_OP   4u   /* some op's key or value extent is outside d_payload[0, payload_bytes) */

size_t lv_memtable_build_workspace_bytes(size_t op_cap);
int lv_memtable_build_device(const uint8_t *d_payload, size_t payload_bytes,
                             const lv_wb_op *d_ops, const uint64_t *d_n_ops,
                             const uint64_t *d_upstream_status, size_t op_cap,
                             uint32_t *d_order, lv_mt_totals *d_totals, uint32_t flags,
                             void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- Get: MemTable::get (memtable.rs:105-143) for nq queries ----------------
 *
 * Query q is the user key d_qkeys[d_q_off[q], d_q_off[q] + d_q_len[q]) at the
 * snapshot d_q_seq[q].  Over the table in internal-key order:
 *   1. seek to the first entry not less than (user key, (seq << 8) | 1);
 *   2. if there is one and its user key equals the query's: FOUND for a VALUE,
 *      with val_off / val_len the value's extent in d_payload, DELETED for a
 *      DELETION; op = the op index of that entry;
 *   3. otherwise ABSENT.
 * Every field of d_results[q] is written; those a status does not set are 0.
 * A query whose snapshot is above LV_MT_MAX_SEQUENCE is BAD_SEQ (the
 * reference asserts) and is not searched; one whose key extent is outside
 * d_qkeys[0, qkeys_bytes) (u64 arithmetic that cannot wrap) is BAD_QUERY and
 * no byte of it is read.  If the build's status is not 0 every query is
 * NO_TABLE.  d_payload, payload_bytes, d_ops, d_order and d_totals must be
 * those of the build.
 *
 * One launch that reads *d_totals on the device, so it can follow the build
 * on the stream unsynchronised; capturable like the build.  Arguments checked
 * on the host (LV_ERR_INVALID): NULL pointers (d_payload only with
 * payload_bytes == 0, d_qkeys only with qkeys_bytes == 0, the query arrays and
 * d_results only with nq == 0; d_ops and d_order may be NULL for a table that
 * can only be empty), d_ops 16-byte aligned, d_order and d_q_len 4-byte
 * aligned, d_totals, d_q_off, d_q_seq and d_results 8-byte aligned,
 * flags == 0, nq <= 2^32 - 2. */
#define LV_MT_GET_ABSENT    0u   /* MemTable::get -> None */
#define LV_MT_GET_FOUND     1u   /* Some(Ok(value)): val_off / val_len / op set */
#define LV_MT_GET_DELETED   2u   /* Some(Err(NotFound)): op set */
#define LV_MT_GET_BAD_SEQ   3u   /* snapshot > LV_MT_MAX_SEQUENCE (the reference asserts); not searched */
#define LV_MT_GET_NO_TABLE  4u   /* the build's status != 0 */
#define LV_MT_GET_BAD_QUERY 5u   /* key extent outside d_qkeys[0, qkeys_bytes); not read */
typedef struct lv_mt_get_result { /* 24 bytes */
    uint64_t val_off;
    uint32_t val_len, op, status, reserved;
} lv_mt_get_result;

int lv_memtable_get_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops,
                           const uint32_t *d_order, const lv_mt_totals *d_totals,
                           const uint8_t *d_qkeys, size_t qkeys_bytes, const uint64_t *d_q_off,
                           const uint32_t *d_q_len, const uint64_t *d_q_seq, size_t nq,
                           lv_mt_get_result *d_results, uint32_t flags, void *stream);

/* ---- Range: DBIter's forward walk (Seek, Next*) for nq ranges ---------------
 *
 * Honesty first.  The algorithm is upstream C++ LevelDB's DBIter
 * (db/db_iter.cc: Seek, Next, FindNextUserEntry).  The reference this project
 * is modelled on has the iterator traits (iterator.rs) and no DBIter, so
 * there is nothing of it to compare with, and parity with a stock LevelDB is
 * UNPINNED: no stock build was run against this.  What pins the behaviour is
 * the worked example below (hand-derived; tests/golden/mt_range_example.json),
 * the independent Python model written from FindNextUserEntry
 * (tests/mt_range_cases.py), the host twin, and the Get-agreement rule: a
 * range [k, k + "\0") with limit 1 has count == 1 exactly when
 * lv_memtable_get says FOUND, and then hits[0] is Get's op (over tables whose
 * tags are VALUE or DELETION: Get reads any other type as a deletion, DBIter
 * skips such an entry as unparsable, step 4).
 *
 * The table is the sorted quadruple (d_payload, d_ops, d_order, *d_totals) a
 * memtable build, a scan with d_order or a compaction filter wrote.  Let
 * n = totals->entries, e_i = ops[order[i]], type(e) = tag & 0xff,
 * seq(e) = tag >> 8 and s = query.seq.  Entry i STARTS A GROUP iff i == 0 or
 * the user keys of e_i and e_{i-1} differ (bytes and lengths).  Query q, over
 * key extents into d_qkeys, is answered by this serial loop, which
 * lv_memtable_range_host runs as written:
 *
 *   1. Statuses, in this order.  NO_TABLE: totals->status != 0, n > op_cap,
 *      or n != 0 with null ops / order.  BAD_SEQ: s > LV_MT_MAX_SEQUENCE.
 *      BAD_QUERY: unknown flag bits; SEEN without RESUME; a needed key extent
 *      (lo without RESUME, hi with HAS_HI) outside d_qkeys[0, qkeys_bytes),
 *      in u64 arithmetic that cannot wrap, and no byte of it is read; RESUME
 *      with pos > n.  With any of them count = 0, every other field is 0 and
 *      the query's slot of d_hits is untouched.
 *   2. start: without RESUME the first position whose entry is not less than
 *      (lo, (s << 8) | 1) under InternalKeyComparator (lv_memtable_get's
 *      seek, upstream's Seek); with RESUME, pos.  seek_pos = start.
 *   3. end: with HAS_HI the first position whose user key is >= hi, else n.
 *      end < start behaves like end = start.
 *   4. With seen = RESUME && SEEN, p = start, count = examined = unparsed = 0:
 *        if count == limit: MORE_LIMIT, stop;
 *        if p >= end: DONE, stop;
 *        if examined == max_scan: MORE_SCAN, stop;
 *        e = e_p, ++p, ++examined;
 *        if e starts a group: seen = false;
 *        if type(e) > 1: ++unparsed, next (upstream's ParseKey fails and the
 *          entry is skipped; the state is untouched);
 *        if seq(e) > s: next (invisible to the snapshot);
 *        if seen: next (hidden behind a newer visible entry of its user key);
 *        seen = true; if e is a deletion: next (it shows nothing);
 *        hits[count++] = order[p - 1].
 *      At a stop next_pos = p and result.seen = seen.
 *   5. A later query {RESUME | (seen ? SEEN : 0), pos = next_pos} with the
 *      same seq and hi continues the walk exactly: because of the group rule
 *      (next_pos, seen) is the loop's whole state.  The concatenated hits and
 *      the summed unparsed of a chain of calls are those of one call with a
 *      large limit and max_scan.
 *   6. On a sorted order this is DBIter's forward iteration at snapshot s.
 *   7. start and end are defined on a sorted order.  On an unsorted order, or
 *      a quadruple whose parts were not written for each other, the call
 *      reads nothing outside its buffers, terminates within max_scan entries
 *      per query and writes count <= limit hits inside the query's slot;
 *      which hits is unspecified, and so is which entries a search probes.
 *   8. An order index >= op_cap, or a key extent outside
 *      d_payload[0, payload_bytes), that the walk or a search meets makes the
 *      query NO_TABLE with count = 0 and every other field 0 (what mt_get
 *      does).  The slot may then hold partial writes; nothing outside
 *      d_hits[q * limit, (q + 1) * limit) is written.  The walk meets e_p of
 *      every iteration of step 4 and, in the first, e_{start-1}.
 *   9. With any status nothing at or beyond d_hits[q * limit + count] inside
 *      the slot is written, except in the NO_TABLE case of step 8.
 *
 * The worked example (limit 4, M = LV_MT_MAX_SEQUENCE; entries by position as
 * (user key, sequence, value | DEL | type); hits are positions and stand for
 * order[position]):
 *    0 (a,5,"a5")  1 (a,3,DEL)   2 (a,1,"a1")  3 (b,9,"b9")   4 (b,4,"b4")
 *    5 (c,7,DEL)   6 (c,6,"c6")  7 (d,8,type 2)  8 (d,2,"d2")  9 (e,10,"e10")
 *
 *   query                          seek hits     count next seen unparsed status
 *   lo "", seq M                     0  0 3 8 9    4    10    1     1     MORE_LIMIT
 *                                       (the limit is judged before the end)
 *   lo "a", seq 4                    1  4 8        2    10    0     1     DONE
 *                                       (a's deletion at 3 hides a1)
 *   lo "b", hi "d", seq 6            4  4 6        2     7    1     0     DONE
 *                                       (c's deletion at 7 is above the snapshot)
 *   lo "a", seq M, max_scan 2        0  0          1     2    1     0     MORE_SCAN
 *   RESUME|SEEN, pos 2, seq M,       2  3 8 9      3    10    1     1     DONE
 *     max_scan 100                      (a1 stays hidden)
 *   lo "f", seq M                   10  -          0    10    0     0     DONE
 *   lo "c", hi "b", seq M            5  -          0     5    0     0     DONE
 *
 * One launch, one wave per query, that reads *d_totals on the device:
 * stream-ordered, no host synchronisation, workspace, staging or memset;
 * capturable like the build.  Arguments checked on the host (LV_ERR_INVALID,
 * lv_last_error): NULL pointers (d_payload only with payload_bytes == 0,
 * d_qkeys only with qkeys_bytes == 0, d_queries, d_hits and d_results only
 * with nq == 0; d_ops and d_order both or neither, NULL for a table that can
 * only be empty), d_ops 16-byte aligned, d_order and d_hits 4-byte aligned,
 * d_totals, d_queries and d_results 8-byte aligned, flags == 0,
 * limit >= 1, max_scan >= 1, nq <= 2^32 - 2, nq * limit <= 2^40 (in u64), and
 * d_hits[0, nq * limit) and d_results[0, nq) overlap neither each other nor
 * d_payload, d_ops[0, op_cap), d_order[0, op_cap), *d_totals, d_qkeys or
 * d_queries[0, nq).
 *
 * Out of scope: reading ranges straight from table images (a version's range
 * goes through scans and a memtable build), reverse iteration (Prev,
 * SeekToLast) and a streaming merging iterator. */
#define LV_MT_RANGE_HAS_HI  1u   /* hi is given: stop in front of the first entry whose user key >= hi */
#define LV_MT_RANGE_RESUME  2u   /* start at order position `pos`, lo is ignored */
#define LV_MT_RANGE_SEEN    4u   /* with RESUME: the group that holds entry pos-1 already showed its visible entry */
typedef struct lv_mt_range_query {   /* 48 bytes, 8-B aligned */
    uint64_t lo_off, hi_off, seq, pos;      /* key extents into d_qkeys; seq the snapshot */
    uint32_t lo_len, hi_len, flags, reserved;
} lv_mt_range_query;
typedef struct lv_mt_range_result {  /* 40 bytes, every field always written */
    uint64_t seek_pos, next_pos, unparsed;
    uint32_t count, status, seen, reserved;
} lv_mt_range_result;
#define LV_MT_RANGE_DONE        0u   /* hi or the end of the table reached */
#define LV_MT_RANGE_MORE_LIMIT  1u   /* count == limit */
#define LV_MT_RANGE_MORE_SCAN   2u   /* max_scan entries examined */
/* 3, 4, 5 = LV_MT_GET_BAD_SEQ, NO_TABLE, BAD_QUERY, with Get's meaning and order */

int lv_memtable_range_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops,
                             const uint32_t *d_order, const lv_mt_totals *d_totals, size_t op_cap,
                             const uint8_t *d_qkeys, size_t qkeys_bytes, const lv_mt_range_query *d_queries,
                             size_t nq, uint32_t limit, uint64_t max_scan, uint32_t *d_hits /* nq * limit */,
                             lv_mt_range_result *d_results, uint32_t flags, void *stream);

/* ---- Host twins (pure, no GPU) ----------------------------------------------
 * The same contract over host memory: std::sort by the three rules with the
 * same extent check.  lv_memtable_build_host writes order[0, n) and *totals
 * (status 0 or LV_MT_BUILD_BAD_OP; with BAD_OP order is not written) and
 * returns 0, or LV_ERR_INVALID for a NULL pointer or n > 2^32 - 2.
 * lv_memtable_get_host answers one query over such a table.
 * lv_memtable_range_host answers one range query (the serial loop above, its
 * searches plain binary searches) into hits[0, limit) and *result; it returns
 * LV_ERR_INVALID for a NULL totals, query, hits or result, a NULL payload or
 * qkeys with bytes, limit == 0 or max_scan == 0. */
int lv_memtable_build_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops, size_t n,
                           uint32_t *order, lv_mt_totals *totals);
int lv_memtable_get_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops,
                         const uint32_t *order, const lv_mt_totals *totals, const uint8_t *qkey,
                         size_t qkey_len, uint64_t seq, lv_mt_get_result *result);
int lv_memtable_range_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops,
                           const uint32_t *order, const lv_mt_totals *totals, size_t op_cap, const uint8_t *qkeys,
                           size_t qkeys_bytes, const lv_mt_range_query *query, uint32_t limit, uint64_t max_scan,
                           uint32_t *hits /* limit */, lv_mt_range_result *result);

#ifdef __cplusplus
}
#endif

#endif /* LVGPU_MEMTABLE_H */
