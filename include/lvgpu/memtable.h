/*
 * lvgpu memtable order -- the consumer of the WriteBatch op table.  C ABI.
 *
 * WriteBatchInternal::insert_into (write_batch.rs:148-154) hands every op of a
 * batch to MemTable::add (memtable.rs:75-103).  The memtable exists to be
 * walked in internal-key order (its iterator, memtable.rs:146-180) and to
 * answer MemTable::get (memtable.rs:105-143).  lv_memtable_build_device sorts
 * the op table lv_write_batch_decode_device left in HBM (write_batch.h) into
 * that order, on the device; lv_memtable_get_device answers a batch of point
 * lookups over the result.  The skiplist, the arena, reference counting and
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

/* ---- Host twins (pure, no GPU) ----------------------------------------------
 * The same contract over host memory: std::sort by the three rules with the
 * same extent check.  lv_memtable_build_host writes order[0, n) and *totals
 * (status 0 or LV_MT_BUILD_BAD_OP; with BAD_OP order is not written) and
 * returns 0, or LV_ERR_INVALID for a NULL pointer or n > 2^32 - 2.
 * lv_memtable_get_host answers one query over such a table. */
int lv_memtable_build_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops, size_t n,
                           uint32_t *order, lv_mt_totals *totals);
int lv_memtable_get_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops,
                         const uint32_t *order, const lv_mt_totals *totals, const uint8_t *qkey,
                         size_t qkey_len, uint64_t seq, lv_mt_get_result *result);

#ifdef __cplusplus
}
#endif

#endif /* LVGPU_MEMTABLE_H */
