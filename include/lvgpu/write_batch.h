/*
 * lvgpu WriteBatch -- the consumer of the WAL's logical records.  C ABI.
 *
 * Every logical record of a LevelDB log is a WriteBatch::rep
 * (write_batch.rs:46-55):
 *
 *   rep    := sequence: fixed64, count: fixed32, entry[count]
 *   entry  := VALUE (1) varstring varstring | DELETION (0) varstring
 *   varstring := len: varint32, data: u8[len]
 *
 * Recovery walks each record with WriteBatch::iterate (write_batch.rs:92-122),
 * driven by WriteBatchInternal::insert_into (:148-154): a MemTableInserter
 * (:178-188) hands entry i to the memtable under the sequence number
 * sequence + i, which the memtable packs as (seq << 8) | type (memtable.rs:95).
 *
 * lv_write_batch_iterate is that walk on the host, one rep at a time.
 * lv_write_batch_decode_device is the same walk over the records
 * lv_wal_decode_device left in HBM (wal.h): it turns them into a flat,
 * log-ordered table of operations -- internal-key tag, key extent, value
 * extent -- with a per-record status that restates the reference's error
 * returns, and nothing comes back to the host.
 */
#ifndef LVGPU_WRITE_BATCH_H
#define LVGPU_WRITE_BATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LV_WB_HEADER_SIZE 12u          /* write_batch.rs:28-29 */
#define LV_WB_TYPE_DELETION 0u         /* dbformat.rs:39-40 */
#define LV_WB_TYPE_VALUE 1u

/* per-record status: what WriteBatch::iterate returned for this rep */
#define LV_WB_OK 0u
#define LV_WB_TOO_SMALL 1u     /* "malformed WriteBatch (too small)" */
#define LV_WB_BAD_VARINT 2u    /* "Error when decoding varint-32" */
#define LV_WB_BAD_LENGTH 3u    /* "Input slice doesn't contain a length-prefixed encoded value." */
#define LV_WB_WRONG_COUNT 4u   /* "WriteBatch has wrong count" */
#define LV_WB_BAD_TAG 5u       /* tag byte > 1: the reference panics here ("invalid tag") */
#define LV_WB_OUT_OF_RANGE 6u  /* device only: record extent outside d_payload[0, payload_bytes); not read */

typedef struct lv_wb_op {      /* 32 bytes, the same on host and device */
    uint64_t tag;              /* ((sequence + i) << 8) | type, wrapping u64: memtable.rs:95 */
    uint64_t key_off, val_off; /* byte offsets (host: into rep; device: into d_payload) */
    uint32_t key_len, val_len; /* DELETION: val_off = key_off + key_len, val_len = 0 */
} lv_wb_op;

/* WriteBatch::iterate with a MemTableInserter as its Handler
 * (write_batch.rs:92-122, :178-188), over rep[0, n).  Host, pure, no GPU.
 *
 *   n < 12                      LV_WB_TOO_SMALL, no ops.
 *   entries from byte 12 while input remains: a tag byte, then a key
 *   varstring, then for VALUE a value varstring.  A tag above 1 is
 *   LV_WB_BAD_TAG (the reference panics; nothing is handed on for it).
 *   varint32 as coding.rs:186-204 decodes it: at most 5 bytes, the bits of the
 *   fifth byte above bit 31 are discarded; a fifth byte with its continuation
 *   bit set, or input that ends inside the varint, is LV_WB_BAD_VARINT.
 *   a body longer than the remaining input is LV_WB_BAD_LENGTH
 *   (coding.rs:294-305).
 *   An op is handed on only when its whole entry parsed (a VALUE whose value
 *   varstring fails hands on nothing); the ops before a parse error stay
 *   handed on ("Put(foo, bar)@200ParseError()", write_batch.rs:262-274).
 *   After a clean walk, found != count is LV_WB_WRONG_COUNT, with every found
 *   op handed on.
 *
 * Returns LV_WB_*.  *found = the ops handed to the Handler before the return
 * (all of them are valid even when the status is not OK); min(*found, op_cap)
 * of them are written to ops, which may be NULL with op_cap 0 to count.  Op i
 * carries tag = ((sequence + i) << 8) | type in wrapping u64 arithmetic, and
 * offsets into rep.  *sequence / *count = the header fields (0 if TOO_SMALL).
 * found, sequence and count may each be NULL. */
uint32_t lv_write_batch_iterate(const uint8_t *rep, size_t n, lv_wb_op *ops, size_t op_cap,
                                size_t *found, uint64_t *sequence, uint32_t *count);

/* ---- Device: the records of lv_wal_decode_device to an op table in HBM ----
 *
 * Inputs.  Record r is d_payload[d_rec_off[r], d_rec_off[r] + d_rec_len[r]),
 * r < *d_records: exactly what lv_wal_decode_device wrote.  d_records may
 * point at &d_totals->records and d_upstream_status at &d_totals->status of
 * that call; both are read on the device in stream order, never on the host.
 * d_upstream_status may be NULL (no upstream status).  d_payload may have any
 * byte alignment and records may start at any byte; they need not lie end to
 * end, be ordered or be disjoint: any record whose extent lies inside
 * [0, payload_bytes) is decoded.  One whose extent does not (checked in u64
 * arithmetic that cannot wrap) gets LV_WB_OUT_OF_RANGE and no ops, and no byte
 * of it is read.
 *
 * Semantics per record: those of lv_write_batch_iterate above, bit for bit,
 * with key_off / val_off as offsets into d_payload.
 *
 * Outputs (device memory the caller owns).  d_ops holds the ops in log order:
 * record order, then entry order.  d_rec_op is the exclusive prefix of the
 * per-record op counts, *d_records + 1 entries: record r's ops are
 * d_ops[d_rec_op[r] .. d_rec_op[r + 1]).  d_rec_status[r] is LV_WB_*.
 * *d_totals is always written: records = *d_records; ops, key_bytes and
 * value_bytes = the sums over the emitted ops; bad_records = the records whose
 * status is not LV_WB_OK; last_sequence = the unsigned maximum, over the
 * records with at least one emitted op, of sequence + ops - 1 (wrapping per
 * record), or 0 if there is none -- the project's own definition, the
 * reference has no recovery loop to pin it; status = LV_WB_DECODE_* bits.
 *
 * Capacities.  rec_cap is the capacity of d_rec_off / d_rec_len (the decode's
 * rec_cap).  op_cap = payload_bytes / 2 always suffices, because the smallest
 * entry (a DELETION of an empty key) is 2 bytes, so everything can be sized
 * without a round trip.  If a capacity is exceeded, or UPSTREAM is raised,
 * only *d_totals is written, with the true totals and the status bits:
 *   UPSTREAM  *d_upstream_status != 0: the upstream call wrote no arrays, so
 *             the totals are those of zero records (records = 0).
 *   REC_OVER  *d_records > rec_cap: records = *d_records; the arrays do not
 *             hold that many, so nothing is decoded and the other totals are 0.
 *   OP_OVER   total ops > op_cap: all totals are the true ones.
 * Otherwise status == 0.
 *
 * Arguments.  Every argument is checked on the host before any device call
 * (LV_ERR_INVALID, lv_last_error): NULL pointers (d_payload only with
 * payload_bytes == 0, d_ops only with op_cap == 0, the record arrays only
 * with rec_cap == 0; d_rec_op holds rec_cap + 1 entries and is never NULL),
 * d_ops 16-byte aligned, d_totals and d_rec_op 8-byte aligned, d_workspace
 * 16-byte aligned and >= lv_write_batch_decode_workspace_bytes(rec_cap) bytes
 * (not shared with a call that may run concurrently), flags == 0 (no flag is
 * defined yet), rec_cap <= 2^32 - 2, op_cap <= 2^58, and d_ops[0, op_cap)
 * must not overlap d_payload[0, payload_bytes).  Without a usable GPU a
 * well-formed call fails with the runtime's error, like the other batch entry
 * points: there is no host fallback.
 *
 * Reads.  Apart from the records' own bytes the kernels read only the aligned
 * 16-byte granules that hold a record's first and last byte (an aligned
 * granule never leaves a page), and of a record's bytes only the entry
 * headers: keys and values are skipped, not read.
 *
 * Stream-ordered, no host synchronisation, staging or stream queries: one
 * memset and three launches on `stream`, sized by rec_cap (threads beyond
 * *d_records do nothing).  Like lv_wal_decode_device it may be captured into a
 * HIP graph once the device has been initialised. */
#define LV_WB_DECODE_UPSTREAM 1u  /* *d_upstream_status != 0: upstream wrote no arrays; decoded as 0 records */
#define LV_WB_DECODE_REC_OVER 2u  /* *d_records > rec_cap */
#define LV_WB_DECODE_OP_OVER  4u  /* total ops > op_cap */

typedef struct lv_wb_totals {     /* device memory, 8-B aligned, always written */
    uint64_t records, ops, key_bytes, value_bytes, bad_records, last_sequence, status;
} lv_wb_totals;

typedef struct lv_wb_decode_out { /* device memory the caller owns */
    lv_wb_op *d_ops;        size_t op_cap;   /* 16-B aligned */
    uint64_t *d_rec_op;     /* rec_cap + 1 bounds: record r's ops are d_ops[d_rec_op[r] .. d_rec_op[r+1]) */
    uint32_t *d_rec_status; /* rec_cap */
    lv_wb_totals *d_totals;
} lv_wb_decode_out;

size_t lv_write_batch_decode_workspace_bytes(size_t rec_cap);
int lv_write_batch_decode_device(const uint8_t *d_payload, size_t payload_bytes,
                                 const uint64_t *d_rec_off, const uint64_t *d_rec_len,
                                 const uint64_t *d_records, const uint64_t *d_upstream_status,
                                 size_t rec_cap, const lv_wb_decode_out *out, uint32_t flags,
                                 void *d_workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LVGPU_WRITE_BATCH_H */
