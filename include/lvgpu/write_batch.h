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
 * Stream-ordered, no host synchronisation, staging or stream queries: four
 * launches on `stream`, sized by rec_cap (threads beyond
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

/* ---- The inverse: ops over a key/value arena to WriteBatch records ----
 *
 * What a writer does before it logs a commit group (DBImpl::Write upstream):
 * WriteBatch::put / delete per op (write_batch.rs:64-78 over coding.rs'
 * encode_length_prefixed_slice), WriteBatchInternal::set_sequence with
 * last_sequence + 1, and WriteBatchInternal::append over the group's batches
 * (write_batch.rs:131-161).  The reps come out end to end in d_out with the
 * (d_rec_off, d_rec_len) arrays lv_wal_encode_device and
 * lv_write_batch_decode_device take, and with the op table over d_out that
 * lv_memtable_build_device takes: the log append and the memtable insert of a
 * commit run from one encode.
 *
 * Inputs.  Record r, r < *d_records, is the ops d_ops[d_rec_op[r] ..
 * d_rec_op[r + 1]): the bounds array lv_write_batch_decode_device writes,
 * *d_records + 1 entries; d_rec_op[0] need not be 0.  Of an op the call reads
 * tag & 0xFF (the type; the other 56 bits are ignored, so a decoded op table
 * feeds in as it is), key_off / key_len and, for a VALUE only, val_off /
 * val_len: a DELETION's value fields are neither read nor checked.  Offsets
 * are into d_src[0, src_bytes) at any alignment; extents may overlap or
 * repeat.  d_records and d_upstream_status are read on the device in stream
 * order; d_upstream_status may be NULL.
 *
 * Outputs, when status == 0.  With ops = d_rec_op[*d_records] - d_rec_op[0]:
 *   d_out[0, out_bytes)  the reps end to end.  Record r with n_r ops is
 *       fixed64 first_sequence + (d_rec_op[r] - d_rec_op[0]) (wrapping u64),
 *       fixed32 n_r, then per op the type byte, varint32(key_len), the key and
 *       for a VALUE varint32(val_len), the value.  A record with no ops is its
 *       12-byte header (WriteBatch::new and set_sequence).  These are the
 *       bytes put / delete calls in op order and set_sequence leave, and what
 *       WriteBatchInternal::append leaves over any split of the record's ops
 *       into batches.
 *   d_rec_off[r], d_rec_len[r]  r < records: the rep's extent in d_out;
 *       d_rec_off[r] is the sum of the earlier lengths.
 *   d_ops_out[j]  j = i - d_rec_op[0] < ops, unless d_ops_out is NULL: the op
 *       lv_write_batch_decode_device writes for that entry of d_out: tag =
 *       ((first_sequence + j) << 8) | type (the record's sequence plus the
 *       index in the record), key_off / val_off into d_out, a DELETION with
 *       val_off = key_off + key_len and val_len = 0.  (d_out, out_bytes,
 *       d_ops_out, &d_totals->ops) goes straight into lv_memtable_build_device.
 *   *d_totals  always written.  records, ops, key_bytes, value_bytes (VALUE
 *       ops only), out_bytes; last_sequence = first_sequence - 1 + ops,
 *       wrapping (DBImpl::Write's last_sequence += count) -- with the ops this
 *       struct reports, so first_sequence - 1 whenever ops is 0; bad_record and
 *       bad_op = 2^64 - 1 unless a bit below sets them.
 *
 * All or nothing.  If a status bit is set, only *d_totals is written.  The
 * bits are judged in this order and the first one raised ends the judging:
 *   UPSTREAM    *d_upstream_status != 0: the totals of zero records.
 *   REC_OVER    *d_records > rec_cap: records = *d_records, the sums 0.
 *   BAD_BOUNDS  not (d_rec_op[r] <= d_rec_op[r + 1] <= op_cap) for some r:
 *               bad_record = the lowest such r, records = *d_records, the
 *               sums 0.  No op is read.
 *   BAD_OP      an op of some record has a type above 1, a key extent outside
 *               [0, src_bytes) or, for a VALUE, a value extent outside it (u64
 *               arithmetic, nothing wraps): bad_op = the lowest such index
 *               into d_ops, bad_record = its record, records = *d_records, the
 *               sums 0.  No byte of d_src is read.
 *   OUT_OVER    out_bytes > out_cap: every total is the true one, so the
 *               caller can size and call again.  12 records + 11 ops +
 *               key_bytes + value_bytes always suffices (a header; a type byte
 *               and two varint32 of at most five bytes per op).
 *
 * Arguments.  Every argument is checked on the host before any device call
 * (LV_ERR_INVALID, lv_last_error): NULL pointers (out, d_totals, d_records and
 * d_rec_op always; d_src only with src_bytes == 0, d_ops only with op_cap ==
 * 0, d_out only with out_cap == 0, d_rec_off / d_rec_len only with rec_cap ==
 * 0; d_ops_out may be NULL, and then no op table is written), d_ops and
 * d_ops_out 16-byte aligned, d_totals, d_rec_op, d_rec_off and d_rec_len
 * 8-byte aligned, d_workspace 16-byte aligned and >=
 * lv_write_batch_encode_workspace_bytes(rec_cap, op_cap) bytes (not shared
 * with a call that may run concurrently), flags == 0 (no flag is defined yet),
 * rec_cap <= 2^32 - 2, op_cap <= 2^30 -- a record's count is a fixed32, and
 * with u32 lengths an op's entry is below 2^33 + 11 bytes, so no sum of sizes
 * over 2^30 ops and 2^32 headers can leave u64 --, d_out[0, out_cap) must not
 * overlap d_src, d_ops or d_ops_out, and d_ops_out must not overlap d_ops.
 * Without a usable GPU a well-formed call fails with the runtime's error:
 * there is no host fallback.
 *
 * Reads and writes.  Nothing is read outside d_rec_op[0 .. *d_records], the
 * ops of the records and, once every op has been accepted, their extents of
 * d_src; nothing is written outside d_out[0, out_bytes), the first `records`
 * entries of d_rec_off / d_rec_len, d_ops_out[0, ops) and *d_totals, whatever
 * the inputs say.
 *
 * Stream-ordered, no host synchronisation, staging or stream queries: six
 * launches on `stream` (four when op_cap == 0), their grids
 * sized by rec_cap and op_cap; threads beyond the device-resident counts do
 * nothing.  A key or value is copied by one group of lanes however long it is
 * (as in lv_sst_build_device): a single very long value is the call's serial
 * worst case. */
#define LV_WB_ENCODE_UPSTREAM    1u
#define LV_WB_ENCODE_REC_OVER    2u
#define LV_WB_ENCODE_BAD_BOUNDS  4u
#define LV_WB_ENCODE_BAD_OP      8u
#define LV_WB_ENCODE_OUT_OVER   16u

typedef struct lv_wb_encode_totals {   /* device memory, 8-B aligned, always written */
    uint64_t records, ops, key_bytes, value_bytes, out_bytes, last_sequence, status, bad_record, bad_op;
} lv_wb_encode_totals;

typedef struct lv_wb_encode_out {      /* device memory the caller owns */
    uint8_t *d_out;  size_t out_cap;   /* any byte alignment */
    uint64_t *d_rec_off, *d_rec_len;   /* rec_cap each: exactly what lv_write_batch_decode_device takes */
    lv_wb_op *d_ops_out;               /* op_cap, 16-B aligned; may be NULL */
    lv_wb_encode_totals *d_totals;
} lv_wb_encode_out;

size_t lv_write_batch_encode_workspace_bytes(size_t rec_cap, size_t op_cap);
int lv_write_batch_encode_device(const uint8_t *d_src, size_t src_bytes,
                                 const lv_wb_op *d_ops, size_t op_cap,
                                 const uint64_t *d_rec_op, const uint64_t *d_records,
                                 const uint64_t *d_upstream_status, size_t rec_cap,
                                 uint64_t first_sequence, const lv_wb_encode_out *out,
                                 uint32_t flags, void *d_workspace, size_t workspace_bytes, void *stream);

/* The same on the host, serially (no GPU): the arrays are host memory and
 * `records` is the caller's own count (rec_off / rec_len hold that many
 * entries), so UPSTREAM and REC_OVER do not arise; the other bits are judged
 * as above and 0 is returned with the status in *totals; LV_ERR_INVALID
 * for a NULL totals, rec_op, src with src_bytes (but see sizing), ops with op_cap, rec_off /
 * rec_len with records, out with out_cap, records > 2^32 - 2 or op_cap > 2^30.
 * ops_out may be NULL.
 * Sizing mode, out == NULL and out_cap == 0: rec_off, rec_len, ops_out and the
 * totals are written as if the capacity sufficed, OUT_OVER is not raised, and
 * src is only bounds-checked, never read (it may be NULL) -- the host arrays
 * lv_wal_encode_device wants, without a round trip. */
int lv_write_batch_encode_host(const uint8_t *src, size_t src_bytes, const lv_wb_op *ops, size_t op_cap,
                               const uint64_t *rec_op, size_t records, uint64_t first_sequence,
                               uint8_t *out, size_t out_cap, uint64_t *rec_off, uint64_t *rec_len,
                               lv_wb_op *ops_out, lv_wb_encode_totals *totals);

#ifdef __cplusplus
}
#endif

#endif /* LVGPU_WRITE_BATCH_H */
