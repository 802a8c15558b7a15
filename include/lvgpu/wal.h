/*
 * lvgpu WAL — batched write-ahead-log encode / verify on MI355X, the callers
 * of the CRC path.  C ABI.
 *
 * Reader side (log_reader.rs): a whole log is scanned on the GPU — every
 * 32 KiB block's physical-record header chain is walked (the framing of
 * read_physical_record, log_reader.rs:271-331) and every [type || payload]
 * CRC unit is checksummed in one batch (log_reader.rs:335-336).  A host
 * reader then replays the reference Reader state machine (fragments, drops,
 * reports, initial offset; log_reader.rs:44-393) taking each record's CRC from
 * the scan instead of computing it.
 *
 * Writer side (log_writer.rs): many logical records are laid out exactly as
 * Writer::add_record does (log_writer.rs:62-110) and every fragment header's
 * masked CRC (log_writer.rs:123-125) comes from one GPU batch.  From host
 * memory (lv_wal_encode_host) the bytes are laid out by host threads; with the
 * payload already in HBM (lv_wal_encode_device) the log is written there too,
 * by a kernel that produces it in aligned 16-byte stores.
 */
#ifndef LVGPU_WAL_H
#define LVGPU_WAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* log_format.rs:22-29, 62-66 */
#define LV_WAL_BLOCK_SIZE 32768u
#define LV_WAL_HEADER_SIZE 7u

/* Physical-record status in lv_wal_scan info (bits 8..15) */
#define LV_WAL_REC_OK 0u          /* header fits its block: CRC computed       */
#define LV_WAL_REC_BAD_LENGTH 1u  /* HEADER_SIZE + length > bytes left in block */
#define LV_WAL_REC_ZERO 2u        /* type ZERO with length 0 (reader skips)      */

typedef struct lv_wal_scan lv_wal_scan;

/* Scan a host-memory log on `device`: copies it in, frames every block on
 * the GPU, CRCs every record and copies the results back.  Returns NULL on
 * error (lv_last_error()).  Records are in log order. */
lv_wal_scan *lv_wal_scan_host(const uint8_t *log, size_t bytes, int device);
/* The same scan, pipelined against its reader: returns at once, while a
 * worker thread scans the log in 32 MiB block-aligned chunks (upload, device
 * scan, results back).  A reader over this scan (lv_wal_reader_new) waits only
 * for the chunk holding the next header it reaches, so replaying chunk k
 * overlaps the scan of chunk k + 1; the accessors below wait for the whole
 * scan.  `log` must stay valid until lv_wal_scan_free.  NULL on an argument
 * error; a scan error surfaces from the reader (< 0) or lv_wal_scan_wait. */
lv_wal_scan *lv_wal_scan_host_pipelined(const uint8_t *log, size_t bytes, int device);
/* Waits for a pipelined scan to finish: 0, or its error (lv_last_error).
 * Immediate for any other scan.  Memory: a pipelined scan keeps its per-chunk
 * arrays (readers over it point into them) and, once this or an accessor below
 * is called, also the flat arrays -- about 16 B per record twice (a 1 GiB log
 * of 178 K records: ~5.7 MB).  A caller that only reads records through
 * lv_wal_reader never pays the second copy. */
int lv_wal_scan_wait(lv_wal_scan *scan);
/* Device-resident scan of a log already in HBM (8-byte aligned), with no
 * host synchronisation: every 32 KiB block's header chain is walked as
 * read_physical_record frames it and every [type || payload] unit is
 * checksummed, in five launches on `stream` (framing, one global length sort,
 * the CRC kernel, the log-order write-back).  Records go to d_hdr_off / d_crc /
 * d_info in log order (the lv_wal_scan arrays below), at most `cap` of them;
 * *d_count (device memory) receives the number of records.  If that number
 * exceeds cap, nothing else is written: call again with a larger capacity.
 * d_workspace: >= lv_wal_scan_workspace_bytes(bytes, cap) bytes, 16-B aligned. */
size_t lv_wal_scan_workspace_bytes(size_t bytes, size_t cap);
int lv_wal_scan_device(const uint8_t *d_log, size_t bytes, uint64_t *d_hdr_off, uint32_t *d_crc, uint32_t *d_info,
                       size_t cap, uint64_t *d_count, void *d_workspace, size_t workspace_bytes, void *stream);
/* Number of physical records reached by the blocks' header chains (a
 * pipelined scan: waits for it; 0 if it failed). */
size_t lv_wal_scan_count(const lv_wal_scan *scan);
/* Header offsets (ascending), value([type||payload]) (0 unless status OK),
 * and info = type | status << 8 | payload_length << 16. */
const uint64_t *lv_wal_scan_offsets(const lv_wal_scan *scan);
const uint32_t *lv_wal_scan_crcs(const lv_wal_scan *scan);
const uint32_t *lv_wal_scan_info(const lv_wal_scan *scan);
/* Build a scan from caller arrays (copied): tests / externally computed CRCs. */
lv_wal_scan *lv_wal_scan_from_arrays(const uint64_t *offsets, const uint32_t *crcs, const uint32_t *info,
                                     size_t n);
void lv_wal_scan_free(lv_wal_scan *scan);

/* Reporter: Reporter::corruption(bytes, reason) (log_reader.rs:37-42). */
typedef void (*lv_wal_reporter_fn)(void *ctx, size_t bytes, const char *reason);

typedef struct lv_wal_reader lv_wal_reader;

/* Reader::new(file, reporter, checksum, initial_offset) (log_reader.rs:75-94)
 * over an in-memory log and its scan (both must outlive the reader).
 * `reporter` may be NULL. */
lv_wal_reader *lv_wal_reader_new(const uint8_t *log, size_t bytes, const lv_wal_scan *scan,
                                 lv_wal_reporter_fn reporter, void *ctx, int checksum,
                                 uint64_t initial_offset);
/* Reader::read_record (log_reader.rs:120-265): 1 and (*data, *len) = the next
 * record (valid until the next call), 0 at end of input, < 0 on error (a
 * header the scan does not cover). */
int lv_wal_reader_read_record(lv_wal_reader *reader, const uint8_t **data, size_t *len);
/* Reader::last_record_offset (log_reader.rs:99). */
uint64_t lv_wal_reader_last_record_offset(const lv_wal_reader *reader);
void lv_wal_reader_free(lv_wal_reader *reader);

/* Writer::add_record for n logical records at once (log_writer.rs:62-134):
 * record i is payload[rec_off[i] .. rec_off[i] + rec_len[i]).  dest_length is
 * the existing log length (Writer::new_with_dest_length, log_writer.rs:48-56).
 * Writes the appended bytes to out (capacity out_cap) and their count to
 * *out_len; header CRCs are one GPU batch on `device`.  If out is NULL or too
 * small, only *out_len is set and LV_ERR_INVALID is returned. */
int lv_wal_encode_host(const uint8_t *payload, const uint64_t *rec_off, const uint64_t *rec_len, size_t n,
                       uint64_t dest_length, uint8_t *out, size_t out_cap, size_t *out_len, int device);

/* Host, pure, no GPU: the number of bytes Writer::add_record appends for n
 * records of these lengths to a log whose Writer has already written
 * dest_length bytes (log_writer.rs:48-56; only dest_length % 32768 matters).
 * *fragments (may be NULL) = physical records emitted. */
size_t lv_wal_encode_size(const uint64_t *rec_len, size_t n, uint64_t dest_length, size_t *fragments);

/* Device workspace of lv_wal_encode_device for a batch of `fragments` physical
 * records: the fragment table and its CRCs (32 bytes per fragment) plus
 * lv_crc32c_workspace_bytes(fragments). */
size_t lv_wal_encode_workspace_bytes(size_t fragments);

/* lv_wal_encode_host with the payload and the output in device memory.
 * rec_off / rec_len are HOST arrays (the group-commit writer knows its
 * records' lengths on the host, as lv_batch_hint already assumes); record i is
 * d_payload[rec_off[i] .. rec_off[i]+rec_len[i]).  Records may overlap, repeat
 * or be in any order within d_payload[0, payload_bytes).  Writes exactly
 * d_out[0, *out_len) and no other byte; *out_len is always set; if d_out is
 * NULL or out_cap is too small, LV_ERR_INVALID and nothing is enqueued (a
 * batch that appends no bytes -- n == 0 -- is LV_OK with nothing enqueued).
 * Stream-ordered and asynchronous; the host arrays are consumed before return.
 *
 * d_payload and d_out may have any byte alignment; d_out[0, *out_len) must not
 * overlap d_payload[0, payload_bytes).  d_workspace: at least
 * lv_wal_encode_workspace_bytes(fragments) bytes, 16-B aligned, not shared
 * with a call that may run concurrently.  Every argument is checked on the
 * host before any device call (LV_ERR_INVALID, lv_last_error).
 *
 * Limit: a batch may emit at most 2^32-1 fragments, what one
 * lv_crc32c_batch_device call accepts; more is LV_ERR_INVALID.
 *
 * Two steps on `stream`, no host synchronisation: the fragment table goes up
 * through page-locked staging the library owns (a staging buffer is reused
 * only after the copy that read it has completed, so calls enqueued back to
 * back, on one stream or several, never share one) and the offsets API
 * checksums every fragment where it lies in d_payload; then wal_frame_kernel
 * writes the log, every 16-byte granule of d_out with one aligned store.  The
 * call asks the runtime whether earlier copies have finished, which a stream
 * capture does not allow: do not capture it into a HIP graph. */
int lv_wal_encode_device(const uint8_t *d_payload, uint64_t payload_bytes, const uint64_t *rec_off,
                         const uint64_t *rec_len, size_t n, uint64_t dest_length, uint8_t *d_out, size_t out_cap,
                         size_t *out_len, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- Device-resident Reader: the inverse of lv_wal_encode_device ----------
 *
 * lv_wal_decode_device replays Reader::read_record (log_reader.rs:120-364, as
 * lv_wal_reader restates it) over a log in HBM and the arrays
 * lv_wal_scan_device made of the same d_log and bytes: stored checksums are
 * compared with the computed ones, FIRST/MIDDLE/LAST fragments are joined into
 * logical records, and the Reader's drop rules are applied and reported.
 * Scope: Reader::new(.., initial_offset = 0).  An initial offset and the
 * resyncing it brings are not offered; use lv_wal_reader for those.
 * As in lv_wal_reader and the reference, a well-formed physical record whose
 * type byte is 5 or 6 reads as the Reader's own Eof / BadRecord code: type 5
 * ends the replay there, silently (nothing after it is read or reported), and
 * type 6 drops an open record ("error in middle of record") and reading goes
 * on; types >= 7 are "unknown record type".
 *
 * Output (all device memory the caller owns): record r is
 * d_payload[d_rec_off[r], d_rec_off[r] + d_rec_len[r]) -- the records lie end
 * to end in log order, d_rec_off[0] = 0 -- and d_rec_log_off[r] is what
 * Reader::last_record_offset returns after reading it (the header offset of
 * its FULL or FIRST fragment).  Report q is what Reporter::corruption received
 * q-th: d_rep_bytes[q] bytes for d_rep_reason[q] (LV_WAL_DROP_*), and
 * d_rep_log_off[q] is the header offset of the physical record at which the
 * Reader made it.  *d_totals is always written: the numbers of records,
 * payload bytes and reports, the sum of the reports' byte counts, and status.
 *
 * Capacities.  rec_cap = scan_cap, rep_cap = 2 * scan_cap and payload_cap =
 * bytes always suffice, so everything can be sized without a round trip:
 * every record ends at a scan entry of its own (its FULL or LAST), an entry
 * makes at most two reports (a kill inside an open record: the kill, then
 * "error in middle of record"), and every payload byte is a log byte.  If a
 * capacity is exceeded, or the scan itself overflowed (*d_count > scan_cap:
 * it wrote no entries, and the totals are those of an empty log), only
 * *d_totals is written, with the true totals and the LV_WAL_DECODE_*_OVER
 * bits; otherwise status == 0.  d_rep_bytes / d_rep_log_off / d_rep_reason
 * may all be NULL with rep_cap == 0: reports are then only counted and
 * REPORT_OVER is not raised.
 *
 * Arguments.  d_hdr_off / d_crc / d_info / d_count are exactly what
 * lv_wal_scan_device wrote for d_log[0, bytes) at capacity scan_cap (read in
 * stream order; *d_count is read on the device, never on the host).  d_log is
 * 8-B aligned, d_payload may have any byte alignment, and
 * d_payload[0, payload_cap) must not overlap d_log[0, bytes).  d_workspace:
 * >= lv_wal_decode_workspace_bytes(scan_cap) bytes, 16-B aligned, not shared
 * with a call that may run concurrently.  Every argument is checked on the
 * host before any device call (LV_ERR_INVALID, lv_last_error).
 *
 * Stream-ordered, no host synchronisation: six launches on
 * `stream`, sized by scan_cap (threads beyond *d_count do nothing).  Unlike
 * lv_wal_encode_device the call stages nothing and asks the runtime nothing
 * about the stream's progress, so it may be captured into a HIP graph, once
 * the device has been initialised (lv_device_init or any earlier call). */
#define LV_WAL_DECODE_NO_CHECKSUM 0x1u   /* Reader::new(checksum = false): d_crc may be NULL */

/* reasons, one per string lv_wal_reader reports with initial_offset == 0 */
#define LV_WAL_DROP_BAD_LENGTH 1u        /* "bad record length" */
#define LV_WAL_DROP_CHECKSUM 2u          /* "checksum mismatch" */
#define LV_WAL_DROP_MID_RECORD 3u        /* "error in middle of record" */
#define LV_WAL_DROP_NO_END_1 4u          /* "partial record without end(1)" */
#define LV_WAL_DROP_NO_END_2 5u          /* "partial record without end(2)" */
#define LV_WAL_DROP_NO_START_1 6u        /* "missing start of fragmented record(1)" */
#define LV_WAL_DROP_NO_START_2 7u        /* "missing start of fragmented record(2)" */
#define LV_WAL_DROP_UNEXPECTED_TYPE 8u   /* "unexpected record type" */
#define LV_WAL_DROP_UNKNOWN_TYPE 9u      /* "unknown record type" */

/* status bits in lv_wal_decode_totals.status */
#define LV_WAL_DECODE_SCAN_OVER 1u       /* *d_count > scan_cap: the scan itself wrote nothing */
#define LV_WAL_DECODE_REC_OVER 2u
#define LV_WAL_DECODE_PAYLOAD_OVER 4u
#define LV_WAL_DECODE_REPORT_OVER 8u

typedef struct lv_wal_decode_totals {   /* device memory, 8-B aligned, always written */
    uint64_t records, payload_bytes, reports, dropped_bytes, status;
} lv_wal_decode_totals;

typedef struct lv_wal_decode_out {      /* every pointer is device memory the caller owns */
    uint8_t *d_payload;   size_t payload_cap;   /* any byte alignment */
    uint64_t *d_rec_off, *d_rec_len, *d_rec_log_off;  size_t rec_cap;
    uint64_t *d_rep_bytes, *d_rep_log_off;  uint32_t *d_rep_reason;  size_t rep_cap;
    lv_wal_decode_totals *d_totals;
} lv_wal_decode_out;

size_t lv_wal_decode_workspace_bytes(size_t scan_cap);
int lv_wal_decode_device(const uint8_t *d_log, size_t bytes,
                         const uint64_t *d_hdr_off, const uint32_t *d_crc, const uint32_t *d_info,
                         const uint64_t *d_count, size_t scan_cap,
                         const lv_wal_decode_out *out, uint32_t flags,
                         void *d_workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LVGPU_WAL_H */
