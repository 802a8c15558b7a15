/*
 * lvgpu VersionEdit -- the record of the MANIFEST.  C ABI.
 *
 * A compaction leaves its output in HBM as a run of tables with their
 * lv_version_file records (lv_compact_output_device, compact.h), and
 * lv_version_open_device / lv_version_get_device read such a version
 * (version.h).  What writes down that the version changed is a VersionEdit
 * (src/version_edit.rs), one logical record of the MANIFEST, which is a log in
 * the WAL format: lv_wal_encode_device / lv_wal_scan_device /
 * lv_wal_decode_device (wal.h) carry it as they carry a WriteBatch.
 *
 *   record := field*
 *   field  := 01 varstring                      comparator name
 *           | 02 varint64                       log number
 *           | 09 varint64                       previous log number
 *           | 03 varint64                       next file number
 *           | 04 varint64                       last sequence
 *           | 05 level varstring                compact pointer (internal key)
 *           | 06 level varint64                 deleted file (level, number)
 *           | 07 level varint64 varint64 varstring varstring
 *                                               new file (level, number, file
 *                                               size, smallest, largest)
 *   level  := varint32;  varstring := len: varint32, data: u8[len]
 *
 * Parity.  Unlike the stages around it this one is in the reference:
 * encode_to (version_edit.rs:192-234) and decode_from (:236-319) over the
 * coding.rs the WriteBatch stages already restate.  Both directions are pinned
 * by it: the worked example below and the reference's own test (:391-417,
 * tests/golden/version_edit_example.json), an independent serial Python model
 * written from the two Rust files (tests/version_edit_cases.py), and the host
 * twins below.  last_has of the decode totals is the project's own definition
 * (what upstream's VersionSet::Recover keeps); the reference has no VersionSet.
 *
 * Applying edits to a version (VersionSet::Builder, Recover), and with it
 * turning decoded rows into lv_version_file records (the image placements the
 * manifest does not hold come in as a directory), is lv_version_apply_device,
 * version_set.h.  Out of scope: the CURRENT file; compaction picking;
 * allowed_seeks; the comparator-name check.
 *
 * ---- Data ---------------------------------------------------------------------
 *
 * Offsets are u64 into one byte buffer at any alignment: d_payload on decode,
 * d_src on encode.  The row tables are 16-byte aligned.  Record r's rows are
 * d_files[d_rec_file[r] .. d_rec_file[r + 1]), and the same for d_rec_deleted
 * and d_rec_pointer: each bounds array has rec_cap + 1 entries (the d_rec_op
 * idiom of write_batch.h).
 */
#ifndef LVGPU_VERSION_EDIT_H
#define LVGPU_VERSION_EDIT_H

#include <stddef.h>
#include <stdint.h>

#include "table.h"
#include "version.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LV_VE_NUM_LEVELS 7u            /* config.rs:18 */

/* per-record status: what VersionEdit::decode_from returned for this record */
#define LV_VE_OK 0u
#define LV_VE_UNKNOWN_TAG 1u    /* "unknown tag": the tag's low byte is none of 1-7, 9 */
#define LV_VE_INVALID_TAG 2u    /* "invalid tag": a tag varint failed with input left */
#define LV_VE_BAD_VARINT32 3u   /* "Error when decoding varint-32" */
#define LV_VE_BAD_VARINT64 4u   /* "Input doesn't contain a valid varint-64." */
#define LV_VE_BAD_LENGTH 5u     /* "Input slice doesn't contain a length-prefixed encoded value." */
#define LV_VE_BAD_LEVEL 6u      /* "exceeded max level" */
#define LV_VE_OUT_OF_RANGE 7u   /* device only: record extent outside d_payload[0, payload_bytes); not read */

#define LV_VE_HAS_COMPARATOR 1u
#define LV_VE_HAS_LOG_NUMBER 2u
#define LV_VE_HAS_PREV_LOG_NUMBER 4u
#define LV_VE_HAS_NEXT_FILE 8u
#define LV_VE_HAS_LAST_SEQUENCE 16u
#define LV_VE_HAS_ALL 31u

#define LV_VE_FLAG_NEG_LEVEL 1u  /* some row's level is >= 2^31: negative as the reference's i32 */
#define LV_VE_FLAG_SHORT_KEY 2u  /* some pointer / smallest / largest key is under 8 bytes: no internal key */

typedef struct lv_ve_edit {     /* 64 B, one per record */
    uint64_t log_number, prev_log_number, next_file_number, last_sequence, comparator_off;
    uint32_t comparator_len, has;    /* has: LV_VE_HAS_* */
    uint32_t status, flags;          /* decode writes both (LV_VE_*, LV_VE_FLAG_*); encode ignores both */
    uint64_t reserved;               /* written 0 */
} lv_ve_edit;
typedef struct lv_ve_file {     /* 48 B: NewFile */
    uint64_t number, file_size, smallest_off, largest_off;
    uint32_t smallest_len, largest_len, level, reserved;
} lv_ve_file;
typedef struct lv_ve_deleted { uint64_t number;  uint32_t level, reserved; } lv_ve_deleted;  /* 16 B */
typedef struct lv_ve_pointer { uint64_t key_off; uint32_t key_len, level;  } lv_ve_pointer;  /* 16 B */

/* ---- Decode: one record on the host ---------------------------------------------
 *
 * VersionEdit::decode_from (version_edit.rs:236-319) on a fresh
 * VersionEdit::new(), over rec[0, n).  Host, pure, no GPU.
 *
 *   The loop reads a tag, a varint32, of which only the low 8 bits are looked
 *   at (`tag_num.unwrap() as u8`, :251): the bytes 81 02 (257) are tag 1.  Low
 *   bytes 1, 2, 3, 4, 5, 6, 7 and 9 are fields; any other value is
 *   LV_VE_UNKNOWN_TAG, whatever input remains.
 *   A tag varint that fails to decode ends the loop: with no input left the
 *   record is LV_VE_OK (the empty record is OK with nothing set), otherwise
 *   LV_VE_INVALID_TAG.
 *   A failing field returns coding.rs's own error at once: BAD_VARINT32 (the
 *   varint32 write_batch.h describes: five bytes at most, the fifth byte's bits
 *   above bit 31 are dropped); BAD_VARINT64 (coding.rs:223-241: ten bytes at
 *   most, the tenth byte's bits above bit 63 are dropped; a tenth byte with the
 *   continuation bit set, or input that ends inside the varint, is the error);
 *   BAD_LENGTH (a body longer than the remaining input); BAD_LEVEL.
 *   get_level (:361-369) compares as i32, so a level of 2^31 or more passes:
 *   the row carries the 32 bits and the record's flags get
 *   LV_VE_FLAG_NEG_LEVEL.  Levels 7 to 2^31 - 1 are BAD_LEVEL.
 *   Keys of any length pass, the empty key included (InternalKey::from copies).
 *   A record with a pointer, smallest or largest key under 8 bytes gets
 *   LV_VE_FLAG_SHORT_KEY: user_key() would assert on it, so a consumer can
 *   refuse.
 *   A repeated scalar tag overwrites the earlier value.  Rows are emitted in
 *   the order met; deleted files are neither sorted nor deduplicated (the
 *   reference's BTreeSet does that, and it is the encoder's side).
 *   A record with a status other than OK emits no rows, and its lv_ve_edit is
 *   all zero except status: the reference returns Err, and what it leaves in
 *   the object is not a result.
 *   clear() (:131-141), which decode_from calls first, does not reset
 *   has_log_number or the three collections; that matters only for a reused
 *   object and has no effect here, where every record starts from
 *   VersionEdit::new().
 *
 * Returns LV_VE_* and writes *edit (may be NULL).  counts[0..3) = the file,
 * deleted and pointer rows found (0 when the status is not OK); min(count,
 * cap) of each are written, and a table may be NULL with its cap 0 to count.
 * counts may be NULL.  Offsets are into rec. */
uint32_t lv_version_edit_decode_host(const uint8_t *rec, size_t n, lv_ve_edit *edit,
                                     lv_ve_file *files, size_t file_cap,
                                     lv_ve_deleted *deleted, size_t deleted_cap,
                                     lv_ve_pointer *pointers, size_t pointer_cap, size_t *counts);

/* ---- Decode: the records of lv_wal_decode_device in HBM ---------------------------
 *
 * Inputs: exactly lv_write_batch_decode_device's.  Record r is
 * d_payload[d_rec_off[r], d_rec_off[r] + d_rec_len[r]), r < *d_records;
 * d_records and the optional d_upstream_status are read on the device in
 * stream order.  Records lie at any byte, in any order, and may overlap.  A
 * record whose extent lies outside [0, payload_bytes) (u64 arithmetic that
 * cannot wrap) gets LV_VE_OUT_OF_RANGE, and no byte of it is read.
 *
 * Semantics per record: lv_version_edit_decode_host's, bit for bit, with
 * offsets into d_payload.
 *
 * Outputs.  d_edits[r], r < records; the three row tables in record order,
 * then the order met, with their bounds (records + 1 entries each).
 * *d_totals is always written: records = *d_records; files, deleted and
 * pointers = the rows emitted; bad_records = the records whose status is not
 * OK; first_bad = the lowest such record, or records if there is none;
 * last_has[b], one per has bit (COMPARATOR first) = 1 + the index of the last
 * record below first_bad that carries the bit, 0 for none (the seek_file idiom
 * of version.h): the value of that record is the one a recovery keeps;
 * status = LV_VE_DECODE_* bits.
 *
 * With any status bit set, only *d_totals is written:
 *   UPSTREAM      *d_upstream_status != 0: the totals of zero records.
 *   REC_OVER      *d_records > rec_cap: records = *d_records, every other
 *                 total is 0.
 *   FILE_OVER, DELETED_OVER, POINTER_OVER   more rows than the capacity: all
 *                 totals are the true ones.
 * Capacities that always suffice follow from the smallest encodings: a NewFile
 * is at least 6 bytes (tag, level, two numbers, two empty keys), so file_cap =
 * payload_bytes / 6; a DeletedFile or CompactPointer is at least 3 bytes, so
 * deleted_cap = pointer_cap = payload_bytes / 3 -- when records do not overlap.
 *
 * Arguments, checked on the host before any device call (LV_ERR_INVALID,
 * lv_last_error): out, d_totals, d_records and the three bounds arrays are
 * never NULL; d_payload only with payload_bytes == 0, a row table only with
 * its cap == 0, d_rec_off / d_rec_len / d_edits only with rec_cap == 0; the row
 * tables and d_edits 16-byte aligned, d_totals and the bounds 8-byte aligned;
 * d_workspace 16-byte aligned and >=
 * lv_version_edit_decode_workspace_bytes(rec_cap) bytes; flags == 0; rec_cap
 * <= 2^32 - 2; every row cap <= 2^56; no row table may overlap d_payload.
 * Without a usable GPU a well-formed call fails with the runtime's error:
 * there is no host fallback.
 *
 * Reads.  Of a record only the field headers are read: comparator and key
 * bodies are skipped, never read.  Apart from the records' own bytes the
 * kernels read only the aligned 16-byte granules that hold a byte of a record.
 *
 * Stream-ordered, no host synchronisation, no memset: four launches on
 * `stream` (one thread that zeroes the call's head; a count walk; one wave
 * that scans the tiles' three row counts and writes the totals; an emit walk),
 * sized by rec_cap, one workgroup per tile of 256 records.  Capturable into a
 * HIP graph once the device is initialised.
 * A record of up to 16 KiB is walked by one lane, a longer one by one wave
 * through an LDS window.  The format is a varint chain, so one record is
 * walked serially: a snapshot edit (upstream's WriteSnapshot: every file of
 * the version in one record) is the call's serial worst case, and a host
 * decode of that one record is the faster route (README, "VersionEdit"). */
#define LV_VE_DECODE_UPSTREAM      1u
#define LV_VE_DECODE_REC_OVER      2u
#define LV_VE_DECODE_FILE_OVER     4u
#define LV_VE_DECODE_DELETED_OVER  8u
#define LV_VE_DECODE_POINTER_OVER 16u

typedef struct lv_ve_totals {     /* device memory, 8-B aligned, always written */
    uint64_t records, files, deleted, pointers, bad_records, first_bad, last_has[5], status;
} lv_ve_totals;

typedef struct lv_ve_decode_out { /* device memory the caller owns */
    lv_ve_edit *d_edits;                                                  /* rec_cap, 16-B aligned */
    lv_ve_file *d_files;        size_t file_cap;     uint64_t *d_rec_file;     /* rec_cap + 1 bounds */
    lv_ve_deleted *d_deleted;   size_t deleted_cap;  uint64_t *d_rec_deleted;
    lv_ve_pointer *d_pointers;  size_t pointer_cap;  uint64_t *d_rec_pointer;
    lv_ve_totals *d_totals;
} lv_ve_decode_out;

size_t lv_version_edit_decode_workspace_bytes(size_t rec_cap);
int lv_version_edit_decode_device(const uint8_t *d_payload, size_t payload_bytes,
                                  const uint64_t *d_rec_off, const uint64_t *d_rec_len,
                                  const uint64_t *d_records, const uint64_t *d_upstream_status,
                                  size_t rec_cap, const lv_ve_decode_out *out, uint32_t flags,
                                  void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- Encode: a batch of edits to records, all or nothing ---------------------------
 *
 * The inverse.  The decode's outputs feed in as they are (status, flags and
 * reserved fields are ignored); offsets are into d_src[0, src_bytes).  Only
 * rows inside [bounds[0], bounds[*d_records]) are read: leading and trailing
 * rows of a table are never looked at.
 *
 * Record r's bytes are encode_to's (version_edit.rs:192-234), in this order:
 * tag 1 and the length-prefixed comparator, tag 2 log number, tag 9 previous
 * log number, tag 3 next file number, tag 4 last sequence -- each only if its
 * has bit is set --, then every pointer `05 level key`, every deleted file
 * `06 level number`, every new file `07 level number file_size smallest
 * largest`.  Levels are varint32, numbers varint64, keys a varint32 length and
 * the bytes.
 *
 * Outputs, when status == 0: d_out[0, out_bytes), the records end to end;
 * d_rec_off[r] / d_rec_len[r], the arrays the WAL and decode stages take.
 * *d_totals is always written: records, files, deleted, pointers (the rows of
 * the records), key_bytes (the comparator and key bytes copied from d_src),
 * out_bytes, status, and bad_record / bad_kind / bad_row = 2^64 - 1 unless a
 * bit below sets them.
 *
 * The status bits are judged in this order and the first one raised ends the
 * judging; with a bit set only *d_totals is written:
 *   UPSTREAM    *d_upstream_status != 0: the totals of zero records.
 *   REC_OVER    *d_records > rec_cap: records = *d_records, the sums 0.
 *   BAD_BOUNDS  not (b[r] <= b[r + 1] <= cap) for a bounds array b: bad_record
 *               = the lowest such r, bad_kind = the lowest kind that fails on
 *               it, records = *d_records, the sums 0.  No row is read.
 *   BAD_ROW     an edit with undefined has bits or, with HAS_COMPARATOR, a
 *               comparator extent outside d_src; a row with a level of 7 or
 *               more or a key extent outside d_src; a deleted row that is not
 *               strictly above its predecessor in the record by (level,
 *               number) -- the reference's BTreeSet iterates in that order and
 *               holds no duplicate, so requiring it of the caller keeps the
 *               output equal to encode_to's.  bad_kind = the lowest kind with
 *               such an item (EDIT, POINTER, DELETED, FILE: the order of the
 *               bytes), bad_row = the lowest such index into that kind's table
 *               (for EDIT the record index), bad_record = its record; records
 *               = *d_records, the sums 0.  No byte of d_src is read before
 *               every row is accepted.
 *   OUT_OVER    out_bytes > out_cap: every total is the true one, so one retry
 *               suffices.  50 records + 7 pointers + 12 deleted + 32 files +
 *               key_bytes always suffices (a tag and a level of one byte each,
 *               varint64s of ten bytes, varint32 lengths of five).
 *
 * Arguments, checked on the host before any device call: in, out, d_totals,
 * d_records and the three bounds arrays are never NULL; d_src only with
 * src_bytes == 0, a row table only with its cap == 0, d_out only with out_cap
 * == 0, d_edits / d_rec_off / d_rec_len only with rec_cap == 0; tables 16-byte
 * aligned, d_totals, bounds, d_rec_off and d_rec_len 8-byte aligned;
 * d_workspace 16-byte aligned and >= lv_version_edit_encode_workspace_bytes
 * (rec_cap, file_cap, deleted_cap, pointer_cap); flags == 0; rec_cap <= 2^32 -
 * 2, every row cap <= 2^30 (so no sum of sizes leaves u64); d_out must not
 * overlap d_src or a table.
 *
 * Stream-ordered, no host synchronisation, no memset: five launches (one
 * thread that zeroes the call's head, validate, size with a tile scan, carry,
 * emit); capturable.  An item is a record's
 * scalar group or one row, one per lane; the item order is the four tables one
 * after another (edits, pointers, deleted, files), each with cap + 1 slots
 * rounded up to whole tiles of 1024.  Keys are copied by groups of lanes
 * however long they are.
 *
 * lv_wal_encode_device takes host rec_off / rec_len: that is wal.h's rule and
 * stays.  A device chain copies records x 8 bytes of d_rec_len back, or sizes
 * on the host with lv_version_edit_encode_host's sizing mode. */
#define LV_VE_ENCODE_UPSTREAM    1u
#define LV_VE_ENCODE_REC_OVER    2u
#define LV_VE_ENCODE_BAD_BOUNDS  4u
#define LV_VE_ENCODE_BAD_ROW     8u
#define LV_VE_ENCODE_OUT_OVER   16u

#define LV_VE_KIND_EDIT 0u
#define LV_VE_KIND_POINTER 1u
#define LV_VE_KIND_DELETED 2u
#define LV_VE_KIND_FILE 3u

typedef struct lv_ve_encode_totals {   /* device memory, 8-B aligned, always written */
    uint64_t records, files, deleted, pointers, key_bytes, out_bytes, status, bad_record, bad_kind, bad_row;
} lv_ve_encode_totals;

typedef struct lv_ve_encode_in {       /* the decode's outputs, or the same made by hand */
    const lv_ve_edit *d_edits;                                                       /* rec_cap */
    const lv_ve_file *d_files;        size_t file_cap;     const uint64_t *d_rec_file;    /* rec_cap + 1 */
    const lv_ve_deleted *d_deleted;   size_t deleted_cap;  const uint64_t *d_rec_deleted;
    const lv_ve_pointer *d_pointers;  size_t pointer_cap;  const uint64_t *d_rec_pointer;
} lv_ve_encode_in;

typedef struct lv_ve_encode_out {
    uint8_t *d_out;  size_t out_cap;   /* any byte alignment */
    uint64_t *d_rec_off, *d_rec_len;   /* rec_cap each */
    lv_ve_encode_totals *d_totals;
} lv_ve_encode_out;

size_t lv_version_edit_encode_workspace_bytes(size_t rec_cap, size_t file_cap, size_t deleted_cap, size_t pointer_cap);
int lv_version_edit_encode_device(const uint8_t *d_src, size_t src_bytes, const lv_ve_encode_in *in,
                                  const uint64_t *d_records, const uint64_t *d_upstream_status,
                                  size_t rec_cap, const lv_ve_encode_out *out, uint32_t flags,
                                  void *d_workspace, size_t workspace_bytes, void *stream);

/* The same on the host, serially (no GPU): the arrays are host memory (the
 * same lv_ve_encode_in / lv_ve_encode_out structs, their pointers host
 * pointers) and `records` is the caller's own count, so UPSTREAM and REC_OVER
 * do not arise; the other bits are judged as above and 0 is returned with the
 * status in *out->d_totals; LV_ERR_INVALID for what the device call refuses
 * (alignment and overlap are not checked).
 * Sizing mode, out->d_out == NULL and out->out_cap == 0: d_rec_off, d_rec_len
 * and the totals are written as if the capacity sufficed, OUT_OVER is not
 * raised, and src is only bounds-checked, never read (it may be NULL). */
int lv_version_edit_encode_host(const uint8_t *src, size_t src_bytes, const lv_ve_encode_in *in,
                                size_t records, const lv_ve_encode_out *out);

/* ---- The link from a compaction ----------------------------------------------------
 *
 * lv_compact_output_device's d_version_files and d_tables to NewFile rows, one
 * lane per file.  *d_file_count (e.g. &d_totals->files of that call) is read
 * on the device.  Row i < min(*d_file_count, files_cap): level and number are
 * the file's, file_size = d_tables[i].file_bytes, and the bound extents are
 * copied as they are, so that call's d_bound_keys is the encode's d_src.
 * d_rec_file, unless NULL, gets the bounds {0, min(*d_file_count, files_cap)}
 * of one record.  *d_status (u64, 8-byte aligned, always written) = the files
 * whose status != 0 or whose table's status != 0, plus the files beyond
 * files_cap; it is the encode's d_upstream_status.  Two launches on `stream`,
 * no memset; LV_ERR_INVALID for a NULL or misaligned argument. */
int lv_version_edit_files_device(const lv_version_file *d_version_files, const lv_sst_table *d_tables,
                                 const uint64_t *d_file_count, size_t files_cap, lv_ve_file *d_files,
                                 uint64_t *d_rec_file, uint64_t *d_status, void *stream);

/* Worked example (tests/golden/version_edit_example.json).  The edit with
 * comparator "foo", log 300, prev log 0, next file 7, last sequence 128, the
 * pointer (1, "x"@5 VALUE), the deleted file (2, 9) and the new file (3,
 * number 10, size 1000, "a"@1 VALUE .. "b"@2 DELETION) is these 55 bytes:
 *
 *   01 03 66 6f 6f  02 ac 02  09 00  03 07  04 80 01
 *   05 01 09 78 01 05 00 00 00 00 00 00
 *   06 02 09
 *   07 03 0a e8 07 09 61 01 01 00 00 00 00 00 00 09 62 00 02 00 00 00 00 00 00
 *
 * and decodes to the comparator at (2, 3), the pointer key at (18, 9),
 * smallest at (36, 9) and largest at (46, 9).  The reference's own test
 * (version_edit.rs:391-417) ends in an edit of 288 bytes with SHA-256
 * 9b8d210bdabf8a1c824a8786ced4a9f8599209bdb1b78e9f40f437caf6465a46. */

#ifdef __cplusplus
}
#endif

#endif /* LVGPU_VERSION_EDIT_H */
