/*
 * lvgpu table — SSTable block trailers on MI355X and the table-format codecs
 * around them.
 *
 * Format (src/table/format.rs): BlockHandle {offset, size} as two varint64s
 * (format.rs:26-50, coding.rs:144-166, 223-241, 284-288) and the 48-byte
 * Footer {metaindex handle, index handle, zero pad to 40 B, LE64 magic
 * 0xdb4775248b80fb57} (format.rs:52-104).
 *
 * Block trailer: the reference declares Options::verify_checksums
 * (options.rs:84) but has no block trailer yet, so the layout is upstream
 * LevelDB's: block contents, then type (1 B, 0 = no compression), then
 * LE32(mask(crc32c(contents || type))) — 5 bytes after each handle's extent.
 * Parity beyond the crc32c KATs is unpinned (no reference code or fixture).
 */
#ifndef LVGPU_TABLE_H
#define LVGPU_TABLE_H

#include <stddef.h>
#include <stdint.h>

#include "memtable.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LV_SST_MAGIC 0xdb4775248b80fb57ull   /* format.rs:24 */
#define LV_SST_BLOCK_HANDLE_MAX 20u          /* format.rs:35 */
#define LV_SST_FOOTER_SIZE 48u               /* format.rs:70 */
#define LV_SST_TRAILER_SIZE 5u               /* type + masked crc */
#define LV_SST_NO_COMPRESSION 0u

/* Per-block verify status */
#define LV_SST_BLOCK_OK 0u
#define LV_SST_BLOCK_CHECKSUM_MISMATCH 1u
#define LV_SST_BLOCK_OUT_OF_RANGE 2u  /* offset + size + 5 > file bytes, or size >= 2^32 - 1 */

/* BlockHandle::encode_to (format.rs:37-40): writes <= 20 bytes, returns the count. */
size_t lv_sst_block_handle_encode(uint64_t offset, uint64_t size, uint8_t *dst);
/* BlockHandle::decode_from (format.rs:42-49) over src[0..n): LV_OK and the
 * bytes consumed, or LV_ERR_CORRUPTION ("bad handle"). */
int lv_sst_block_handle_decode(const uint8_t *src, size_t n, uint64_t *offset, uint64_t *size, size_t *consumed);
/* Footer::encode_to (format.rs:72-80) into out[48]. */
void lv_sst_footer_encode(uint64_t metaindex_offset, uint64_t metaindex_size, uint64_t index_offset,
                          uint64_t index_size, uint8_t *out);
/* Footer::decode_from (format.rs:82-103) over src[0..n), n >= 48:
 * handles = {metaindex offset, size, index offset, size}.  LV_ERR_CORRUPTION
 * with "not a sstable (bad magic number)" or "bad handle". */
int lv_sst_footer_decode(const uint8_t *src, size_t n, uint64_t handles[4]);

/* Seal n blocks of a device-resident table being built: for handle i
 * (d_handles[2i] = offset, d_handles[2i+1] = size) write the type byte
 * (d_types ? d_types[i] : 0) at offset+size and the masked crc32c of
 * contents||type at offset+size+1.  Handles must be in range and disjoint. */
int lv_sst_seal_blocks_device(uint8_t *d_file, uint64_t file_bytes, const uint64_t *d_handles,
                              const uint8_t *d_types, size_t n, void *stream);
/* Verify n blocks of a device-resident table: d_status[i] = LV_SST_BLOCK_*
 * (a ReadOptions::verify_checksums read of every block at once).  Optionally
 * d_crc[i] = crc32c(contents || type) (NULL to skip). */
int lv_sst_verify_blocks_device(const uint8_t *d_file, uint64_t file_bytes, const uint64_t *d_handles, size_t n,
                                uint32_t *d_status, uint32_t *d_crc, void *stream);
/* Host-memory variant: copies the table and handles in, verifies, copies
 * the statuses back (end-to-end path). */
int lv_sst_verify_blocks_host(const uint8_t *file, uint64_t file_bytes, const uint64_t *handles, size_t n,
                              uint32_t *status, int device);

/* ---- Build: the sorted memtable to an SSTable image ------------------------
 *
 * The level-0 flush.  lv_sst_build_device walks the memtable
 * lv_memtable_build_device left in HBM (memtable.h) in d_order order and
 * writes a complete table file image into d_file: data blocks, a metaindex
 * block, an index block, every block's trailer, the footer.  Every entry of
 * d_order is written: shadowed versions, deletions and exact duplicates stay
 * unless lv_compact_filter_device (compact.h) took them out of the order.
 *
 * Parity.  The reference stops at table/format.rs (BlockHandle, Footer, the
 * magic number): it has no BlockBuilder, no TableBuilder and no
 * FindShortestSeparator.  The block and index layout below is therefore
 * upstream C++ LevelDB's, as the trailer's (above) and the memtable order's
 * (memtable.h) are.  No LevelDB library was available to open an image, so
 * "a stock LevelDB opens it" is UNPINNED.  What pins the format: the worked
 * example below (tests/golden/sst_build_one_entry.json), an independent Python
 * model with a reader (tests/sst_build_cases.py), lv_sst_footer_decode,
 * lv_sst_verify_blocks_device and the project's own reader (lv_sst_open_device
 * and lv_sst_get_device, below), which opens and reads every table it writes.
 *
 * Options: block_size (default 4096), restart_interval (default 16); no
 * compression (type byte 0), no filter policy (lv_sst_build_bloom_device,
 * "Bloom filter blocks" below, is the build with one).  A NULL opt means the
 * defaults.
 *
 * An entry's key is the internal key: the user key, then the tag as 8
 * little-endian bytes.
 *
 * Data block (BlockBuilder).  State: buffer, restarts = [0], counter = 0,
 * last_key = "".  add(key, value): if counter < restart_interval, shared =
 * the common-prefix length of last_key and key over internal-key bytes (it may
 * run through the user key into the tag, or from one key's tag into the next
 * key's user bytes); otherwise push len(buffer) onto restarts, counter = 0,
 * shared = 0.  Append varint32(shared), varint32(len(key) - shared),
 * varint32(len(value)), key[shared:], value; last_key = key; ++counter.
 * estimate = len(buffer) + 4 * len(restarts) + 4.  finish() appends every
 * restart as fixed32 LE, then len(restarts) as fixed32 LE.
 *
 * Table (TableBuilder).  add(key, value): if an index entry is pending, add
 * (shortest_separator(last_key, key), handle encoding of the pending handle)
 * to the index block and clear it; last_key = key; add the entry to the data
 * block; if estimate >= block_size (checked after the add, so a block holds
 * at least one entry) finish the block, write it and set pending.  Writing a
 * block at offset: the handle is {offset, len(raw)}; the file gets raw, the
 * type byte 0 and LE32(mask(crc32c(raw || type))); offset += len(raw) + 5.
 * finish(): flush the open data block if it is not empty; write the metaindex
 * block, an empty BlockBuilder (the 8 bytes 00 00 00 00 01 00 00 00); if an
 * index entry is pending add (short_successor(last_key), handle encoding);
 * write the index block, a BlockBuilder with restart_interval = 1; write the
 * footer, lv_sst_footer_encode(metaindex, index).
 *
 * Separators.  u(k) is the user key of internal key k; MAXTAG is
 * ((2^56 - 1) << 8) | 1, the bytes 01 ff ff ff ff ff ff ff.
 *   shortest_separator(a, b): d = the common-prefix length of u(a) and u(b).
 *     If d >= min(len u(a), len u(b)): a.  Otherwise c = u(a)[d]; if c < 0xff
 *     and c + 1 < u(b)[d]: u(a)[:d] + byte(c + 1) + MAXTAG; otherwise a.
 *   short_successor(a): i = the first index with u(a)[i] != 0xff; none (the
 *     empty key included): a.  Otherwise t = u(a)[:i] + byte(u(a)[i] + 1); if
 *     len(t) < len(u(a)): t + MAXTAG, else a.
 *
 * Worked example: one entry, key "k", sequence 1, VALUE, value "v", defaults.
 *   [0,21)    data block 00 09 01 6b 01 01 00 00 00 00 00 00 76 | 00 00 00 00
 *             | 01 00 00 00          [21,26)  its trailer
 *   [26,34)   the metaindex block    [34,39)  its trailer
 *   [39,61)   index block 00 09 02 6b 01 01 00 00 00 00 00 00 00 15 |
 *             00 00 00 00 | 01 00 00 00      [61,66)  its trailer
 *   [66,114)  footer 1a 08 27 16, zero padding to 40 bytes, the magic
 *
 * Inputs.  d_payload, payload_bytes, d_ops and op_cap are those of the
 * memtable build; d_order and *d_mt_totals are what it wrote.  *d_mt_totals is
 * read on the device in stream order; entries is never read on the host.
 *
 * Outputs.  d_file[0, file_bytes) is the image.  d_handles holds
 * {offset, size} pairs of the data blocks in file order, then the metaindex
 * block, then the index block: data_blocks + 2 pairs, directly usable by
 * lv_sst_verify_blocks_device; the caller provides room for block_cap + 2
 * pairs.  *d_totals is always written.  The statuses are bits and may
 * combine; on any of them no byte of d_file or d_handles is written:
 *   NO_TABLE     the memtable's status is not 0 (or its entries exceed
 *                op_cap, or an order index or an extent is out of range:
 *                not the memtable build's arguments); entries = 0.
 *   HANDLE_OVER  data_blocks > block_cap; the true data_blocks and file_bytes
 *                are still reported.
 *   FILE_OVER    file_bytes > file_cap; the true file_bytes is reported, so
 *                the caller can retry once.
 *   BLOCK_LARGE  some block's raw size is >= 2^32 - 1, which the seal kernel
 *                rejects.  Sizes are computed in u64: no length wraps.
 * With status 0 no byte of d_file at or beyond file_bytes is written.  An
 * empty memtable (entries == 0, status 0) writes nothing and reports
 * file_bytes = 0, data_blocks = 0 (upstream's BuildTable leaves no file).
 *
 * lv_sst_build_file_bound returns a file_cap that always suffices when the
 * ops' key and value extents are disjoint, as lv_write_batch_decode_device's
 * are (saturating at 2^64 - 1).  With n = op_cap entries and B <= n blocks:
 *   data entries   sum(key_len + val_len) <= payload_bytes, plus per entry at
 *                  most 15 bytes of varints, 8 tag bytes and 4 bytes of its
 *                  restart (restart_interval >= 1): payload_bytes + 27 n;
 *   per data block 4 (the restart count) + 5 (the trailer): 9 n;
 *   index          one entry per block: a key no longer than the block's last
 *                  (the index keys together <= payload_bytes) + 8 tag bytes +
 *                  7 of varints + at most 20 of handle + 4 of restart:
 *                  payload_bytes + 39 n, and 4 + 5 for its count and trailer;
 *   metaindex 8 + 5, footer 48.
 * so the bound is 2 payload_bytes + 75 n + 70.
 *
 * Arguments, checked on the host before any device call (LV_ERR_INVALID,
 * lv_last_error): NULL pointers (d_payload only with payload_bytes == 0, d_ops
 * and d_order only with op_cap == 0, d_file only with file_cap == 0), d_ops
 * and d_file 16-byte aligned, d_handles, d_totals and d_mt_totals 8-byte
 * aligned, d_order 4-byte aligned, d_workspace 16-byte aligned and >=
 * lv_sst_build_workspace_bytes(op_cap, block_cap) bytes, flags == 0,
 * 1 <= restart_interval <= 1024, 1 <= block_size <= 2^30,
 * op_cap <= 2^32 - 2, block_cap <= 2^32 - 4, and d_file[0, file_cap) and
 * d_handles[0, 2 (block_cap + 2)) must not overlap d_payload, d_ops, d_order
 * or each other.  Without a usable GPU a well-formed call fails with the
 * runtime's error: there is no host fallback.
 *
 * Stream-ordered, no host synchronisation, staging or stream queries.  The
 * launch sequence depends only on values the host holds, never on the
 * device-side counts: op_cap and block_cap size the grids and the number of
 * passes, restart_interval the grid of the first carry scan (one wave per
 * residue), and file_cap == 0 leaves out the trailer launches, which could
 * write nothing.  In order: init; entry sizes with a tile-local scan; the tile
 * carries; the successor of every entry; ceil(log2(op_cap)) pointer-doubling
 * passes that mark the block starts (none for op_cap <= 1); the block layout
 * (two tile scans with their carries); the plan, which decides the status
 * once; the entry emit; the index, metaindex, footer and handles; then, with
 * file_cap != 0, the seal (lv_sst_seal_blocks_device's own kernel over a
 * handle array padded to block_cap + 2 in the workspace) for the data blocks
 * and the metaindex block, lv_crc32c_batch_device_ws over the index block as
 * one buffer, which grows with the table, and a one-thread trailer write.
 * With op_cap == 0 only the init, the plan and the handle kernel run.
 * Launches whose work lies beyond the device-side counts return at once.  No
 * workgroup waits on another inside a launch.  It may be captured into a HIP
 * graph once the device has been initialised. */
typedef struct lv_sst_build_options { uint32_t block_size, restart_interval; } lv_sst_build_options;
typedef struct lv_sst_build_totals {   /* device memory, 8-B aligned, always written */
    uint64_t entries, data_blocks, file_bytes,
             metaindex_offset, metaindex_size, index_offset, index_size, status;
} lv_sst_build_totals;
#define LV_SST_BUILD_NO_TABLE     1u
#define LV_SST_BUILD_HANDLE_OVER  2u
#define LV_SST_BUILD_FILE_OVER    4u
#define LV_SST_BUILD_BLOCK_LARGE  8u
#define LV_SST_DEFAULT_BLOCK_SIZE 4096u
#define LV_SST_DEFAULT_RESTART_INTERVAL 16u
#define LV_SST_MAX_BLOCK_SIZE (1u << 30)
#define LV_SST_MAX_RESTART_INTERVAL 1024u

size_t lv_sst_build_workspace_bytes(size_t op_cap, size_t block_cap);
uint64_t lv_sst_build_file_bound(uint64_t payload_bytes, uint64_t op_cap, const lv_sst_build_options *opt);
int lv_sst_build_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops,
                        const uint32_t *d_order, const lv_mt_totals *d_mt_totals, size_t op_cap,
                        const lv_sst_build_options *opt,
                        uint8_t *d_file, uint64_t file_cap, uint64_t *d_handles, size_t block_cap,
                        lv_sst_build_totals *d_totals, uint32_t flags,
                        void *d_workspace, size_t workspace_bytes, void *stream);
/* The host twin (pure, no GPU): a serial restatement of the format above over
 * host memory with the same statuses; trailers by lv_crc32c_extend.  The entry
 * count is mt_totals->entries.  file == NULL with file_cap == 0 is a sizing
 * pass: nothing is written and FILE_OVER is not reported (nor HANDLE_OVER
 * when handles == NULL and block_cap == 0); the totals are the true ones.
 * Returns 0, or LV_ERR_INVALID for a NULL pointer the call needs, options out
 * of range or more than 2^32 - 2 entries. */
int lv_sst_build_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops,
                      const uint32_t *order, const lv_mt_totals *mt_totals,
                      const lv_sst_build_options *opt,
                      uint8_t *file, uint64_t file_cap, uint64_t *handles, size_t block_cap,
                      lv_sst_build_totals *totals);

/* ---- Open: Table::Open over an image in HBM ---------------------------------
 *
 * The read side.  lv_sst_open_device checks the footer and the whole index
 * block of the image d_file[0, *d_file_bytes) and writes *d_table, which
 * lv_sst_get_device then reads on the device.  d_file_bytes and
 * d_upstream_status may point at &build_totals->file_bytes and
 * &build_totals->status of an lv_sst_build_device call; both are read on the
 * device in stream order, never on the host.  d_upstream_status may be NULL.
 * d_file may have any byte alignment (a foreign image may sit anywhere in a
 * buffer): every fixed32 is assembled from bytes.
 *
 * Written from upstream C++ LevelDB's Table::Open, Block::Iter and
 * DecodeEntry, as the build is from its builders.  The project now opens and
 * reads the tables it writes; that a stock LevelDB does so too stays UNPINNED.
 *
 * *d_table is always written.  The statuses are bits; on any of them no byte
 * of d_handles is written.  In the order they are decided:
 *   UPSTREAM     *d_upstream_status != 0.  Every other field is 0.
 *   (empty)      file_bytes == 0 with no upstream status is the empty table
 *                (upstream never writes one; lv_sst_build_device reports it as
 *                file_bytes = 0): status 0, every field 0, nothing written,
 *                and every get answers ABSENT.
 *   NOT_A_TABLE  file_bytes < 48, file_bytes > file_cap, or the last 8 bytes
 *                are not the magic.  file_bytes is reported from here on.
 *   BAD_FOOTER   the footer's two handles, decoded by the rules of
 *                lv_sst_footer_decode over its 48 bytes: a bad varint, or a
 *                handle with offset + size + 5 > file_bytes (u64, no wrap) or
 *                size >= 2^32 - 1.  The four handle fields are reported from
 *                here on.
 *   BAD_INDEX    the index block's type byte is not 0; its size is below 4;
 *                n = LE32 of its last four bytes is not in
 *                [1, (size - 4) / 4] (data_blocks = n from here on; arr =
 *                size - 4 - 4 n); or some restart i does not hold entries that
 *                decode: its run is [restart[i], restart[i + 1]), or
 *                [restart[i], arr) for the last, which must be non-empty and
 *                end at or below arr; its entries (decode, below, with the
 *                run's end as the limit) must tile it exactly, the first with
 *                shared == 0 and every other with shared <= the previous key's
 *                length; every key must be at least 8 bytes; every value must
 *                begin with two varint64s (lv_sst_block_handle_decode; trailing
 *                bytes are ignored) that name a block in range by the footer's
 *                rule.  A failing restart is not walked further.
 *   INDEX_SHAPE  some restart run decodes but holds more than one entry.
 *                Upstream's TableBuilder writes the index with restart
 *                interval 1, as this project does; other shapes are
 *                unsupported, not corrupt.
 *   HANDLE_OVER  d_handles != NULL and data_blocks > block_cap; the true count
 *                is reported.
 * Every restart is judged whatever the others gave, so the status is the OR
 * over all of them and does not depend on a search path.  On status 0
 * d_handles receives the data_blocks data handles in index order, then the
 * metaindex handle, then the index handle: data_blocks + 2 pairs in the layout
 * lv_sst_build_device writes, so lv_sst_verify_blocks_device takes them
 * unchanged (verify_checksums for an image whose handles the caller does not
 * hold).  The caller provides room for block_cap + 2 pairs.
 *
 * Arguments, checked on the host before any device call (LV_ERR_INVALID,
 * lv_last_error): NULL d_table or d_file_bytes, NULL d_file with file_cap != 0,
 * NULL d_handles with block_cap != 0; d_table, d_file_bytes, d_upstream_status
 * and d_handles 8-byte aligned; flags == 0; block_cap <= 2^32 - 4;
 * d_handles[0, 2 (block_cap + 2)) must not overlap d_file[0, file_cap).
 * Without a usable GPU a well-formed call fails with the runtime's error.
 *
 * Stream-ordered, no workspace, no host synchronisation.  A linear chain whose
 * shape depends only on host values: a one-thread kernel (the footer and the
 * index header); a validate kernel, one lane per index restart in a
 * grid-stride loop over a grid sized from block_cap (from file_cap / 4096
 * when block_cap is 0) and capped, which ORs its bits into d_table->status;
 * and, with d_handles != NULL, an emit kernel that decodes the handles again
 * and writes them when the status is 0.  Capturable into a HIP graph once the
 * device has been initialised. */
typedef struct lv_sst_table {            /* device memory, 8-B aligned, always written */
    uint64_t file_bytes, metaindex_offset, metaindex_size, index_offset, index_size,
             data_blocks, reserved, status;
} lv_sst_table;
#define LV_SST_OPEN_UPSTREAM     1u
#define LV_SST_OPEN_NOT_A_TABLE  2u
#define LV_SST_OPEN_BAD_FOOTER   4u
#define LV_SST_OPEN_BAD_INDEX    8u
#define LV_SST_OPEN_INDEX_SHAPE 16u
#define LV_SST_OPEN_HANDLE_OVER 32u
int lv_sst_open_device(const uint8_t *d_file, uint64_t file_cap,
                       const uint64_t *d_file_bytes, const uint64_t *d_upstream_status,
                       uint64_t *d_handles, size_t block_cap,
                       lv_sst_table *d_table, uint32_t flags, void *stream);
/* The host twin (pure, no GPU) over file[0, file_bytes): the same statuses but
 * UPSTREAM.  Returns 0, or LV_ERR_INVALID for a NULL table, a NULL file with
 * file_bytes != 0 or NULL handles with block_cap != 0. */
int lv_sst_open_host(const uint8_t *file, uint64_t file_bytes, uint64_t *handles, size_t block_cap,
                     lv_sst_table *table);

/* ---- Get: Table::InternalGet + SaveValue for nq queries ---------------------
 *
 * Query q is the user key d_qkeys[d_q_off[q], d_q_off[q] + d_q_len[q]) at the
 * snapshot d_q_seq[q]; the query arrays, the BAD_SEQ / BAD_QUERY rules and the
 * status numbers 0-5 are lv_memtable_get_device's (memtable.h), so a caller
 * falls through from memtable to table with one switch.  NO_TABLE: the open's
 * status is not 0 (or d_table->file_bytes > file_cap: not this file's table).
 * Checked in the order NO_TABLE, BAD_SEQ, BAD_QUERY.  Every field of every
 * result is written; those a status does not set are 0 (CORRUPT and ABSENT
 * set none).  file_bytes and the index handle come from *d_table on the
 * device.  Get never reads outside d_file[0, file_bytes), even when given a
 * d_table that open did not write for this file.
 *
 * The target is (user key, (seq << 8) | 1) under InternalKeyComparator: user
 * key bytewise ascending, then tag descending.  The contract is this serial
 * algorithm; for every image, corrupt ones included, the device returns what
 * it returns.
 *
 *   Index seek.  file_bytes == 0: ABSENT.  The index handle is range-checked
 *   again and the block's header read as in block_seek (CORRUPT).  lo = 0,
 *   hi = n; while lo < hi: mid = lo + (hi - lo) / 2; decode the entry at
 *   restart[mid] with limit arr (a failed decode, shared != 0 or a key shorter
 *   than 8 bytes: CORRUPT); if its key is less than the target lo = mid + 1,
 *   otherwise hi = mid.  lo == n: ABSENT.  Otherwise block = lo; its entry is
 *   decoded again, its value must begin with a handle that is in range
 *   (CORRUPT).
 *   Data block.  A type byte at offset + size other than 0: CORRUPT
 *   (compression is unsupported).  The checksum is not verified here: that is
 *   lv_sst_verify_blocks_device over the open's handles.
 *   block_seek(raw, size, target).  size < 4: corrupt.  n = LE32(raw[size-4:]);
 *   n > (size - 4) / 4: corrupt; n == 0: no entry; arr = size - 4 - 4 n.
 *   left = 0, right = n - 1; while left < right: mid = (left + right + 1) / 2;
 *   decode at restart[mid] with limit arr (a failed decode, shared != 0 or a
 *   key shorter than 8 bytes: corrupt); key < target: left = mid, otherwise
 *   right = mid - 1.  Then at = restart[left], previous key length 0; loop:
 *   at >= arr: no entry; decode at `at` (a failed decode, shared > the previous
 *   key's length or a resulting key shorter than 8 bytes: corrupt); key not
 *   less than the target: this entry; otherwise at = the end of its value.
 *   decode(p, limit).  Fewer than 3 bytes before limit fails.  Three varint32
 *   (shared, non_shared, value_len) by GetVarint32Ptr's rule: at most 5 bytes
 *   each, none at or beyond limit, the fifth byte's bits beyond 2^32 dropped, a
 *   sixth continuation byte fails.  limit - p < non_shared + value_len (u64)
 *   fails.
 *   SaveValue.  No entry: ABSENT (upstream does not step into the next block:
 *   a shortened separator's user key is in no block).  The entry's user key
 *   differs from the query's: ABSENT.  Otherwise its type byte 1: FOUND with
 *   val_off (absolute in d_file), val_len, tag, block; 0: DELETED with tag,
 *   block; any other: CORRUPT.
 *
 * Keys may have any length: no key is materialised and no buffer scales with
 * the table's key lengths (csrc/lvk/sst_read.h keeps four registers per lane).
 *
 * One launch, one lane per query, its shape depending only on nq;
 * stream-ordered, no host synchronisation, capturable like the open.
 * Arguments checked on the host (LV_ERR_INVALID): NULL d_table, NULL d_file
 * with file_cap != 0, NULL d_qkeys with qkeys_bytes != 0, NULL query arrays or
 * d_results with nq != 0; d_table, d_q_off, d_q_seq and d_results 8-byte
 * aligned, d_q_len 4-byte aligned; flags == 0; nq <= 2^32 - 2;
 * d_results[0, nq) must not overlap d_file[0, file_cap). */
#define LV_SST_GET_ABSENT    0u
#define LV_SST_GET_FOUND     1u
#define LV_SST_GET_DELETED   2u
#define LV_SST_GET_BAD_SEQ   3u
#define LV_SST_GET_NO_TABLE  4u
#define LV_SST_GET_BAD_QUERY 5u
#define LV_SST_GET_CORRUPT   6u
typedef struct lv_sst_get_result {       /* 32 bytes */
    uint64_t val_off;                    /* absolute offset of the value in d_file */
    uint64_t tag;                        /* (sequence << 8) | type of the entry answered */
    uint32_t val_len, block, status, reserved;
} lv_sst_get_result;
int lv_sst_get_device(const uint8_t *d_file, uint64_t file_cap, const lv_sst_table *d_table,
                      const uint8_t *d_qkeys, size_t qkeys_bytes, const uint64_t *d_q_off,
                      const uint32_t *d_q_len, const uint64_t *d_q_seq, size_t nq,
                      lv_sst_get_result *d_results, uint32_t flags, void *stream);
/* The host twin (pure, no GPU) for one query over file[0, table->file_bytes):
 * the same algorithm compiled for the host.  Returns 0, or LV_ERR_INVALID for
 * a NULL table or result, a NULL file with table->file_bytes != 0 or a NULL
 * qkey with qkey_len != 0 (or qkey_len >= 2^32). */
int lv_sst_get_host(const uint8_t *file, const lv_sst_table *table, const uint8_t *qkey, size_t qkey_len,
                    uint64_t seq, lv_sst_get_result *result);

/* ---- Scan: Table::NewIterator walked to the end, every entry at once --------
 *
 * A table image back to an op table.  lv_sst_scan_device decodes every entry
 * of the image d_file[0, d_table->file_bytes) that lv_sst_open_device opened
 * (*d_table is read on the device in stream order): prefix-compressed keys are
 * materialised, values copied, one lv_wb_op written per entry.  The result is
 * what lv_memtable_build_device and lv_sst_build_device read, so a table can
 * be rewritten with other options, and several tables can be scanned into one
 * arena, sorted by the memtable build and flushed by the table build: a major
 * compaction.  What such a compaction drops (versions hidden behind a newer one
 * that every snapshot sees, deletions with nothing beneath them) is
 * lv_compact_filter_device's to decide, between the sort and the flush
 * (compact.h); without it nothing is dropped.  The merging iterator as a
 * streaming object, several output files and version edits are not part of
 * this.  d_file may have any byte alignment.
 *
 * Output.  base_e / base_b are d_prev->entries / d_prev->arena_bytes, or 0
 * with a NULL d_prev.  Entry i of the table, in table order (index order, then
 * block order), becomes d_ops[base_e + i]: tag is the last 8 bytes of its
 * internal key, little-endian, whatever the type byte (an iterator passes
 * tags through); its user key is materialised at d_arena[key_off, key_off +
 * key_len) and its value copied directly behind, val_off = key_off + key_len
 * always (lv_wb_op's DELETION convention too).  Entries are packed without
 * gaps from base_b on; offsets are relative to d_arena, which may have any
 * byte alignment.  So table_bytes = sum(key_len + val_len) and there is one
 * correct arena, byte for byte.  For a table lv_sst_build_device wrote,
 * table_bytes is the sum of the source ops' key and value lengths; for a
 * foreign image one retry after ARENA_OVER sizes the arena.
 *
 * d_order and d_mt_totals are both NULL or both not; with them d_prev must be
 * NULL.  They complete a memtable quadruple (d_arena as d_payload, d_ops,
 * d_order, *d_mt_totals) that lv_sst_build_device and lv_memtable_get_device
 * take as it is: d_order[i] = i, entries = table_entries, user_keys counted as
 * the memtable build counts it, status 0 when no entry comes before its
 * predecessor under lv_internal_key_compare (equal is allowed: exact
 * duplicates), otherwise status = LV_SST_SCAN_MT_UNORDERED and user_keys = 0;
 * both consumers refuse a status.  On any scan status *d_mt_totals is
 * {0, 0, LV_MT_BUILD_UPSTREAM} and d_order is not written.
 *
 * Appending.  With d_prev a table's entries go behind those of the scan that
 * wrote *d_prev (read on the device; d_prev == d_totals is LV_ERR_INVALID) in
 * the same arena and op table; entries and arena_bytes are cumulative.
 * &d_totals->entries and &d_totals->status of the last scan are then
 * lv_memtable_build_device's d_n_ops and d_upstream_status.
 *
 * *d_totals is always written.  The statuses are bits, decided once, before
 * any byte of d_arena, d_ops or d_order is written; on any of them none of the
 * three is written.
 *   UPSTREAM    d_prev->status != 0.
 *   NO_TABLE    d_table->status != 0, or d_table->file_bytes > file_cap.
 *               With either of these two nothing of the image is read.
 *   CORRUPT     the serial algorithm below says so.
 *   BLOCK_OVER  the index names more data blocks than block_cap; the true
 *               data_blocks is reported and no index entry or block is read.
 *   With any of these four table_entries = table_bytes = runs = 0, entries =
 *   base_e and arena_bytes = base_b.
 *   OP_OVER     base_e + table_entries > op_cap.
 *   ARENA_OVER  base_b + table_bytes > arena_cap.
 *   With only these two every count is the true one, so one retry suffices.
 * file_bytes == 0 with status 0 is the empty table: no entries, status 0.
 * data_blocks is the index block's restart count once its header is sound;
 * runs is the number of restart runs of all data blocks.
 *
 * The contract for bytes is this serial algorithm; the scan never reads
 * outside d_file[0, file_bytes), even when given a d_table that open did not
 * write for this file.  decode, the restart-array header (n, arr) and the
 * handle's range rule are Get's (above).
 *   Index.  The index handle of *d_table is range-checked again; its type
 *   byte must be 0 and its header is read as in Get; n must equal
 *   d_table->data_blocks (CORRUPT).  For restart i in order: decode at
 *   restart[i] with limit arr; a failed decode, shared != 0, a key under 8
 *   bytes, a value that does not begin with a handle, a handle out of range
 *   or a data block whose type byte is not 0: CORRUPT.  (Open has walked the
 *   runs of the index; the scan reads each restart's first entry, as Get.)
 *   Data block.  A header that does not decode: CORRUPT.  n == 0: no entries
 *   and no run.  n == 1 and arr == 0: one run, no entries (the empty
 *   BlockBuilder).  Otherwise restart[0] == 0, the restarts strictly increase
 *   and the last is below arr.  Run r is [restart[r], restart[r + 1]), or ends
 *   at arr for the last; its entries, decoded with the run's end as the limit,
 *   must tile it exactly; the first has shared == 0, every other shared <= the
 *   previous key's length; every key is at least 8 bytes.  Any violation:
 *   CORRUPT.
 * This is stricter than upstream's Block::Iter, which never looks at the
 * restart array while it steps; every block a BlockBuilder writes passes.  It
 * is also what makes the runs independent of each other, so that each can be
 * given to a lane.  The checksums are not verified here: that is
 * lv_sst_verify_blocks_device over the open's handles.
 *
 * Arguments, checked on the host before any device call (LV_ERR_INVALID,
 * lv_last_error): NULL pointers (d_file only with file_cap == 0, d_arena only
 * with arena_cap == 0, d_ops only with op_cap == 0; d_prev may be NULL), d_ops
 * 16-byte aligned, d_table, d_prev, d_totals and d_mt_totals 8-byte aligned,
 * d_order 4-byte aligned, d_workspace 16-byte aligned and >=
 * lv_sst_scan_workspace_bytes(op_cap, block_cap) bytes, flags == 0, op_cap <=
 * 2^32 - 2, block_cap <= 2^32 - 4, the pairing rules of d_order, d_mt_totals
 * and d_prev, and d_arena[0, arena_cap), d_ops[0, op_cap) and d_order[0,
 * op_cap) must overlap neither d_file[0, file_cap) nor each other.  Without a
 * usable GPU a well-formed call fails with the runtime's error.
 *
 * Stream-ordered, no host synchronisation.  The launch sequence depends only
 * on op_cap, block_cap and whether d_order is NULL: a one-thread header (it
 * zeroes the call's state in the workspace); with block_cap != 0 a lane per
 * data block (handle, header, run count, with a tile scan and its carries),
 * then a lane per run that walks it keeping lengths (two tile scans with their
 * carries; the workspace holds op_cap + block_cap runs, and a table with more
 * is OP_OVER, whose true counts are atomic sums); the one-thread plan, which
 * decides every status; with op_cap and block_cap != 0 the emit, a lane per
 * run; with d_order the order kernel and a one-thread finish.  No workgroup
 * waits on another.  Capturable into a HIP graph once the device has been
 * initialised. */
typedef struct lv_sst_scan_totals {      /* device memory, 8-B aligned, always written */
    uint64_t entries, arena_bytes,       /* cumulative: d_prev's plus this table's */
             table_entries, table_bytes, /* this table's alone */
             data_blocks, runs, reserved, status;
} lv_sst_scan_totals;
#define LV_SST_SCAN_UPSTREAM    1u
#define LV_SST_SCAN_NO_TABLE    2u
#define LV_SST_SCAN_CORRUPT     4u
#define LV_SST_SCAN_BLOCK_OVER  8u
#define LV_SST_SCAN_OP_OVER    16u
#define LV_SST_SCAN_ARENA_OVER 32u
#define LV_SST_SCAN_MT_UNORDERED 8u      /* a bit of d_mt_totals->status only; distinct from LV_MT_BUILD_* */

size_t lv_sst_scan_workspace_bytes(size_t op_cap, size_t block_cap);
int lv_sst_scan_device(const uint8_t *d_file, uint64_t file_cap, const lv_sst_table *d_table,
                       const lv_sst_scan_totals *d_prev,
                       uint8_t *d_arena, uint64_t arena_cap, lv_wb_op *d_ops, size_t op_cap, size_t block_cap,
                       uint32_t *d_order, lv_mt_totals *d_mt_totals,
                       lv_sst_scan_totals *d_totals, uint32_t flags,
                       void *d_workspace, size_t workspace_bytes, void *stream);
/* The host twin (pure, no GPU) over file[0, table->file_bytes): the same
 * algorithm compiled for the host, with the same statuses but BLOCK_OVER
 * (and NO_TABLE only from table->status).  Returns 0, or LV_ERR_INVALID for a
 * NULL table or totals, prev == totals, a NULL file, arena or ops the call
 * needs, order and mt_totals not paired or given with prev, or op_cap above
 * 2^32 - 2. */
int lv_sst_scan_host(const uint8_t *file, const lv_sst_table *table, const lv_sst_scan_totals *prev,
                     uint8_t *arena, uint64_t arena_cap, lv_wb_op *ops, size_t op_cap,
                     uint32_t *order, lv_mt_totals *mt_totals, lv_sst_scan_totals *totals);

/* ---- Bloom filter blocks: the build with a filter policy, and a filtered Get --
 *
 * lv_sst_build_bloom_device is lv_sst_build_device with upstream's
 * NewBloomFilterPolicy(bits_per_key): the image gains a filter block and a
 * metaindex block that names it.  lv_sst_bloom_open_device finds the filter of
 * an opened image (Table::ReadMeta / ReadFilter) and lv_sst_get_bloom_device
 * is lv_sst_get_device asking it before it touches a data block, so a lookup
 * of a key the table does not hold usually stops after the index seek.
 * lv_sst_build_device, lv_sst_open_device, lv_sst_get_device and
 * lv_sst_scan_device are unchanged, and they and lv_sst_verify_blocks_device
 * take a bloom image as it is: a reader without a filter policy ignores the
 * metaindex entry.
 *
 * Parity.  The reference has no filter policy at all.  The filter, the filter
 * block and the metaindex entry below are therefore upstream C++ LevelDB's
 * (util/bloom.cc, table/filter_block.cc, table/table_builder.cc,
 * table/table.cc), as the block and index layout (above) and the trailer's
 * are.  No LevelDB library was available to open an image, so "a stock LevelDB
 * opens it" is UNPINNED.  What pins the format: the worked example below
 * (tests/golden/sst_bloom_one_entry.json), the reference's own KAT of the hash
 * at the Bloom seed (hash([0x62], 0xbc9f1d34) == 0xef1345c4), an independent
 * Python model with a reader (tests/sst_bloom_cases.py) and the project's own
 * reader.
 *
 * Bloom filter over n keys at bits_per_key = bpk.
 *   k = min(30, max(1, bpk * 69 / 100)) in integers (upstream's
 *   (size_t)(bpk * 0.69) clamped to [1, 30]; equal for every bpk below 300).
 *   bits = max(64, n * bpk); bytes = (bits + 7) / 8; bits = 8 * bytes.  The
 *   filter is `bytes` zero bytes, then the byte k.  For each key:
 *   h = lv_hash(key, 0xbc9f1d34), delta = rotr32(h, 17); k times: set bit
 *   h % bits (byte pos / 8, bit pos % 8), h += delta (u32 wrap).
 *   A key is a USER key (upstream's InternalFilterPolicy strips the tag), and
 *   every entry adds its key: versions and exact duplicates count in n.
 *   key_may_match(key, filter): len < 2: false.  k = the last byte; k > 30:
 *   true.  bits = 8 (len - 1); probe as above; a clear bit: false.
 *
 * Filter block (FilterBlockBuilder, base lg LV_SST_FILTER_BASE_LG = 11).  A
 * data block that starts at file offset o belongs to window o >> 11.  Filter f
 * is the Bloom filter over the entries of all data blocks of window f, in
 * order; if there are none it is zero bytes, not an empty Bloom filter.
 * Serially: StartBlock(0) at the start; after each data block is written,
 * StartBlock(next offset) runs GenerateFilter while offset / 2048 > filters so
 * far; at finish one more GenerateFilter runs if keys are pending.  The filter
 * count is therefore F = max((last block's offset >> 11) + 1, data_end >> 11)
 * with data_end the offset behind the last data block's trailer.  Contents:
 * the F filters end to end, F fixed32 start offsets, fixed32 array_offset (the
 * filters' total size), the byte 11.  It is written raw at data_end with type
 * 0 and the usual trailer.
 *
 * Metaindex: a BlockBuilder with the table's restart_interval holding the one
 * entry LV_SST_BLOOM_NAME (34 bytes) -> the handle encoding of the filter
 * block.  Order in the file: data blocks, filter block, metaindex, index,
 * footer.
 *
 * Worked example: key "k", sequence 1, VALUE, value "v", defaults, bpk 10.
 * lv_hash("k", 0xbc9f1d34) = 0xeadd29bc, k = 6.
 *   [0,21)    the data block of the example above      [21,26)  its trailer
 *   [26,44)   filter block 40 00 00 01 04 04 10 10 06 | 00 00 00 00 |
 *             09 00 00 00 | 0b                          [44,49)  its trailer
 *   [49,96)   metaindex 00 22 02, the 34 name bytes, 1a 12 | 00 00 00 00 |
 *             01 00 00 00                               [96,101) its trailer
 *   [101,123) the index block, as above                [123,128) its trailer
 *   [128,176) footer 31 2f 65 16, zero padding to 40 bytes, the magic
 *
 * lv_sst_build_bloom_device takes lv_sst_build_device's arguments, with the
 * same checks, and bloom != NULL with 1 <= bits_per_key <= 64 and reserved ==
 * 0 (LV_ERR_INVALID otherwise).  *d_totals is written as there, its metaindex
 * fields naming the metaindex block that holds the entry; *d_bloom_totals
 * (8-byte aligned, always written) is {filter_offset, filter_size, filters,
 * filter_keys}: the filter block's handle, F and the keys added (= entries);
 * all 0 unless the status is 0 and entries != 0.  d_handles receives
 * data_blocks + 3 pairs: the data blocks, the filter block, the metaindex
 * block, the index block; the caller provides room for block_cap + 3 pairs,
 * and lv_sst_verify_blocks_device takes them unchanged.  The four statuses are
 * lv_sst_build_device's, decided once in the plan before any byte is written;
 * BLOCK_LARGE also when the filter block's size reaches 2^32 - 1 (all filter
 * sizes are u64).  file_bytes, metaindex_* and index_* are the true ones under
 * HANDLE_OVER and FILE_OVER.  An empty memtable writes nothing.
 *
 * lv_sst_build_bloom_file_bound: lv_sst_build_file_bound plus
 *   filters        a non-empty filter over n_w keys is max(8, ceil(n_w bpk / 8))
 *                  + 1 <= n_w bpk / 8 + 9 bytes; the n_w sum to n and there
 *                  are at most n of them (one per block): n bpk / 8 + 1 + 9 n;
 *   offsets        4 per window; data_end <= payload_bytes + 36 n (the data
 *                  entries' and blocks' terms above), F <= data_end / 2048 + 1:
 *                  (payload_bytes + 36 n) / 512 + 4;
 *   array_offset, the base byte and the trailer: 10;
 *   metaindex      3 + 34 + at most 20 of handle + 8, against the 8 counted: 57
 * so the bound is 2 payload_bytes + 75 n + 70 + n bpk / 8 + 9 n +
 * (payload_bytes + 36 n) / 512 + 72 (saturating; 0 for op_cap == 0 or a bad
 * bloom).
 *
 * Launch sequence.  lv_sst_build_device's, with two launches added before
 * the plan (per data block its window, whether it is the window's first, the
 * window's key count and filter size with a tile scan; the tile carries) and
 * three behind the entry emit: the filter emit, a wave per non-empty filter in
 * a grid-stride loop over the data blocks, which zeroes the filter's bits in
 * LDS, has its lanes hash the window's user keys and OR their k bits in with
 * LDS atomics, and stores the bytes with plain stores of the destination's
 * alignment (a filter beyond the wave's LDS budget is zero-filled instead);
 * the large-filter kernel, which sets such a filter's bits with atomic ORs on
 * aligned dwords of d_file and stores nothing else; and the offsets kernel, a
 * lane per window.  Bit OR is order-free, so the image is bit-exact however
 * the lanes are scheduled.  The seal covers the data blocks and the metaindex
 * block; the filter block, which grows with the table, joins the index block
 * in the one lv_crc32c_batch_device_ws call as a second buffer.  The grids
 * depend on op_cap, block_cap and file_cap only.  No workgroup waits on
 * another.  Capturable like the build. */
#define LV_SST_BLOOM_NAME "filter.leveldb.BuiltinBloomFilter2"
#define LV_SST_FILTER_BASE_LG 11u
#define LV_SST_BLOOM_SEED 0xbc9f1d34u
typedef struct lv_sst_bloom_options { uint32_t bits_per_key, reserved; } lv_sst_bloom_options;
typedef struct lv_sst_bloom_totals {     /* device memory, 8-B aligned, always written */
    uint64_t filter_offset, filter_size, filters, filter_keys;
} lv_sst_bloom_totals;

/* Host scalars (pure).  lv_bloom_hash is lv_hash at the Bloom seed.
 * lv_bloom_filter_bytes(n, bpk) is the filter's size with its k byte (0 for
 * bpk == 0).  lv_bloom_create_filter builds the filter over the n keys
 * keys[off[i], off[i] + len[i]) into dst[0, lv_bloom_filter_bytes(n, bpk)):
 * LV_OK, or LV_ERR_INVALID for a NULL pointer the call needs or bpk == 0. */
uint32_t lv_bloom_hash(const uint8_t *key, size_t n);
size_t lv_bloom_filter_bytes(size_t n, uint32_t bits_per_key);
int lv_bloom_create_filter(const uint8_t *keys, const uint64_t *off, const uint32_t *len, size_t n,
                           uint32_t bits_per_key, uint8_t *dst);
int lv_bloom_key_may_match(const uint8_t *key, size_t key_len, const uint8_t *filter, size_t filter_len);

size_t lv_sst_build_bloom_workspace_bytes(size_t op_cap, size_t block_cap);
uint64_t lv_sst_build_bloom_file_bound(uint64_t payload_bytes, uint64_t op_cap, const lv_sst_build_options *opt,
                                       const lv_sst_bloom_options *bloom);
int lv_sst_build_bloom_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops,
                              const uint32_t *d_order, const lv_mt_totals *d_mt_totals, size_t op_cap,
                              const lv_sst_build_options *opt, const lv_sst_bloom_options *bloom,
                              uint8_t *d_file, uint64_t file_cap, uint64_t *d_handles, size_t block_cap,
                              lv_sst_build_totals *d_totals, lv_sst_bloom_totals *d_bloom_totals, uint32_t flags,
                              void *d_workspace, size_t workspace_bytes, void *stream);
/* The host twin (pure, no GPU), with lv_sst_build_host's sizing-pass rule and
 * return values; handles has room for block_cap + 3 pairs. */
int lv_sst_build_bloom_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops,
                            const uint32_t *order, const lv_mt_totals *mt_totals,
                            const lv_sst_build_options *opt, const lv_sst_bloom_options *bloom,
                            uint8_t *file, uint64_t file_cap, uint64_t *handles, size_t block_cap,
                            lv_sst_build_totals *totals, lv_sst_bloom_totals *bloom_totals);

/* Reader (FilterBlockReader, Table::ReadMeta / ReadFilter, InternalGet).  Any
 * failure to find or parse the filter means "no filter"; it is never an error.
 *   ReadMeta.  The metaindex handle of *d_table is range-checked, its type
 *   byte must be 0 and its restart header sound (BAD_METAINDEX).  The first
 *   entry whose key is not less than LV_SST_BLOOM_NAME bytewise is found by a
 *   linear walk from offset 0 with limit arr (decode, above; a failed decode
 *   or shared > the previous key's length: BAD_METAINDEX); none, or a key
 *   other than the name: NO_ENTRY.  Its value must begin with a handle that is
 *   in range (BAD_HANDLE) and whose type byte is 0 (BAD_TYPE).  Filter
 *   contents of n < 5 bytes: SHORT; array_offset = LE32 at n - 5 > n - 5:
 *   BAD_ARRAY.  num = (n - 5 - array_offset) / 4; base_lg = the last byte.
 *   may_match(block_offset, key).  i = block_offset >> base_lg (0 for a shift
 *   of 64 or more).  i >= num: true.  start, limit = LE32 at array + 4 i and
 *   array + 4 i + 4.  start <= limit <= array_offset: key_may_match over
 *   [start, limit).  Otherwise start == limit: false.  Otherwise true.
 *
 * lv_sst_bloom_open_device writes *d_bloom (8-byte aligned, every field) from
 * the image and the *d_table lv_sst_open_device wrote, read on the device.
 * {filter_offset, filter_size} is a handle pair lv_sst_verify_blocks_device
 * takes with n = 1.  present is 0 or 1; why is 0 with a filter and otherwise
 * the first reason there is none, in this order: TABLE (d_table->status != 0
 * or its file_bytes > file_cap), EMPTY (file_bytes == 0), then ReadMeta's.
 * One one-thread launch, stream-ordered, capturable.  Arguments (LV_ERR_INVALID):
 * NULL d_table or d_bloom, NULL d_file with file_cap != 0, either not 8-byte
 * aligned, flags != 0.
 *
 * lv_sst_get_bloom_device is lv_sst_get_device plus d_bloom, read on the
 * device in stream order (NULL or misaligned: LV_ERR_INVALID).  With present
 * == 0 the results are byte for byte lv_sst_get_device's.  With a filter it is
 * asked after the index seek has produced a handle that is in range and before
 * anything of the data block is read: a query it rejects gets ABSENT with
 * every other field 0 and reserved = LV_SST_GET_FILTERED; every other query
 * gets what lv_sst_get_device gives.  Every offset taken from *d_bloom is
 * range-checked again against file_bytes: a d_bloom that was not written for
 * this file never causes a read outside d_file[0, file_bytes). */
typedef struct lv_sst_bloom {            /* device memory, 8-B aligned, always written */
    uint64_t filter_offset, filter_size, array_offset, num, base_lg, present, why, reserved;
} lv_sst_bloom;
#define LV_SST_BLOOM_TABLE         1u
#define LV_SST_BLOOM_EMPTY         2u
#define LV_SST_BLOOM_BAD_METAINDEX 3u
#define LV_SST_BLOOM_NO_ENTRY      4u
#define LV_SST_BLOOM_BAD_HANDLE    5u
#define LV_SST_BLOOM_BAD_TYPE      6u
#define LV_SST_BLOOM_SHORT         7u
#define LV_SST_BLOOM_BAD_ARRAY     8u
#define LV_SST_GET_FILTERED 1u           /* lv_sst_get_result.reserved of a query the filter rejected */
int lv_sst_bloom_open_device(const uint8_t *d_file, uint64_t file_cap, const lv_sst_table *d_table,
                             lv_sst_bloom *d_bloom, uint32_t flags, void *stream);
/* The host twin over file[0, table->file_bytes): 0, or LV_ERR_INVALID for a
 * NULL table or bloom or a NULL file with table->file_bytes != 0. */
int lv_sst_bloom_open_host(const uint8_t *file, const lv_sst_table *table, lv_sst_bloom *bloom);
int lv_sst_get_bloom_device(const uint8_t *d_file, uint64_t file_cap, const lv_sst_table *d_table,
                            const lv_sst_bloom *d_bloom,
                            const uint8_t *d_qkeys, size_t qkeys_bytes, const uint64_t *d_q_off,
                            const uint32_t *d_q_len, const uint64_t *d_q_seq, size_t nq,
                            lv_sst_get_result *d_results, uint32_t flags, void *stream);
/* One query on the host: lv_sst_get_host with the filter (bloom != NULL). */
int lv_sst_get_bloom_host(const uint8_t *file, const lv_sst_table *table, const lv_sst_bloom *bloom,
                          const uint8_t *qkey, size_t qkey_len, uint64_t seq, lv_sst_get_result *result);

#ifdef __cplusplus
}
#endif

#endif /* LVGPU_TABLE_H */
