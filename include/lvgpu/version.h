/*
 * lvgpu version: Version::Get for a batch of queries over the tables of a
 * version in HBM: several overlapping level-0 tables, then sorted, disjoint
 * runs of tables on levels 1-6.
 *
 * A read that misses the memtable goes through Version::Get.  With K tables a
 * caller of table.h has one route: K launches of lv_sst_get_bloom_device, each
 * over every query, and then a pick among K result arrays.  Upstream touches
 * at most one table per level >= 1 and stops at the first answer; so does
 * lv_version_get_device, in one launch.
 *
 * Parity.  The reference holds the data and nothing that uses it:
 * FileMetaData {number, file_size, smallest, largest, allowed_seeks}
 * (src/version_edit.rs:63-91), NUM_LEVELS = 7 (src/config.rs:18), and `fn get`
 * is an unimplemented trait line (src/db.rs:37).  The algorithm is therefore
 * upstream C++ LevelDB's (db/version_set.cc: Version::Get, ForEachOverlapping,
 * Match, FindFile), as the block layout and the filter are (table.h).  No
 * LevelDB library was available, so parity with a stock LevelDB is UNPINNED.
 * What pins the behaviour: the worked example below
 * (tests/golden/version_get_example.json), an independent serial Python model
 * (tests/version_cases.py), and the rule that over a consistent version (newer
 * data never below older data) every answer equals lv_memtable_get_host's over
 * the union of all files' entries.
 *
 * Out of scope: the memtable / immutable-memtable fall-through in front
 * (DBImpl::Get's first two steps: lv_memtable_get_device has the same query
 * arrays and status numbers); UpdateStats / allowed_seeks bookkeeping
 * (seek_file and files_read are what it needs);
 * the table cache; iterators and range reads over a version; compression.
 * (VersionEdit encode / decode, the record of the MANIFEST:
 * lv_version_edit_decode_device / lv_version_edit_encode_device,
 * version_edit.h.  Applying decoded edits to the ordered d_files this header
 * reads (VersionSet::Builder, Recover): lv_version_apply_device,
 * version_set.h; the CURRENT file, compaction picking, allowed_seeks and the
 * comparator-name check stay out of scope.  A compaction's output as a run of tables with their records:
 * lv_compact_output_device, compact.h.  Range reads: lv_memtable_range_device,
 * memtable.h, is DBIter's forward walk over a sorted memtable quadruple; for
 * now a version's range goes through lv_sst_scan_device per table, appended,
 * and lv_memtable_build_device, the merged view, and is read there.  Reading
 * ranges straight from table images, reverse iteration (Prev, SeekToLast) and
 * a streaming merging iterator stay out of scope.)
 *
 * ---- Data (all in device memory) --------------------------------------------
 *
 * Images.  All table images of a version lie in one buffer d_images[0,
 * images_bytes), the "several tables in one arena" idiom of
 * lv_sst_scan_device.  File f occupies [file_off, file_off + file_cap) at any
 * byte alignment (a BUILT image needs file_off % 16 == 0: the build's rule, not
 * this one's).  With one buffer the device can range-check all it is told.
 * d_tables[f] is the lv_sst_table lv_sst_open_device wrote for image f.
 * d_blooms is NULL or lv_sst_bloom[n_files] as lv_sst_bloom_open_device wrote
 * them; present == 0 means no filter for that file.  The smallest and largest
 * internal keys (user key, then the tag as 8 little-endian bytes) lie in
 * d_bound_keys[0, bound_keys_bytes).
 *
 * d_files[0, n_files) is ordered by level ascending.  Level 0 is in strictly
 * descending `number`, newest first (upstream sorts its level-0 candidates by
 * NewestFirst on every Get; here the caller does it once).  Levels >= 1 are in
 * key order.  The structs are plain data: a caller may fill d_files from the
 * host (status 0) as well as with lv_version_file_device.
 *
 * ---- lv_version_file_device --------------------------------------------------
 *
 * Fills one lv_version_file from an opened image, so a device chain needs no
 * host knowledge of keys.  One one-thread launch; stream-ordered, capturable.
 * *d_bound_used is a device cursor into d_bound_keys, read and advanced, so
 * calls append.  *d_out is always written: number, file_off, file_cap and
 * level are the arguments'; status is decided once, in this order:
 *   NO_TABLE    d_table->status != 0 or d_table->file_bytes > file_cap.
 *   BAD_EXTENT  [file_off, file_off + file_cap) is not inside d_images[0,
 *               images_bytes).
 *   EMPTY       file_bytes == 0, or a boundary block has no entry.
 *   CORRUPT     the serial contract below says so.
 *   BOUND_OVER  the two keys do not fit behind the cursor: the cursor is not
 *               advanced and the bytes needed are reported in `reserved`, so
 *               one retry suffices.
 * On any status the off / len fields are 0 and the cursor stays; no byte of
 * d_bound_keys at or beyond bound_keys_cap is ever written.
 *   Serial contract (decode, the restart header (n, arr), the handle's range
 *   rule: table.h, "Get").  The index handle of *d_table is range-checked and
 *   its header read; n < 1: CORRUPT.  A boundary block is named by the entry at
 *   an index restart: a failed decode (limit arr), shared != 0, a key under 8
 *   bytes, a value that does not begin with a handle in range, or a type byte
 *   other than 0: CORRUPT; so is a block header that does not decode.
 *   smallest: the block of index restart 0; n == 0 or arr == 0: EMPTY; its
 *   entry at offset 0 must decode with shared == 0 and a key of at least 8
 *   bytes (CORRUPT); smallest is that key.  largest: the block of the last
 *   index restart; n == 0: EMPTY; walk from its last restart to arr: each
 *   entry must decode (limit arr) with shared <= the previous key's length (0
 *   at the start) and a resulting key of at least 8 bytes (CORRUPT); no entry:
 *   EMPTY; largest is the last key, materialised in place in d_bound_keys.
 *   smallest goes to [cursor, cursor + smallest_len), largest directly behind.
 *
 * ---- lv_version_open_device --------------------------------------------------
 *
 * Validates the descriptor and writes *d_version.  Two launches: a one-thread
 * init, then (n_files != 0) one lane per file with an uncapped grid.  Each
 * lane judges file f and the pair (f - 1, f) whatever the others found; its
 * bits are ORed into status, and first_bad is the smallest index with a bit,
 * by atomic min, or n_files if there is none.  files = n_files always.
 *   UPSTREAM   the optional *d_upstream_status != 0.  No file is judged:
 *              status is UPSTREAM alone and first_bad = n_files.
 *   BAD_FILE   file.status != 0, level >= 7, the image extent lies outside
 *              d_images[0, images_bytes), or d_tables[f].file_bytes is 0 or
 *              > file_cap.
 *   BAD_TABLE  d_tables[f].status != 0.
 *   BAD_BOUND  a bound's extent lies outside d_bound_keys[0,
 *              bound_keys_bytes), a bound is shorter than 8 bytes, or smallest
 *              > largest under InternalKeyComparator.
 *   UNSORTED   level[f-1] > level[f]; or both on level 0 and number[f-1] <=
 *              number[f]; or both on one level >= 1 and icmp(largest[f-1],
 *              smallest[f]) >= 0 (Builder::SaveTo's assertion; made only when
 *              the bounds of both files are in range, a bad one being its own
 *              lane's BAD_BOUND).
 * level_start[l] is the index of the first file with level >= l, and
 * level_start[7] = n_files.  With any status every level_start is 0.  (The
 * init stores n_files everywhere; the lane of the first file of a level takes
 * the atomic min with its index, a lane with a bit the atomic min with 0: min
 * is order-free, so the result does not depend on scheduling.)  n_files == 0
 * is the empty version: status 0, and every get answers ABSENT.
 *
 * ---- lv_version_get_device ---------------------------------------------------
 *
 * One launch, one lane per query, its shape depending only on nq;
 * stream-ordered, no host synchronisation, workspace or staging; capturable
 * like the open.  The query arrays, the statuses 0-6 and their order are
 * exactly lv_sst_get_device's (table.h): NO_TABLE when *d_version is not sound
 * (its status != 0; or, not this version's: files != n_files, level_start[0]
 * != 0, level_start[7] != n_files or level_start not ascending), then BAD_SEQ,
 * then BAD_QUERY.  Every field of every result is written.  The contract is
 * this serial algorithm, with target (q, (seq << 8) | 1) and user(k) the
 * internal key k without its tag:
 *
 *   visit(f): if last != none and seek_file == 0: seek_file = last + 1
 *                                                      (upstream's GetStats)
 *             last = f; ++files_read
 *             r = Get of table.h over image f by d_tables[f], asking the filter
 *                 of f if d_blooms and d_blooms[f].present == 1
 *             if r.reserved == LV_SST_GET_FILTERED: ++filtered
 *             if r.status == ABSENT: go on
 *             else: the answer is r with val_off += file_off (FOUND only),
 *                   file = f, level = level of f; stop
 *   level 0:  for f in [level_start[0], level_start[1]) in order:
 *               if q >= user(smallest_f) and q <= user(largest_f) bytewise:
 *                 visit(f)
 *   level 1..6, its n files from `first`: none: next level.  FindFile: lo = 0,
 *             hi = n; while lo < hi: mid = lo + (hi - lo) / 2;
 *             icmp(largest[first + mid], target) < 0 ? lo = mid + 1 : hi = mid.
 *             If lo < n and q >= user(smallest[first + lo]): visit(first + lo).
 *   no answer: ABSENT.
 *
 * files_read, seek_file (1 + index, 0 = none) and filtered are set for every
 * searched query, ABSENT included.  val_off (absolute in d_images), tag,
 * val_len, block, file and level are 0 unless the status sets them: FOUND all
 * of them, DELETED all but val_off and val_len, CORRUPT file and level.  A
 * file's CORRUPT stops the search (upstream returns the table's error).  A
 * filtered file counts as read, as upstream's Match counts it.
 *
 * Safety.  Get reads nothing outside d_images[0, images_bytes), d_bound_keys[0,
 * bound_keys_bytes) and the n_files entries of d_files, d_tables and d_blooms,
 * even for a *d_version, d_files, d_tables or d_blooms that were not written
 * for each other: every bound extent, image extent, table and level_start
 * taken from device memory is range-checked again in the kernel where it is
 * used (a bound: in range and at least 8 bytes; a visit: the image extent in
 * range, d_tables[f].status == 0 and file_bytes <= file_cap).  A failing check
 * makes the query NO_TABLE with every other field 0.
 *
 * Worked example (tests/golden/version_get_example.json; entries are
 * (user key, sequence, value) or DEL; M = LV_MT_MAX_SEQUENCE; level 2 is
 * empty):
 *   f0  L0  number 9   (b,10,"b10") (d,11,DEL)
 *   f1  L0  number 5   (a,7,"a7") (b,8,"b8") (e,9,"e9")
 *   f2  L1  number 3   (a,3,"a3") (c,4,"c4")
 *   f3  L1  number 4   (d,5,"d5") (f,6,"f6")
 *   f4  L3  number 1   (b,1,"b1") (g,2,"g2")
 *   query    result      file level files_read seek_file
 *   (b,M)    FOUND b10    0    0      1          0
 *   (b,9)    FOUND b8     1    0      2          1
 *   (b,5)    FOUND b1     4    3      4          1    f0, f1, f2 read and absent
 *   (d,M)    DELETED      0    0      1          0
 *   (d,10)   FOUND d5     3    1      3          1
 *   (c,M)    FOUND c4     2    1      3          1
 *   (c,3)    ABSENT       -    -      3          1    FindFile passes f2: (c,4) <
 *            (c,3) under icmp; f3 is skipped by its smallest; f4 is read.  A
 *            FindFile by user key would read f2.
 *   (e,M)    FOUND e9     1    0      1          0    f0 does not overlap
 *   (h,M)    ABSENT       -    -      0          0
 *   ("",M)   ABSENT       -    -      0          0
 *
 * Arguments, checked on the host before any device call (LV_ERR_INVALID,
 * lv_last_error): NULL pointers the call needs (d_images only with
 * images_bytes == 0, d_bound_keys only with a capacity of 0, d_files and
 * d_tables only with n_files == 0, d_qkeys only with qkeys_bytes == 0, the
 * query arrays and d_results only with nq == 0; d_blooms and
 * d_upstream_status may be NULL); every struct array, d_bound_used,
 * d_upstream_status, d_q_off and d_q_seq 8-byte aligned, d_q_len 4-byte
 * aligned; flags == 0; nq <= 2^32 - 2; n_files <= LV_VERSION_MAX_FILES; level
 * < LV_NUM_LEVELS (lv_version_file_device); d_results[0, nq) must not overlap
 * d_images[0, images_bytes).  Without a usable GPU a well-formed call fails
 * with the runtime's error: there is no host fallback.
 */
#ifndef LVGPU_VERSION_H
#define LVGPU_VERSION_H

#include <stddef.h>
#include <stdint.h>

#include "table.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LV_NUM_LEVELS 7u                 /* config.rs:18 */
#define LV_VERSION_MAX_FILES (1u << 20)

typedef struct lv_version_file {         /* 64 bytes, 8-B aligned; FileMetaData (version_edit.rs:63-72) + level */
    uint64_t number, file_off, file_cap, smallest_off, largest_off;
    uint32_t smallest_len, largest_len, level, status;   /* status: lv_version_file_device's, 0 when filled by hand */
    uint64_t reserved;
} lv_version_file;
#define LV_VERSION_FILE_NO_TABLE   1u
#define LV_VERSION_FILE_BAD_EXTENT 2u
#define LV_VERSION_FILE_EMPTY      3u
#define LV_VERSION_FILE_CORRUPT    4u
#define LV_VERSION_FILE_BOUND_OVER 5u
#define LV_VERSION_FILE_UNPLACED   6u    /* lv_version_apply_device (version_set.h): no image placement for the file */

/* (lv_version_state, not lv_version: that name is crc32c.h's version-string function) */
typedef struct lv_version_state {        /* device memory, 8-B aligned, always written */
    uint64_t files, level_start[LV_NUM_LEVELS + 1], first_bad, status;
} lv_version_state;
#define LV_VERSION_OPEN_UPSTREAM   1u
#define LV_VERSION_OPEN_BAD_FILE   2u
#define LV_VERSION_OPEN_BAD_TABLE  4u
#define LV_VERSION_OPEN_BAD_BOUND  8u
#define LV_VERSION_OPEN_UNSORTED  16u

typedef struct lv_version_get_result {   /* 48 bytes */
    uint64_t val_off;                    /* absolute in d_images */
    uint64_t tag;
    uint32_t val_len, block, status, file;          /* file: index into d_files of the table that answered */
    uint32_t level, files_read, seek_file, filtered; /* seek_file: 1 + index, 0 = none */
} lv_version_get_result;

int lv_version_file_device(const uint8_t *d_images, uint64_t images_bytes, uint64_t file_off, uint64_t file_cap,
                           const lv_sst_table *d_table, uint64_t number, uint32_t level,
                           uint8_t *d_bound_keys, uint64_t bound_keys_cap, uint64_t *d_bound_used,
                           lv_version_file *d_out, uint32_t flags, void *stream);
int lv_version_open_device(uint64_t images_bytes, const lv_version_file *d_files, const lv_sst_table *d_tables,
                           size_t n_files, const uint8_t *d_bound_keys, uint64_t bound_keys_bytes,
                           const uint64_t *d_upstream_status, lv_version_state *d_version, uint32_t flags, void *stream);
int lv_version_get_device(const uint8_t *d_images, uint64_t images_bytes, const lv_version_file *d_files,
                          const lv_sst_table *d_tables, const lv_sst_bloom *d_blooms, size_t n_files,
                          const uint8_t *d_bound_keys, uint64_t bound_keys_bytes, const lv_version_state *d_version,
                          const uint8_t *d_qkeys, size_t qkeys_bytes, const uint64_t *d_q_off,
                          const uint32_t *d_q_len, const uint64_t *d_q_seq, size_t nq,
                          lv_version_get_result *d_results, uint32_t flags, void *stream);

/* The host twins (pure, no GPU): the same core compiled for the host, over
 * host memory, with the same statuses (lv_version_open_host has no UPSTREAM).
 * lv_version_get_host answers one query (BAD_QUERY cannot occur).  Each
 * returns 0, or LV_ERR_INVALID for a NULL pointer the call needs, n_files
 * above LV_VERSION_MAX_FILES, level >= LV_NUM_LEVELS or qkey_len >= 2^32. */
int lv_version_file_host(const uint8_t *images, uint64_t images_bytes, uint64_t file_off, uint64_t file_cap,
                         const lv_sst_table *table, uint64_t number, uint32_t level,
                         uint8_t *bound_keys, uint64_t bound_keys_cap, uint64_t *bound_used, lv_version_file *out);
int lv_version_open_host(uint64_t images_bytes, const lv_version_file *files, const lv_sst_table *tables,
                         size_t n_files, const uint8_t *bound_keys, uint64_t bound_keys_bytes, lv_version_state *version);
int lv_version_get_host(const uint8_t *images, uint64_t images_bytes, const lv_version_file *files,
                        const lv_sst_table *tables, const lv_sst_bloom *blooms, size_t n_files,
                        const uint8_t *bound_keys, uint64_t bound_keys_bytes, const lv_version_state *version,
                        const uint8_t *qkey, size_t qkey_len, uint64_t seq, lv_version_get_result *result);

#ifdef __cplusplus
}
#endif

#endif /* LVGPU_VERSION_H */
