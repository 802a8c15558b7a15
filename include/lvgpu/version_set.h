/*
 * lvgpu version set -- MANIFEST edits applied to a readable version.  C ABI.
 *
 * lv_version_edit_decode_device (version_edit.h) turns the records of a
 * MANIFEST into edits and three row tables; lv_version_open_device and
 * lv_version_get_device (version.h) read a version, an ordered array of
 * lv_version_file.  lv_version_apply_device is the step between them: upstream
 * C++ LevelDB's VersionSet::Builder (db/version_set.cc: Apply over every edit,
 * then SaveTo) together with the bookkeeping of VersionSet::Recover (the last
 * value of each scalar, MarkFileNumberUsed), for edits in HBM.
 *
 * Parity.  The reference has VersionEdit and no VersionSet, so the algorithm
 * is upstream's, restricted to the inputs LevelDB writes; parity with a stock
 * LevelDB is UNPINNED (no LevelDB library was available).  What pins the
 * behaviour: the worked example below (tests/golden/version_apply_example.json),
 * an independent serial Python model written from this comment
 * (tests/version_apply_cases.py), the host twin, which is upstream's Builder
 * written out literally (per-level deleted and added sets, then SaveTo), and
 * the store of tests/store_cases.py, whose Python bookkeeping predates this
 * header.
 *
 * Out of scope: the CURRENT file; compaction picking (Finalize's scores need
 * level_files and level_bytes below, and that is all of it that is here);
 * allowed_seeks; the comparator-name check of Recover (comparator_off /
 * comparator_len name the bytes, the caller compares them).
 *
 * ---- Inputs -------------------------------------------------------------------
 *
 * d_src[0, src_bytes), an lv_ve_encode_in (edits, the three row tables and
 * their bounds arrays), d_records, d_upstream_status and rec_cap: exactly what
 * lv_version_edit_encode_device takes, so the decode's outputs feed in as they
 * are (an edit's status, flags and reserved are ignored).  A caller who points
 * d_upstream_status at the decode totals' bad_records gets upstream's rule
 * that one bad edit fails the recovery.  Only rows inside [bounds[0],
 * bounds[*d_records]) are read.
 *
 * There is no separate base version: a base is record 0 with every file of the
 * version as a NewFile row, which is what upstream's WriteSnapshot writes, and
 * lv_version_edit_files_device makes those rows from lv_version_file records.
 *
 * d_dir[0, dir_n), optional (NULL with dir_n == 0): where each file's image
 * lies in the caller's d_images, lv_vs_placement {number, file_off, file_cap,
 * reserved}, strictly ascending by number.  The MANIFEST does not hold
 * placements; a host keeps them (a table cache's role).
 *
 * ---- Semantics ----------------------------------------------------------------
 *
 * Per (level, number) pair, upstream's Builder:
 *   Records apply in order; within a record the deleted rows apply before the
 *   NewFile rows (Apply's order).
 *   A pair is LIVE iff it has a NewFile row in record r and no deleted row in a
 *   record after r.
 *   Not errors: a deleted row in the record of the NewFile row or in an earlier
 *   one (it has no effect on that file); a deleted row for a pair that was
 *   never added; the same number live on two levels (a trivial move is delete
 *   (L, n) plus add (L + 1, n), and nothing here forbids both to stay).
 *   Two NewFile rows for one pair raise DUPLICATE, whatever lies between them.
 *   LevelDB never reuses a file number, so no MANIFEST it writes has them;
 *   what upstream's std::set would make of such input (it depends on whether
 *   the bounds also repeat) is not worth restating.
 * Compact pointers: per level the last row wins, in record order and then row
 * order: compact_pointer[level] = 1 + that row's index into d_pointers, 0 for
 * none (the seek_file idiom of version.h).
 * Scalars: for each has bit the value of the last record that carries it;
 * has = the OR over all records of the defined bits (LV_VE_HAS_ALL).
 * next_file_number is then raised as MarkFileNumberUsed does, first by
 * log_number and then by prev_log_number where those are set: if
 * next_file_number <= v it becomes v + 1 (u64 arithmetic).  max_file_number is
 * the largest number among the live files, 0 for none: what to do with it
 * stays with the host.  Missing scalars are reported through `has` and not
 * judged (Recover's "no meta-nextfile entry" is the caller's to raise).
 * A key (level << 56 | number) must fit 64 bits, so a file number of 2^56 or
 * more is BAD_ROW (LevelDB's numbers count files; 2^56 is out of reach).
 *
 * ---- Outputs ------------------------------------------------------------------
 *
 * d_files_out[0, live): lv_version_file rows in the order version.h requires:
 * level ascending; level 0 by number descending; levels >= 1 by smallest
 * internal key under InternalKeyComparator (user key ascending bytewise, tag
 * descending), then number ascending.  The bound extents are the NewFile rows'
 * own extents into d_src, so d_src is the d_bound_keys of
 * lv_version_open_device: no key byte is copied.  file_off and file_cap come
 * from the directory; with no directory they are 0 and file_size.  reserved =
 * the NewFile row's index into d_files, so file_size stays reachable.  status
 * is 0, or LV_VERSION_FILE_UNPLACED when there is a directory and the number
 * is not in it or its file_cap < file_size: lv_version_open_device then
 * reports BAD_FILE, unchanged.
 * d_dir_index[0, live), optional (NULL allowed): the directory index of each
 * live file, 2^32 - 1 when the file is unplaced or there is no directory.
 * *d_totals is always written:
 *   records                       *d_records
 *   new_files, deleted, pointers  the rows read
 *   live, unplaced                the live files, and those of them UNPLACED
 *   level_files[7], level_bytes[7] per level the live files and the sum of
 *                                 their file_size
 *   compact_pointer[7], the four scalars, comparator_off / comparator_len (of
 *   the last record with HAS_COMPARATOR), has, max_file_number: as above
 *   status                        LV_VS_* bits
 *   bad_kind, bad_row             2^64 - 1 unless a bit below sets them
 *
 * The status bits are judged in this order and the first one raised ends the
 * judging; with a bit set only *d_totals is written, and of the totals only
 * records, status, bad_kind and bad_row are not 0 -- except FILE_OVER:
 *   UPSTREAM       *d_upstream_status != 0: records = 0 too.
 *   REC_OVER       *d_records > rec_cap: records = *d_records.
 *   BAD_BOUNDS     not (b[r] <= b[r + 1] <= cap) for a bounds array b: bad_row
 *                  = the lowest such record r, bad_kind = the lowest kind that
 *                  fails on it (LV_VE_KIND_POINTER, _DELETED, _FILE).  No row
 *                  is read.
 *   BAD_ROW        a row with a level of 7 or more; a deleted or NewFile row
 *                  with a number of 2^56 or more; a pointer, smallest or
 *                  largest key whose extent lies outside d_src or that is
 *                  shorter than 8 bytes.  bad_kind = the lowest kind with such
 *                  a row (the encode's order: POINTER, DELETED, FILE), bad_row
 *                  = the lowest such index into that kind's table.  No byte of
 *                  d_src is read before every row is accepted.
 *   DUPLICATE      bad_kind = LV_VE_KIND_FILE, bad_row = the lowest NewFile row
 *                  index that has an earlier row of its pair.
 *   BAD_DIRECTORY  bad_kind = LV_VS_KIND_DIRECTORY, bad_row = the lowest i with
 *                  d_dir[i - 1].number >= d_dir[i].number.
 *   FILE_OVER      live > files_cap: every total is the true one, so one retry
 *                  suffices.
 *
 * Arguments, checked on the host before any device call (LV_ERR_INVALID,
 * lv_last_error): in, out, d_totals, d_records and the three bounds arrays are
 * never NULL; d_src only with src_bytes == 0, a row table only with its cap ==
 * 0, d_edits only with rec_cap == 0, d_dir only with dir_n == 0, d_files_out
 * only with files_cap == 0; the row tables and d_edits 16-byte aligned;
 * d_totals, the bounds, d_dir and d_files_out 8-byte aligned, d_dir_index
 * 4-byte aligned; d_workspace 16-byte aligned and >=
 * lv_version_apply_workspace_bytes(file_cap, deleted_cap, files_cap) bytes;
 * flags == 0; rec_cap <= 2^32 - 2; every row cap and dir_n <= 2^30; files_cap
 * <= LV_VERSION_MAX_FILES; d_files_out and d_dir_index overlap no input.
 * Without a usable GPU a well-formed call fails with the runtime's error:
 * there is no host fallback.
 *
 * Stream-ordered, no host synchronisation, no memset; capturable into a HIP
 * graph once the device is initialised.  The launch sequence depends only on
 * the capacities: a clear of the workspace's head and pair table; the bounds
 * and scalars, a lane per record; the rows and the directory, a lane per item
 * (validation, and each accepted row entered into an open-addressing table of
 * 64-bit keys, a power of two of at least 2 x (file_cap + deleted_cap) slots,
 * which keeps per pair the largest deleting record by atomic max and the
 * lowest adding row by atomic min); liveness, placement and a tile scan, a
 * lane per NewFile row; one wave that carries the tiles, decides the status
 * and writes the totals; a gather of the live rows into sort entries; a tile
 * sort and ceil(log2(files_cap / 1024)) merge passes (the memtable build's
 * sort, lvk/merge_sort.h, under this order); the emit, a lane per live file.
 * No workgroup waits on another inside a launch, and every lowest-index report
 * is an atomic min (or the max of a complement), so no result depends on
 * scheduling.
 *
 * Worked example (tests/golden/version_apply_example.json; k@s is user key k,
 * sequence s, type VALUE; a NewFile row is (level, #number, size, smallest ..
 * largest)):
 *   record  scalars                  rows
 *   0       log 3, next 4, seq 10    new (0, #2, 900, a@5..m@1)
 *   1       log 6, next 7, seq 20    new (0, #5, 800, c@15..z@11)
 *   2       next 10, seq 20          pointer (0, z@11); deleted (0,2), (0,5);
 *                                    new (1, #8, 700, m@1..z@11),
 *                                        (1, #7, 1000, a@5..k@12)
 *   3       log 11, next 12, seq 30  new (0, #9, 500, b@25..d@21)
 *   4       -                        deleted (1,8), (3,99);
 *                                    new (2, #8, 700, m@1..z@11)
 *   5       next 13, seq 31          new (0, #12, 400, a@31..a@31),
 *                                        (2, #10, 300, e@3..f@2)
 * gives the files #12, #9 on level 0, #7 on level 1, #10 and #8 on level 2;
 * level_files 2, 1, 2, 0, ...; level_bytes 900, 1000, 1000, 0, ...;
 * compact_pointer[0] = 1; log 11, next 13, last sequence 31, max_file_number
 * 12.  After record 2 alone level 1 is #7 then #8, although #8's row comes
 * first.
 */
#ifndef LVGPU_VERSION_SET_H
#define LVGPU_VERSION_SET_H

#include <stddef.h>
#include <stdint.h>

#include "version.h"
#include "version_edit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LV_VS_UPSTREAM       1u
#define LV_VS_REC_OVER       2u
#define LV_VS_BAD_BOUNDS     4u
#define LV_VS_BAD_ROW        8u
#define LV_VS_DUPLICATE     16u
#define LV_VS_BAD_DIRECTORY 32u
#define LV_VS_FILE_OVER     64u

#define LV_VS_KIND_DIRECTORY 4u          /* bad_kind behind LV_VE_KIND_FILE */
#define LV_VS_MAX_NUMBER (1ull << 56)    /* file numbers lie below it */
#define LV_VS_NO_DIR_INDEX 0xffffffffu

typedef struct lv_vs_placement {         /* 32 bytes, 8-B aligned */
    uint64_t number, file_off, file_cap, reserved;
} lv_vs_placement;

typedef struct lv_vs_totals {            /* device memory, 8-B aligned, always written */
    uint64_t records, new_files, deleted, pointers, live, unplaced;
    uint64_t level_files[LV_NUM_LEVELS], level_bytes[LV_NUM_LEVELS], compact_pointer[LV_NUM_LEVELS];
    uint64_t log_number, prev_log_number, next_file_number, last_sequence;
    uint64_t comparator_off, comparator_len, has, max_file_number;
    uint64_t status, bad_kind, bad_row;
} lv_vs_totals;

typedef struct lv_vs_out {               /* device memory the caller owns */
    lv_version_file *d_files_out;  size_t files_cap;
    uint32_t *d_dir_index;               /* files_cap entries, or NULL */
    lv_vs_totals *d_totals;
} lv_vs_out;

/* 0 when a capacity is beyond what the call accepts. */
size_t lv_version_apply_workspace_bytes(size_t file_cap, size_t deleted_cap, size_t files_cap);
int lv_version_apply_device(const uint8_t *d_src, size_t src_bytes, const lv_ve_encode_in *in,
                            const uint64_t *d_records, const uint64_t *d_upstream_status, size_t rec_cap,
                            const lv_vs_placement *d_dir, size_t dir_n, const lv_vs_out *out, uint32_t flags,
                            void *d_workspace, size_t workspace_bytes, void *stream);

/* The same on the host, serially (no GPU), written as upstream's Builder: per
 * level a set of deleted numbers and a set of added rows under the version's
 * order, Apply over every record, then SaveTo.  The arrays are host memory and
 * `records` is the caller's own count, so UPSTREAM and REC_OVER do not arise;
 * the other bits are judged as above and 0 is returned with the status in
 * *out->d_totals; LV_ERR_INVALID for what the device call refuses (alignment
 * and overlap are not checked). */
int lv_version_apply_host(const uint8_t *src, size_t src_bytes, const lv_ve_encode_in *in, size_t records,
                          const lv_vs_placement *dir, size_t dir_n, const lv_vs_out *out);

#ifdef __cplusplus
}
#endif

#endif /* LVGPU_VERSION_SET_H */
