// What the host twin of the table build (sst_build.cc) lends the host twin of
// the compaction output (compact_output.cc): its TableBuilder walk with
// upstream's MaxOutputFileSize check.  Host only; not part of the C ABI.
#pragma once
#include <cstdint>

#include "../../include/lvgpu/table.h"

namespace lvgpu_host {

// A fresh TableBuilder (with bpk != 0 a fresh FilterBlockBuilder too) fed
// ops[order[0]], ops[order[1]], ... : it stops after the add that brought the
// flushed bytes (the sum of raw + 5 over the data blocks written) to
// max_file_bytes or more, or after entry n - 1, and finishes the table.
// Returns the entries added.  One walk: file == NULL sizes only; otherwise
// the image goes to file[0, totals->file_bytes) and its handle pairs to
// handles, with the index block at index_offset, which a sizing call over the
// same input reported (as did its status: a file with BLOCK_LARGE is not
// written).  The extents of the entries are the caller's to check.
uint64_t sst_build_prefix(const uint8_t *payload, const lv_wb_op *ops, const uint32_t *order, uint64_t n,
                          uint64_t block_size, uint64_t restart_interval, uint32_t bpk, uint64_t max_file_bytes,
                          uint8_t *file, uint64_t index_offset, uint64_t *handles, lv_sst_build_totals *totals,
                          lv_sst_bloom_totals *bloom_totals);

}  // namespace lvgpu_host
