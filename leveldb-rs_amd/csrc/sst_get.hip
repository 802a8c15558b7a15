// lv_sst_open_device / lv_sst_get_device: Table::Open and a batched
// Table::InternalGet + SaveValue over an SSTable image in HBM
// (include/lvgpu/table.h, "Open" and "Get").
//
// The serial algorithm is lvk/sst_read.h, the text the host twins compile too;
// this file gives it lanes.
//
//   so_header    one thread: the upstream status, *d_file_bytes against
//                file_cap, the footer, the index block's type byte and header;
//                writes every field of *d_table.  data_blocks != 0 exactly
//                when the restarts are to be judged.
//   so_validate  one lane per index restart in a grid-stride loop: each judges
//                its own run whatever the others found, and a lane with bits
//                ORs them into d_table->status (a vector atomic).  It reads
//                the fields so_header wrote, never the status.
//   so_emit      (d_handles != NULL) status 0: one lane per handle decodes its
//                restart's handle again and writes the pair; the metaindex and
//                index pairs follow.  Status 0 implies data_blocks <=
//                block_cap, so every store lies in the caller's array.
//   sg_get       one lane per query: the index seek, the block seek and
//                SaveValue.  Its state is a handful of registers whatever the
//                key lengths; a wave's lanes diverge where their blocks do.
//                sg_get<true> (lv_sst_get_bloom_device) asks the filter of
//                *d_bloom between the two seeks.
//   so_bloom     (lv_sst_bloom_open_device) one thread: Table::ReadMeta and
//                ReadFilter; writes every field of *d_bloom.
//
// No workspace; the launch sequences depend only on host values (block_cap,
// file_cap, whether d_handles is NULL; nq).  No workgroup waits on another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/table.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/sst_read.h"
#include "lvk/stage.h"

namespace lvk {

constexpr uint32_t kSgThreads = 256;
constexpr uint32_t kSoMaxGrid = 2048;  // validate / emit: the rest is the grid-stride loop's

struct SoArgs {
    const uint8_t *file;
    uint64_t file_cap;
    const uint64_t *file_bytes, *upstream;
    uint64_t *handles;
    uint64_t block_cap;
    lv_sst_table *table;
};

__global__ void so_header(const SoArgs A) {
    lv_sst_table t{};
    if (A.upstream && *A.upstream) {
        t.status = LV_SST_OPEN_UPSTREAM;
    } else if (const uint64_t fb = *A.file_bytes) {
        if (fb > A.file_cap) {
            t.file_bytes = fb;
            t.status = LV_SST_OPEN_NOT_A_TABLE;
        } else {
            lvr::open_header(A.file, fb, &t);
        }
        if (A.handles && t.data_blocks > A.block_cap) t.status |= LV_SST_OPEN_HANDLE_OVER;
    }
    *A.table = t;
}

// the fields a restart's judgement reads (not the status: lanes are writing it)
__device__ __forceinline__ lv_sst_table so_fields(const lv_sst_table *p) {
    lv_sst_table t{};
    t.file_bytes = p->file_bytes;
    t.index_offset = p->index_offset;
    t.index_size = p->index_size;
    t.data_blocks = p->data_blocks;
    return t;
}

__global__ __launch_bounds__(kSgThreads) void so_validate(const SoArgs A) {
    const lv_sst_table t = so_fields(A.table);
    const uint64_t step = static_cast<uint64_t>(gridDim.x) * kSgThreads;
    uint32_t bits = 0;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSgThreads + threadIdx.x; i < t.data_blocks; i += step) {
        uint64_t off, size;
        bits |= lvr::open_restart(A.file, t, i, &off, &size);
    }
    if (bits) atomicOr(reinterpret_cast<unsigned long long *>(&A.table->status), static_cast<unsigned long long>(bits));
}

__global__ __launch_bounds__(kSgThreads) void so_emit(const SoArgs A) {
    if (A.table->status || !A.table->file_bytes) return;  // nobody writes the status during this launch
    const lv_sst_table t = *A.table;
    const uint64_t n = t.data_blocks, step = static_cast<uint64_t>(gridDim.x) * kSgThreads;
    if (n > A.block_cap) return;  // (status 0 says so already)
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSgThreads + threadIdx.x; i < n + 2; i += step) {
        uint64_t off = i == n ? t.metaindex_offset : t.index_offset, size = i == n ? t.metaindex_size : t.index_size;
        if (i < n) lvr::open_restart(A.file, t, i, &off, &size);
        A.handles[2 * i] = off;
        A.handles[2 * i + 1] = size;
    }
}

struct SgArgs {
    const uint8_t *file;
    uint64_t file_cap;
    const lv_sst_table *table;
    const uint8_t *qkeys;
    uint64_t qkeys_bytes;
    const uint64_t *q_off;
    const uint32_t *q_len;
    const uint64_t *q_seq;
    uint64_t nq;
    lv_sst_get_result *results;
    const lv_sst_bloom *bloom;  // sg_get<true>: lv_sst_get_bloom_device
};

// kBloom: the filter *G.bloom is asked before a data block is touched (when it
// says present; lvr::may_match checks its offsets against the file again).
template <bool kBloom>
__global__ __launch_bounds__(kSgThreads) void sg_get(const SgArgs G) {
    const uint64_t q = static_cast<uint64_t>(blockIdx.x) * kSgThreads + threadIdx.x;
    if (q >= G.nq) return;
    lv_sst_get_result r{};
    const uint64_t fb = G.table->file_bytes, seq = G.q_seq[q], qo = G.q_off[q];
    const uint32_t ql = G.q_len[q];
    if (G.table->status || fb > G.file_cap) {
        r.status = LV_SST_GET_NO_TABLE;
    } else if (seq > LV_MT_MAX_SEQUENCE) {
        r.status = LV_SST_GET_BAD_SEQ;
    } else if (!extent_ok(qo, ql, G.qkeys_bytes)) {
        r.status = LV_SST_GET_BAD_QUERY;
    } else {
        const lvr::Target t{G.qkeys + qo, ql, (seq << 8) | LV_WB_TYPE_VALUE};
        if constexpr (kBloom) {
            const lv_sst_bloom b = *G.bloom;
            r.status = lvr::get(G.file, fb, G.table->index_offset, G.table->index_size, t, &r,
                                b.present == 1 ? &b : nullptr);
        } else {
            r.status = lvr::get(G.file, fb, G.table->index_offset, G.table->index_size, t, &r);
        }
    }
    G.results[q] = r;
}

// lv_sst_bloom_open_device: one thread, Table::ReadMeta / ReadFilter.
__global__ void so_bloom(const uint8_t *file, uint64_t file_cap, const lv_sst_table *table, lv_sst_bloom *bloom) {
    lv_sst_bloom b{};
    const uint64_t fb = table->file_bytes;
    if (table->status || fb > file_cap)
        b.why = LV_SST_BLOOM_TABLE;
    else if (!fb)
        b.why = LV_SST_BLOOM_EMPTY;
    else
        lvr::bloom_open(file, fb, table->metaindex_offset, table->metaindex_size, &b);
    *bloom = b;
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxNq = 0xfffffffeull;
constexpr uint64_t kMaxBlockCap = 0xfffffffcull;

}  // namespace

// so_validate / so_emit: a lane per restart array or handle, kSgThreads a workgroup trip.
uint64_t lvgpu_internal::so_grid(uint64_t lanes, uint64_t *per_trip) {
    if (per_trip) *per_trip = lvk::kSgThreads;
    return std::min<uint64_t>((lanes + lvk::kSgThreads - 1) / lvk::kSgThreads, lvk::kSoMaxGrid);
}

extern "C" {

int lv_sst_open_device(const uint8_t *d_file, uint64_t file_cap, const uint64_t *d_file_bytes,
                       const uint64_t *d_upstream_status, uint64_t *d_handles, size_t block_cap,
                       lv_sst_table *d_table, uint32_t flags, void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (!d_table) return set_err(LV_ERR_INVALID, "null d_table");
    if (misaligned(d_table, 8)) return set_err(LV_ERR_INVALID, "d_table must be 8-byte aligned");
    if (!d_file_bytes) return set_err(LV_ERR_INVALID, "null d_file_bytes");
    if (misaligned(d_file_bytes, 8)) return set_err(LV_ERR_INVALID, "d_file_bytes must be 8-byte aligned");
    if (misaligned(d_upstream_status, 8)) return set_err(LV_ERR_INVALID, "d_upstream_status must be 8-byte aligned");
    if (!d_file && file_cap) return set_err(LV_ERR_INVALID, "null d_file");
    if (block_cap > kMaxBlockCap) return set_err(LV_ERR_INVALID, "block_cap too large (at most 2^32 - 4)");
    if (!d_handles && block_cap) return set_err(LV_ERR_INVALID, "null d_handles");
    if (misaligned(d_handles, 8)) return set_err(LV_ERR_INVALID, "d_handles must be 8-byte aligned");
    if (d_handles && overlaps(d_handles, 16 * (static_cast<uint64_t>(block_cap) + 2), d_file, file_cap))
        return set_err(LV_ERR_INVALID, "d_handles overlaps d_file");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    lvk::SoArgs A{};
    A.file = d_file;
    A.file_cap = file_cap;
    A.file_bytes = d_file_bytes;
    A.upstream = d_upstream_status;
    A.handles = d_handles;
    A.block_cap = block_cap;
    A.table = d_table;
    // a lane per restart the caller expects; with no handle array, per 4 KiB of the buffer
    const uint64_t lanes = (block_cap ? static_cast<uint64_t>(block_cap) : file_cap / LV_SST_DEFAULT_BLOCK_SIZE) + 2;
    const uint32_t grid = static_cast<uint32_t>(lvgpu_internal::so_grid(lanes));
    hipLaunchKernelGGL(lvk::so_header, dim3(1), dim3(1), 0, s, A);
    hipLaunchKernelGGL(lvk::so_validate, dim3(grid), dim3(lvk::kSgThreads), 0, s, A);
    if (d_handles) hipLaunchKernelGGL(lvk::so_emit, dim3(grid), dim3(lvk::kSgThreads), 0, s, A);
    g_kernel = d_handles ? "so_header+so_validate+so_emit" : "so_header+so_validate";
    return check_launch();
}

}  // extern "C"

namespace {

// lv_sst_get_device (d_bloom == NULL, bloom false) and lv_sst_get_bloom_device.
int sg_launch(const uint8_t *d_file, uint64_t file_cap, const lv_sst_table *d_table, const lv_sst_bloom *d_bloom,
              bool bloom, const uint8_t *d_qkeys, size_t qkeys_bytes, const uint64_t *d_q_off, const uint32_t *d_q_len,
              const uint64_t *d_q_seq, size_t nq, lv_sst_get_result *d_results, uint32_t flags, void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (!d_table) return set_err(LV_ERR_INVALID, "null d_table");
    if (misaligned(d_table, 8)) return set_err(LV_ERR_INVALID, "d_table must be 8-byte aligned");
    if (bloom && !d_bloom) return set_err(LV_ERR_INVALID, "null d_bloom");
    if (misaligned(d_bloom, 8)) return set_err(LV_ERR_INVALID, "d_bloom must be 8-byte aligned");
    if (!d_file && file_cap) return set_err(LV_ERR_INVALID, "null d_file");
    if (!d_qkeys && qkeys_bytes) return set_err(LV_ERR_INVALID, "null d_qkeys");
    if (nq > kMaxNq) return set_err(LV_ERR_INVALID, "nq too large for one call (at most 2^32 - 2)");
    if (nq && (!d_q_off || !d_q_len || !d_q_seq)) return set_err(LV_ERR_INVALID, "null query array");
    if (nq && !d_results) return set_err(LV_ERR_INVALID, "null d_results");
    if (misaligned(d_q_off, 8) || misaligned(d_q_seq, 8))
        return set_err(LV_ERR_INVALID, "d_q_off and d_q_seq must be 8-byte aligned");
    if (misaligned(d_q_len, 4)) return set_err(LV_ERR_INVALID, "d_q_len must be 4-byte aligned");
    if (misaligned(d_results, 8)) return set_err(LV_ERR_INVALID, "d_results must be 8-byte aligned");
    if (overlaps(d_results, static_cast<uint64_t>(nq) * sizeof(lv_sst_get_result), d_file, file_cap))
        return set_err(LV_ERR_INVALID, "d_results overlaps d_file");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    if (!nq) return LV_OK;
    lvk::SgArgs G{};
    G.file = d_file;
    G.file_cap = file_cap;
    G.table = d_table;
    G.qkeys = d_qkeys;
    G.qkeys_bytes = qkeys_bytes;
    G.q_off = d_q_off;
    G.q_len = d_q_len;
    G.q_seq = d_q_seq;
    G.nq = nq;
    G.results = d_results;
    G.bloom = d_bloom;
    const uint32_t grid = static_cast<uint32_t>((static_cast<uint64_t>(nq) + lvk::kSgThreads - 1) / lvk::kSgThreads);
    if (bloom)
        hipLaunchKernelGGL(lvk::sg_get<true>, dim3(grid), dim3(lvk::kSgThreads), 0, static_cast<hipStream_t>(stream), G);
    else
        hipLaunchKernelGGL(lvk::sg_get<false>, dim3(grid), dim3(lvk::kSgThreads), 0, static_cast<hipStream_t>(stream), G);
    g_kernel = bloom ? "sg_get<bloom>" : "sg_get";
    return check_launch();
}

}  // namespace

extern "C" {

int lv_sst_get_device(const uint8_t *d_file, uint64_t file_cap, const lv_sst_table *d_table, const uint8_t *d_qkeys,
                      size_t qkeys_bytes, const uint64_t *d_q_off, const uint32_t *d_q_len, const uint64_t *d_q_seq,
                      size_t nq, lv_sst_get_result *d_results, uint32_t flags, void *stream) {
    return sg_launch(d_file, file_cap, d_table, nullptr, false, d_qkeys, qkeys_bytes, d_q_off, d_q_len, d_q_seq, nq,
                     d_results, flags, stream);
}

int lv_sst_get_bloom_device(const uint8_t *d_file, uint64_t file_cap, const lv_sst_table *d_table,
                            const lv_sst_bloom *d_bloom, const uint8_t *d_qkeys, size_t qkeys_bytes,
                            const uint64_t *d_q_off, const uint32_t *d_q_len, const uint64_t *d_q_seq, size_t nq,
                            lv_sst_get_result *d_results, uint32_t flags, void *stream) {
    return sg_launch(d_file, file_cap, d_table, d_bloom, true, d_qkeys, qkeys_bytes, d_q_off, d_q_len, d_q_seq, nq,
                     d_results, flags, stream);
}

int lv_sst_bloom_open_device(const uint8_t *d_file, uint64_t file_cap, const lv_sst_table *d_table,
                             lv_sst_bloom *d_bloom, uint32_t flags, void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (!d_table) return set_err(LV_ERR_INVALID, "null d_table");
    if (misaligned(d_table, 8)) return set_err(LV_ERR_INVALID, "d_table must be 8-byte aligned");
    if (!d_bloom) return set_err(LV_ERR_INVALID, "null d_bloom");
    if (misaligned(d_bloom, 8)) return set_err(LV_ERR_INVALID, "d_bloom must be 8-byte aligned");
    if (!d_file && file_cap) return set_err(LV_ERR_INVALID, "null d_file");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipLaunchKernelGGL(lvk::so_bloom, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), d_file, file_cap, d_table,
                       d_bloom);
    g_kernel = "so_bloom";
    return check_launch();
}

}  // extern "C"
