// lv_version_file_device / lv_version_open_device / lv_version_get_device: the
// boundary keys of an opened image, the validation of a version's descriptor
// and a batched Version::Get over its levels (include/lvgpu/version.h).
//
// The serial algorithm is lvk/version_read.h over lvk/sst_read.h, the text the
// host twins compile too; this file gives it lanes.
//
//   vs_file      one thread: both boundary keys of one image into d_bound_keys
//                behind the device cursor; writes every field of *d_out.
//   vs_init      one thread: every field of *d_version: status UPSTREAM or 0,
//                first_bad = n_files, level_start = n_files (0 with UPSTREAM).
//   vs_validate  one lane per file, uncapped grid (n_files <= 2^20): each
//                judges its file and the pair in front of it whatever the
//                others found.  A lane with bits ORs them into the status,
//                takes first_bad's atomic min with its index and every
//                level_start's with 0; the lane of a level's first file takes
//                level_start's atomic min with its index.  OR and min are
//                order-free.  It reads no field of *d_version.
//   vg_get       one lane per query: level 0's files in order, then one
//                FindFile per level, each visit an lvr::get.  A latency-bound,
//                divergent lookup like sg_get: level 0's descriptors and
//                boundary keys are the same few cache lines for every lane,
//                and the top probes of a level's FindFile are the same
//                addresses for most lanes of the launch, so they are served
//                from L2 / the vector cache after the first wave, not from
//                HBM once per lane.  A lane's state is sg_get's handful
//                of registers plus a file index and the three counters; no key
//                is materialised.
//
// No workspace; the launch shapes depend only on host values (n_files, nq).  No
// workgroup waits on another.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lvgpu/version.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/stage.h"
#include "lvk/version_read.h"

namespace lvk {

constexpr uint32_t kVgThreads = 256;

struct VfArgs {
    const uint8_t *images;
    uint64_t images_bytes, file_off, file_cap;
    const lv_sst_table *table;
    uint64_t number;
    uint32_t level;
    uint8_t *bounds;
    uint64_t bounds_cap;
    uint64_t *used;
    lv_version_file *out;
};

__global__ void vs_file(const VfArgs A) {
    uint64_t used = *A.used;
    lvv::file_fill(A.images, A.images_bytes, A.file_off, A.file_cap, *A.table, A.number, A.level, A.bounds,
                   A.bounds_cap, &used, A.out);
    *A.used = used;
}

struct VoArgs {
    lvv::View v;
    const uint64_t *upstream;
    lv_version_state *version;
};

__global__ void vs_init(const VoArgs A) {
    const bool up = A.upstream && *A.upstream;
    lv_version_state V{};
    V.files = A.v.n_files;
    for (uint32_t l = 0; l <= LV_NUM_LEVELS; ++l) V.level_start[l] = up ? 0 : A.v.n_files;
    V.first_bad = A.v.n_files;
    V.status = up ? LV_VERSION_OPEN_UPSTREAM : 0;
    *A.version = V;
}

__device__ __forceinline__ void vs_min(uint64_t *p, uint64_t v) {
    atomicMin(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v));
}

__global__ __launch_bounds__(kVgThreads) void vs_validate(const VoArgs A) {
    const uint64_t f = static_cast<uint64_t>(blockIdx.x) * kVgThreads + threadIdx.x;
    if (f >= A.v.n_files || (A.upstream && *A.upstream)) return;
    const uint32_t bits = lvv::judge(A.v, f);
    if (bits) {
        atomicOr(reinterpret_cast<unsigned long long *>(&A.version->status), static_cast<unsigned long long>(bits));
        vs_min(&A.version->first_bad, f);
        for (uint32_t l = 0; l <= LV_NUM_LEVELS; ++l) vs_min(&A.version->level_start[l], 0);
        return;
    }
    uint32_t from, to;
    lvv::starts_of(A.v, f, &from, &to);
    for (uint32_t l = from; l < to; ++l) vs_min(&A.version->level_start[l], f);
}

struct VgArgs {
    lvv::View v;
    const lv_version_state *version;
    const uint8_t *qkeys;
    uint64_t qkeys_bytes;
    const uint64_t *q_off;
    const uint32_t *q_len;
    const uint64_t *q_seq;
    uint64_t nq;
    lv_version_get_result *results;
};

__global__ __launch_bounds__(kVgThreads) void vg_get(const VgArgs G) {
    const uint64_t q = static_cast<uint64_t>(blockIdx.x) * kVgThreads + threadIdx.x;
    if (q >= G.nq) return;
    lv_version_get_result r{};
    const uint64_t seq = G.q_seq[q], qo = G.q_off[q];
    const uint32_t ql = G.q_len[q];
    if (!lvv::version_ok(*G.version, G.v.n_files)) {
        r.status = LV_SST_GET_NO_TABLE;
    } else if (seq > LV_MT_MAX_SEQUENCE) {
        r.status = LV_SST_GET_BAD_SEQ;
    } else if (!extent_ok(qo, ql, G.qkeys_bytes)) {
        r.status = LV_SST_GET_BAD_QUERY;
    } else {
        const lvr::Target t{G.qkeys + qo, ql, (seq << 8) | LV_WB_TYPE_VALUE};
        lvv::get(G.v, *G.version, t, &r);
    }
    G.results[q] = r;
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxNq = 0xfffffffeull;

// the checks the open and the get share: the arrays a View is made of
int check_view(uint64_t images_bytes, const lv_version_file *d_files, const lv_sst_table *d_tables, size_t n_files,
               const uint8_t *d_bound_keys, uint64_t bound_keys_bytes, const lv_version_state *d_version, uint32_t flags) {
    (void)images_bytes;
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (n_files > LV_VERSION_MAX_FILES) return set_err(LV_ERR_INVALID, "n_files too large (at most LV_VERSION_MAX_FILES)");
    if (!d_version) return set_err(LV_ERR_INVALID, "null d_version");
    if (misaligned(d_version, 8)) return set_err(LV_ERR_INVALID, "d_version must be 8-byte aligned");
    if (n_files && !d_files) return set_err(LV_ERR_INVALID, "null d_files");
    if (n_files && !d_tables) return set_err(LV_ERR_INVALID, "null d_tables");
    if (misaligned(d_files, 8)) return set_err(LV_ERR_INVALID, "d_files must be 8-byte aligned");
    if (misaligned(d_tables, 8)) return set_err(LV_ERR_INVALID, "d_tables must be 8-byte aligned");
    if (!d_bound_keys && bound_keys_bytes) return set_err(LV_ERR_INVALID, "null d_bound_keys");
    return LV_OK;
}

}  // namespace

extern "C" {

int lv_version_file_device(const uint8_t *d_images, uint64_t images_bytes, uint64_t file_off, uint64_t file_cap,
                           const lv_sst_table *d_table, uint64_t number, uint32_t level, uint8_t *d_bound_keys,
                           uint64_t bound_keys_cap, uint64_t *d_bound_used, lv_version_file *d_out, uint32_t flags,
                           void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (level >= LV_NUM_LEVELS) return set_err(LV_ERR_INVALID, "level must be below LV_NUM_LEVELS");
    if (!d_table) return set_err(LV_ERR_INVALID, "null d_table");
    if (misaligned(d_table, 8)) return set_err(LV_ERR_INVALID, "d_table must be 8-byte aligned");
    if (!d_out) return set_err(LV_ERR_INVALID, "null d_out");
    if (misaligned(d_out, 8)) return set_err(LV_ERR_INVALID, "d_out must be 8-byte aligned");
    if (!d_bound_used) return set_err(LV_ERR_INVALID, "null d_bound_used");
    if (misaligned(d_bound_used, 8)) return set_err(LV_ERR_INVALID, "d_bound_used must be 8-byte aligned");
    if (!d_images && images_bytes) return set_err(LV_ERR_INVALID, "null d_images");
    if (!d_bound_keys && bound_keys_cap) return set_err(LV_ERR_INVALID, "null d_bound_keys");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    lvk::VfArgs A{};
    A.images = d_images;
    A.images_bytes = images_bytes;
    A.file_off = file_off;
    A.file_cap = file_cap;
    A.table = d_table;
    A.number = number;
    A.level = level;
    A.bounds = d_bound_keys;
    A.bounds_cap = bound_keys_cap;
    A.used = d_bound_used;
    A.out = d_out;
    hipLaunchKernelGGL(lvk::vs_file, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), A);
    g_kernel = "vs_file";
    return check_launch();
}

int lv_version_open_device(uint64_t images_bytes, const lv_version_file *d_files, const lv_sst_table *d_tables,
                           size_t n_files, const uint8_t *d_bound_keys, uint64_t bound_keys_bytes,
                           const uint64_t *d_upstream_status, lv_version_state *d_version, uint32_t flags, void *stream) {
    g_err.clear();
    if (int rc = check_view(images_bytes, d_files, d_tables, n_files, d_bound_keys, bound_keys_bytes, d_version, flags))
        return rc;
    if (misaligned(d_upstream_status, 8)) return set_err(LV_ERR_INVALID, "d_upstream_status must be 8-byte aligned");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    lvk::VoArgs A{};
    A.v = lvv::View{nullptr, images_bytes, d_files, d_tables, nullptr, n_files, d_bound_keys, bound_keys_bytes};
    A.upstream = d_upstream_status;
    A.version = d_version;
    hipLaunchKernelGGL(lvk::vs_init, dim3(1), dim3(1), 0, s, A);
    if (n_files) {
        const uint32_t grid = static_cast<uint32_t>((static_cast<uint64_t>(n_files) + lvk::kVgThreads - 1) / lvk::kVgThreads);
        hipLaunchKernelGGL(lvk::vs_validate, dim3(grid), dim3(lvk::kVgThreads), 0, s, A);
    }
    g_kernel = n_files ? "vs_init+vs_validate" : "vs_init";
    return check_launch();
}

int lv_version_get_device(const uint8_t *d_images, uint64_t images_bytes, const lv_version_file *d_files,
                          const lv_sst_table *d_tables, const lv_sst_bloom *d_blooms, size_t n_files,
                          const uint8_t *d_bound_keys, uint64_t bound_keys_bytes, const lv_version_state *d_version,
                          const uint8_t *d_qkeys, size_t qkeys_bytes, const uint64_t *d_q_off, const uint32_t *d_q_len,
                          const uint64_t *d_q_seq, size_t nq, lv_version_get_result *d_results, uint32_t flags,
                          void *stream) {
    g_err.clear();
    if (int rc = check_view(images_bytes, d_files, d_tables, n_files, d_bound_keys, bound_keys_bytes, d_version, flags))
        return rc;
    if (!d_images && images_bytes) return set_err(LV_ERR_INVALID, "null d_images");
    if (misaligned(d_blooms, 8)) return set_err(LV_ERR_INVALID, "d_blooms must be 8-byte aligned");
    if (!d_qkeys && qkeys_bytes) return set_err(LV_ERR_INVALID, "null d_qkeys");
    if (nq > kMaxNq) return set_err(LV_ERR_INVALID, "nq too large for one call (at most 2^32 - 2)");
    if (nq && (!d_q_off || !d_q_len || !d_q_seq)) return set_err(LV_ERR_INVALID, "null query array");
    if (nq && !d_results) return set_err(LV_ERR_INVALID, "null d_results");
    if (misaligned(d_q_off, 8) || misaligned(d_q_seq, 8))
        return set_err(LV_ERR_INVALID, "d_q_off and d_q_seq must be 8-byte aligned");
    if (misaligned(d_q_len, 4)) return set_err(LV_ERR_INVALID, "d_q_len must be 4-byte aligned");
    if (misaligned(d_results, 8)) return set_err(LV_ERR_INVALID, "d_results must be 8-byte aligned");
    if (overlaps(d_results, static_cast<uint64_t>(nq) * sizeof(lv_version_get_result), d_images, images_bytes))
        return set_err(LV_ERR_INVALID, "d_results overlaps d_images");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    if (!nq) return LV_OK;
    lvk::VgArgs G{};
    G.v = lvv::View{d_images, images_bytes, d_files, d_tables, d_blooms, n_files, d_bound_keys, bound_keys_bytes};
    G.version = d_version;
    G.qkeys = d_qkeys;
    G.qkeys_bytes = qkeys_bytes;
    G.q_off = d_q_off;
    G.q_len = d_q_len;
    G.q_seq = d_q_seq;
    G.nq = nq;
    G.results = d_results;
    const uint32_t grid = static_cast<uint32_t>((static_cast<uint64_t>(nq) + lvk::kVgThreads - 1) / lvk::kVgThreads);
    hipLaunchKernelGGL(lvk::vg_get, dim3(grid), dim3(lvk::kVgThreads), 0, static_cast<hipStream_t>(stream), G);
    g_kernel = "vg_get";
    return check_launch();
}

}  // extern "C"
