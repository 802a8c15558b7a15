// Device-resident WAL group-commit encode (the writer side of SURVEY 8f row 2
// with the payload and the log in HBM): lv_wal_encode_device.  The host lays
// the records out (wal_layout.cc), uploads the fragment table, the offsets API
// checksums the fragments in place in the payload, and wal_frame_kernel below
// writes the log: 7-byte headers, payload, zero trailers (log_writer.rs:62-134).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/wal.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/wal.h"

namespace lvk {

// ---------------------------------------------------------------------------
// wal_frame_kernel: organised by output bytes.  The output is cut into the
// 16-byte granules of its own address alignment (granule g holds the output
// positions [16 g - a, 16 g - a + 16), a = d_out % 16); a workgroup takes one
// 32 KiB log block of the appended span at a time and owns the granules whose
// first byte lies in it, one granule per lane per step.  The block's fragment
// positions go to LDS once (16 bits each: they are relative to the block), so
// a lane finds the fragment under its granule with a binary search that never
// leaves the CU.  A granule wholly inside one fragment's payload is one
// unaligned 16-B load and one aligned 16-B store; any other granule (a header,
// a trailer, a fragment boundary, an end of the output) is composed byte by
// byte, walking the fragment table forward, and stored whole when all its 16
// bytes are output bytes, else byte by byte.  Work per lane follows the
// output bytes: 20,000 one-byte records and one 4 MiB record balance alike.
constexpr uint32_t kFrameThreads = 256;
constexpr uint64_t kFramePosMask = (1ull << 56) - 1;  // pos words: out_pos | type << 56

struct FrameArgs {
    const uint8_t *payload;
    uint8_t *out;
    uint64_t out_len;
    uint32_t first;      // dest_length % 32768: block k starts at output position k * 32768 - first
    uint32_t align;      // d_out % 16
    uint64_t nblocks;
    uint64_t nfrags;
    const uint64_t *src;   // payload offset of each fragment
    const uint64_t *pos;   // header position in the output | type << 56
    const uint32_t *len;
    const uint32_t *crc;   // masked CRC of each fragment (the CRC step's output)
    const uint32_t *bidx;  // first fragment of each block, nblocks + 1 entries
};

// One fragment's header fields and the position of the next header.
struct FrameFrag {
    uint64_t pos, src, next;
    uint32_t len, crc, type;
};

__device__ __forceinline__ void frame_load(const FrameArgs &A, int64_t f, FrameFrag *r) {
    const uint64_t pw = A.pos[f];
    r->pos = pw & kFramePosMask;
    r->type = static_cast<uint32_t>(pw >> 56);
    r->src = A.src[f];
    r->len = A.len[f];
    r->crc = A.crc[f];
    r->next = static_cast<uint64_t>(f + 1) < A.nfrags ? (A.pos[f + 1] & kFramePosMask) : ~0ull;
}

// The granule at output positions [p0, p0 + 16) composed byte by byte; f is
// the last fragment whose header is at or before max(p0, 0) (-1: none).
__device__ __forceinline__ void frame_compose(const FrameArgs &A, int64_t p0, int64_t f) {
    FrameFrag r{};
    if (f >= 0)
        frame_load(A, f, &r);
    else
        r.next = A.nfrags ? (A.pos[0] & kFramePosMask) : ~0ull;
    uint64_t lo = 0, hi = 0;
    uint32_t valid = 0;
    for (uint32_t k = 0; k < 16; ++k) {
        const int64_t p = p0 + k;
        if (p < 0 || static_cast<uint64_t>(p) >= A.out_len) continue;
        valid |= 1u << k;
        while (static_cast<uint64_t>(p) >= r.next) frame_load(A, ++f, &r);
        uint32_t b = 0;
        if (f >= 0) {
            const uint64_t d = static_cast<uint64_t>(p) - r.pos;
            if (d < 4)
                b = (r.crc >> (8 * d)) & 0xffu;  // log_writer.rs:117-125
            else if (d < 6)
                b = (r.len >> (8 * (d - 4))) & 0xffu;
            else if (d == 6)
                b = r.type;
            else if (d < kWalHeader + r.len)
                b = A.payload[r.src + d - kWalHeader];
            // else: the block's zero trailer
        }
        if (k < 8)
            lo |= static_cast<uint64_t>(b) << (8 * k);
        else
            hi |= static_cast<uint64_t>(b) << (8 * (k - 8));
    }
    granule_store(A.out + p0, lo, hi, valid);  // 16-B aligned by construction (only dereferenced at valid bytes)
}

__global__ __launch_bounds__(kFrameThreads) void wal_frame_kernel(const FrameArgs A) {
    __shared__ uint16_t s_pos[kWalMaxFrags];
    const uint32_t tid = threadIdx.x;
    for (uint64_t blk = blockIdx.x; blk < A.nblocks; blk += gridDim.x) {
        // output positions of this block: [lo, hi)
        const uint64_t lo = blk == 0 ? 0 : blk * kWalBlock - A.first;
        const uint64_t end = (blk + 1) * kWalBlock - A.first;
        const uint64_t hi = end < A.out_len ? end : A.out_len;
        const uint32_t f0 = A.bidx[blk];
        const uint32_t cnt = A.bidx[blk + 1] - f0;
        const uint32_t nf = cnt < kWalMaxFrags ? cnt : kWalMaxFrags;
        __syncthreads();  // the previous block's searches are done
        for (uint32_t i = tid; i < nf; i += kFrameThreads)
            s_pos[i] = static_cast<uint16_t>((A.pos[f0 + i] & kFramePosMask) - lo);
        __syncthreads();
        // granules whose first output byte lies in [lo, hi)
        const uint64_t g_lo = blk == 0 ? 0 : (lo + A.align + 15) / 16;
        const uint64_t g_hi = (hi + A.align + 15) / 16;
        for (uint64_t g = g_lo + tid; g < g_hi; g += kFrameThreads) {
            const int64_t p0 = static_cast<int64_t>(g * 16) - static_cast<int64_t>(A.align);
            const uint32_t rel = static_cast<uint32_t>((p0 < 0 ? 0 : p0) - static_cast<int64_t>(lo));
            // the last fragment of the block with s_pos <= rel is the one before a
            const uint32_t a = count_le(s_pos, nf, rel);
            const int64_t f = static_cast<int64_t>(f0) + a - 1;  // (block 0 before its first header: f0 - 1 = -1)
            if (a > 0 && p0 >= 0) {
                const uint32_t d = rel - s_pos[a - 1];
                const uint32_t len = A.len[f];
                if (d >= kWalHeader && d + 16 <= kWalHeader + len) {
                    u32x4 v;
                    __builtin_memcpy(&v, A.payload + A.src[f] + (d - kWalHeader), 16);
                    *reinterpret_cast<u32x4 *>(A.out + p0) = v;
                    continue;
                }
            }
            frame_compose(A, p0, a > 0 ? f : static_cast<int64_t>(f0) - 1);
        }
    }
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxFragments = 0xffffffffull;  // one lv_crc32c_batch_device call (32-bit buffer indices)

// Workspace: the fragment table (the upload image, one copy), the CRCs, then
// the offsets API's sort workspace.
// It is carved three times: without a buffer to measure, over the caller's
// workspace, and over the pinned staging slot the table is written in (only
// the first `image` bytes of that one exist).
struct EncTab {
    uint64_t *src, *pos;
    uint32_t *len, *seed, *bidx, *crc;
    size_t image;   // bytes the upload covers
    uint8_t *sort;  // the rest, for lv_crc32c_batch_device_hint
};
void enc_carve(Carve &C, uint64_t fragments, EncTab &T) {
    T.src = C.take<uint64_t>(fragments);
    T.pos = C.take<uint64_t>(fragments);
    T.len = C.take<uint32_t>(fragments);
    T.seed = C.take<uint32_t>(fragments);
    // every block of the span but the first starts with a header: at most
    // fragments + 1 blocks, plus the closing entry
    T.bidx = C.take<uint32_t>(fragments + 2);
    T.crc = C.take<uint32_t>(fragments);
    T.image = C.at;
    T.sort = C.take<uint8_t>(lv_crc32c_workspace_bytes(fragments));
}

// Page-locked staging for the table upload.  A slot is busy until the event
// recorded behind its copy has completed, so a second call enqueued before the
// first one's copy has run (on the same stream or another) takes another slot.
struct StageSlot {
    uint8_t *p = nullptr;
    size_t cap = 0;
    int dev = -1;
    hipEvent_t done = nullptr;
    bool used = false;     // `done` was recorded at least once
    bool retired = false;  // a copy was enqueued that no event follows: never handed out again
};
std::mutex g_stage_m;
std::vector<StageSlot> *g_stage = nullptr;  // never destroyed: no HIP calls at exit

int stage_acquire(int dev, size_t need, size_t *slot) {
    if (!g_stage) g_stage = new std::vector<StageSlot>();
    std::vector<StageSlot> &v = *g_stage;
    for (size_t i = 0; i < v.size(); ++i) {
        if (v[i].dev != dev || v[i].cap < need || v[i].retired) continue;
        if (v[i].used && hipEventQuery(v[i].done) != hipSuccess) {
            (void)hipGetLastError();  // hipErrorNotReady is not an error here
            continue;
        }
        *slot = i;
        return LV_OK;
    }
    StageSlot s;
    s.dev = dev;
    s.cap = std::max<size_t>(need, size_t{1} << 16);
    LV_HIP(hipHostMalloc(reinterpret_cast<void **>(&s.p), s.cap, hipHostMallocDefault));
    LV_HIP(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    v.push_back(s);
    *slot = v.size() - 1;
    return LV_OK;
}

}  // namespace

// wal_frame_kernel: a workgroup takes one 32 KiB log block a trip.
uint64_t lvgpu_internal::wal_frame_grid(uint64_t blocks, uint64_t cus, uint64_t *per_trip) {
    if (per_trip) *per_trip = 1;
    return std::min<uint64_t>(blocks, 8 * cus);
}

extern "C" {

size_t lv_wal_encode_workspace_bytes(size_t fragments) {
    EncTab T;
    Carve C{nullptr};
    enc_carve(C, fragments, T);
    return C.at;
}

int lv_wal_encode_device(const uint8_t *d_payload, uint64_t payload_bytes, const uint64_t *rec_off,
                         const uint64_t *rec_len, size_t n, uint64_t dest_length, uint8_t *d_out, size_t out_cap,
                         size_t *out_len, void *d_workspace, size_t workspace_bytes, void *stream) {
    g_err.clear();
    if (!out_len) return set_err(LV_ERR_INVALID, "null out_len");
    *out_len = 0;
    if (n && (!rec_off || !rec_len)) return set_err(LV_ERR_INVALID, "null record array");
    if (n && !d_payload && payload_bytes) return set_err(LV_ERR_INVALID, "null payload pointer");
    // (a record of L bytes makes at most L / 32761 + 2 fragments)
    uint64_t frag_bound = 0;
    for (size_t i = 0; i < n; ++i) {
        if (rec_off[i] + rec_len[i] < rec_off[i] || rec_off[i] + rec_len[i] > payload_bytes)
            return set_err(LV_ERR_INVALID, "record " + std::to_string(i) + " exceeds the payload");
        frag_bound += rec_len[i] / (LV_WAL_BLOCK_SIZE - LV_WAL_HEADER_SIZE) + 2;
    }
    // A batch that may exceed the fragment limit is counted first (no table),
    // so that it is refused before a table of that size is built; any other
    // batch is laid out once.
    lvgpu_internal::WalLayout lay;
    const bool count_first = frag_bound > kMaxFragments;
    lvgpu_internal::wal_layout(rec_off, rec_len, n, dest_length, !count_first, &lay);
    *out_len = static_cast<size_t>(lay.out_len);
    if (lay.fragments > kMaxFragments) return set_err(LV_ERR_INVALID, "more than 2^32-1 fragments per call");
    if (out_cap < lay.out_len || (!d_out && lay.out_len)) return set_err(LV_ERR_INVALID, "output buffer too small");
    if (lay.out_len == 0) return LV_OK;  // no records: nothing to enqueue
    if (!d_workspace) return set_err(LV_ERR_INVALID, "null workspace");
    if (misaligned(d_workspace, 16)) return set_err(LV_ERR_INVALID, "workspace must be 16-byte aligned");
    const uint64_t F = lay.fragments;
    EncTab D;  // the table on the device
    Carve C{static_cast<uint8_t *>(d_workspace)};
    enc_carve(C, F, D);
    if (workspace_bytes < C.at) return set_err(LV_ERR_INVALID, "workspace too small");
    if (overlaps(d_out, lay.out_len, d_payload, payload_bytes))
        return set_err(LV_ERR_INVALID, "d_out overlaps d_payload");
    if (count_first) lvgpu_internal::wal_layout(rec_off, rec_len, n, dest_length, true, &lay);
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    // Step a: the fragment table, through staging the library owns.
    uint32_t type_crc[5], type_masked[5];
    for (uint8_t t = 0; t < 5; ++t) {
        type_crc[t] = lv_crc32c_value(&t, 1);  // log_writer.rs:136-142
        type_masked[t] = lv_crc32c_mask(type_crc[t]);
    }
    uint64_t total = 0;
    uint32_t max_len = 0;
    {
        std::lock_guard<std::mutex> lk(g_stage_m);
        size_t slot = 0;
        if (int rc = stage_acquire(c->dev, D.image, &slot)) return rc;
        StageSlot &st = (*g_stage)[slot];
        EncTab H;  // its image in the slot
        Carve S{st.p};
        enc_carve(S, F, H);
        for (uint64_t i = 0; i < F; ++i) {
            const lvgpu_internal::WalFrag &f = lay.frags[i];
            H.src[i] = f.src;
            H.pos[i] = f.out_pos | (static_cast<uint64_t>(f.type) << 56);
            H.len[i] = f.len;
            H.seed[i] = type_crc[f.type];
            H.crc[i] = type_masked[f.type];  // the CRC of an empty fragment (step a overwrites it)
            total += f.len;
            max_len = std::max(max_len, f.len);
        }
        for (size_t k = 0; k < lay.block_first.size(); ++k) H.bidx[k] = static_cast<uint32_t>(lay.block_first[k]);
        LV_HIP(hipMemcpyAsync(d_workspace, st.p, D.image, hipMemcpyHostToDevice, s));
        const hipError_t e = hipEventRecord(st.done, s);
        if (e != hipSuccess) {
            st.retired = true;  // the copy may still be reading the slot and nothing tells when it ends
            return set_err(static_cast<int>(e), std::string("hipEventRecord: ") + hipGetErrorString(e));
        }
        st.used = true;
    }
    // A batch with no payload bytes (every record empty) has nothing to
    // checksum, and possibly no payload buffer: the uploaded CRCs stand.
    const lv_batch_hint hint{total, max_len, 0};
    if (total)
        if (int rc = lv_crc32c_batch_device_hint(d_payload, D.src, D.len, D.seed, D.crc, F, LV_CRC_MASK, &hint, D.sort,
                                                 workspace_bytes - D.image, stream))
            return rc;

    // Step b: the log bytes.
    lvk::FrameArgs A{};
    A.payload = d_payload;
    A.out = d_out;
    A.out_len = lay.out_len;
    A.first = static_cast<uint32_t>(dest_length % LV_WAL_BLOCK_SIZE);
    A.align = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(d_out) % 16);
    A.nblocks = lay.block_first.size() - 1;
    A.nfrags = F;
    A.src = D.src;
    A.pos = D.pos;
    A.len = D.len;
    A.crc = D.crc;
    A.bidx = D.bidx;
    const uint32_t grid = static_cast<uint32_t>(lvgpu_internal::wal_frame_grid(A.nblocks, static_cast<uint64_t>(c->cus)));
    hipLaunchKernelGGL(lvk::wal_frame_kernel, dim3(grid), dim3(lvk::kFrameThreads), 0, s, A);
    return check_launch();
}

}  // extern "C"
