// lv_write_batch_decode_device: WriteBatch::iterate (write_batch.rs:92-122)
// over the logical records lv_wal_decode_device left in HBM, to a flat,
// log-ordered op table.  The format is sequential inside a record and
// independent across records, so the call is three stages:
//
//   wb_count   every record is walked once: its emitted op count and status,
//              the sums for the totals, each tile's op count.
//   wb_tiles   (one workgroup) the exclusive scan of the tile counts, the
//              totals and the status.
//   wb_emit    every record with ops is walked again and its ops are written
//              at its base (tile base + the scan inside the tile).
//
// Count and emit share one walk (wb_walk), templated on the byte source and on
// what is done with an op.  Two record classes use it, chosen per record on
// the device by d_rec_len:
//
//   small (<= kWbSmall bytes): one lane per record.  Neighbouring lanes own
//   neighbouring records, which lie next to each other in d_payload; a lane
//   reads the aligned 16-B granule under the byte it needs into registers.
//
//   large: one wave per record, through an LDS window of kWbWindow bytes the
//   wave loads with coalesced 16-B loads.  The walk runs wave-uniformly over
//   the window (all lanes read the same LDS address: a broadcast); lane k % 64
//   keeps op k in registers and every 64 ops the wave stores them together.
//   When the parser needs a byte outside the window, the next window starts at
//   that byte's granule: keys and values are skipped, not read.
//
// A wave takes 64 consecutive records at a time: each lane walks its own if it
// is small, then the wave walks the large ones among them one after another.
// All position arithmetic is u64.  The two byte sources, the varint read, a
// record's class and the wave's dispatch are lvk/records.h's (LaneSrc,
// WaveSrc, varint32, record_class, dispatch), which version_edit.hip's decode
// uses too; the wave reductions are lvk/stage.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/write_batch.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/records.h"

namespace lvk {

constexpr uint32_t kWbThreads = 256;
constexpr uint32_t kWbPer = 1;                        // records per thread of a scan tile
constexpr uint32_t kWbTile = kWbThreads * kWbPer;     // records per scan tile
constexpr uint32_t kWbWaves = kWbThreads / 64;
constexpr uint32_t kWbChunks = kWbTile / 64;          // 64-record chunks of a tile
constexpr uint32_t kWbSmall = 16384;                  // records up to this many bytes: one lane each
constexpr uint32_t kWbWindow = 4096;                  // LDS window of a wave-class record, bytes
constexpr uint32_t kWbRound = 64 * 16;                // one load of the wave: 64 lanes x 16 B
constexpr uint32_t kWbScanThreads = 1024;             // wb_tiles' one workgroup
static_assert(kWbSmall >= LV_WB_HEADER_SIZE, "the lane class takes whole headers");

// What the count pass keeps of the whole batch (workspace, zeroed by
// wb_init), and what wb_tiles adds for wb_emit.
struct WbHead {
    unsigned long long key_bytes, val_bytes, bad, last_seq;
    uint64_t n, status, pad[2];
};

struct WbArgs {
    const uint8_t *payload;
    uint64_t payload_bytes;
    const uint64_t *rec_off, *rec_len, *records, *upstream;
    uint64_t rec_cap;
    lv_wb_decode_out out;
    // workspace
    WbHead *head;
    uint64_t *cnt;     // ops of each record
    uint32_t *st;      // status of each record
    uint64_t *tsum;    // ops of each tile, then (wb_tiles) the ops before it
};

// ---- op sinks -------------------------------------------------------------
struct WbNoSink {
    __device__ __forceinline__ void put(uint64_t, uint64_t, uint64_t, uint64_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void finish(uint64_t) {}
};

// One lane: op k of the record goes straight to d_ops[base + k].
struct WbLaneSink {
    lv_wb_op *ops;
    uint64_t base, cap;
    __device__ __forceinline__ void put(uint64_t k, uint64_t tag, uint64_t koff, uint64_t voff, uint32_t klen,
                                        uint32_t vlen) {
        const uint64_t at = base + k;
        if (at < cap) store_op(ops + at, lv_wb_op{tag, koff, voff, klen, vlen});  // (the status said it fits)
    }
    __device__ __forceinline__ void finish(uint64_t) {}
};

// One wave: lane k % 64 keeps op k; after every 64th op, and at the end, the
// lanes store what they hold -- 64 consecutive 32-B entries, in 16-B stores.
struct WbWaveSink {
    lv_wb_op *ops;
    uint64_t base, cap;
    uint32_t lane;
    uint64_t tag, koff, voff;
    uint32_t klen, vlen;
    __device__ __forceinline__ void flush(uint64_t first, uint32_t count) {
        const uint64_t at = base + first + lane;
        if (lane < count && at < cap) store_op(ops + at, lv_wb_op{tag, koff, voff, klen, vlen});
    }
    __device__ __forceinline__ void put(uint64_t k, uint64_t t, uint64_t ko, uint64_t vo, uint32_t kl, uint32_t vl) {
        const uint32_t slot = static_cast<uint32_t>(k) & 63u;
        if (slot == lane) {
            tag = t;
            koff = ko;
            voff = vo;
            klen = kl;
            vlen = vl;
        }
        if (slot == 63u) flush(k - 63u, 64u);
    }
    __device__ __forceinline__ void finish(uint64_t found) {
        const uint32_t rest = static_cast<uint32_t>(found) & 63u;
        if (rest) flush(found - rest, rest);
    }
};

// ---- the walk -------------------------------------------------------------
struct WbRes {
    uint64_t found, key_bytes, val_bytes, seq;
    uint32_t status;
};

// coding.rs:186-204 and :294-305 over the record's remaining input
// [*pos, n): LV_WB_OK with *len and *pos past the length, or the error.
template <class Src>
__device__ __forceinline__ uint32_t wb_varstring(Src &src, uint64_t off, uint64_t n, uint64_t *pos, uint32_t *len) {
    uint32_t result;
    if (!varint32(src, off, n, pos, &result)) return LV_WB_BAD_VARINT;
    if (n - *pos < result) return LV_WB_BAD_LENGTH;
    *len = result;
    return LV_WB_OK;
}

// WriteBatch::iterate over d_payload[off, off + n), the extent already known
// to lie inside the payload.  Reads only bytes of the record (through src).
template <class Src, class Sink>
__device__ __forceinline__ WbRes wb_walk(Src &src, Sink &sink, uint64_t off, uint64_t n) {
    WbRes r{0, 0, 0, 0, LV_WB_OK};
    if (n < LV_WB_HEADER_SIZE) {
        r.status = LV_WB_TOO_SMALL;
        return r;
    }
    uint64_t seq = 0;
    uint32_t count = 0;
    for (uint32_t i = 0; i < 8; ++i) seq |= static_cast<uint64_t>(src.byte(off + i)) << (8 * i);
    for (uint32_t i = 0; i < 4; ++i) count |= src.byte(off + 8 + i) << (8 * i);
    r.seq = seq;
    uint64_t pos = LV_WB_HEADER_SIZE;
    while (pos < n) {
        const uint32_t tag = src.byte(off + pos);
        ++pos;
        if (tag > LV_WB_TYPE_VALUE) {
            r.status = LV_WB_BAD_TAG;
            break;
        }
        uint32_t klen = 0, vlen = 0;
        if ((r.status = wb_varstring(src, off, n, &pos, &klen)) != LV_WB_OK) break;
        const uint64_t koff = off + pos;
        pos += klen;
        uint64_t voff = off + pos;
        if (tag == LV_WB_TYPE_VALUE) {
            if ((r.status = wb_varstring(src, off, n, &pos, &vlen)) != LV_WB_OK) break;
            voff = off + pos;
            pos += vlen;
        }
        sink.put(r.found, ((seq + r.found) << 8) | tag, koff, voff, klen, vlen);
        ++r.found;
        r.key_bytes += klen;
        r.val_bytes += vlen;
    }
    sink.finish(r.found);
    if (r.status == LV_WB_OK && r.found != count) r.status = LV_WB_WRONG_COUNT;
    return r;
}

// Workgroup-wide exclusive scan of one u64 per thread (Hillis-Steele in LDS);
// *total = the sum of all.
template <uint32_t kThreads>
__device__ __forceinline__ uint64_t wb_scan(uint64_t v, uint64_t *lds, uint64_t *total) {
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kThreads; d <<= 1) {
        const uint64_t o = t >= d ? lds[t - d] : 0ull;
        __syncthreads();
        v += o;
        lds[t] = v;
        __syncthreads();
    }
    const uint64_t ex = t ? lds[t - 1] : 0ull;
    *total = lds[kThreads - 1];
    __syncthreads();
    return ex;
}

// Kernel 0 (one thread): the head.  A kernel, not a memset: a memset node inside a longer captured graph does not
// replay reliably (DESIGN, mt_init), and a chain of kernels does.
__global__ void wb_init(WbHead *h) { *h = WbHead{}; }

// Kernel 1: the count walk.  A workgroup takes a tile of kWbTile records, its
// waves the tile's 64-record chunks.
__global__ __launch_bounds__(kWbThreads) void wb_count(const WbArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[kWbWaves][kWbWindow + kWinPad];
    __shared__ unsigned long long s_tile;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t n = records_to_walk(A.records, A.upstream, A.rec_cap);
    const uint64_t ntiles = (n + kWbTile - 1) / kWbTile;
    uint64_t kb = 0, vb = 0, bad = 0, last = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0) s_tile = 0;
        __syncthreads();
        uint64_t ops = 0;
        for (uint32_t c = wave; c < kWbChunks; c += kWbWaves) {
            const uint64_t r = tile * kWbTile + c * 64u + lane;
            uint64_t off, len;
            const uint32_t cls = record_class<kWbSmall>(A.rec_off, A.rec_len, A.payload_bytes, r, n, &off, &len);
            WbRes res{0, 0, 0, 0, cls == kRecOutOfRange ? LV_WB_OUT_OF_RANGE : LV_WB_OK};
            dispatch(
                cls, off, len,
                [&] {
                    LaneSrc src(A.payload);
                    WbNoSink sink;
                    res = wb_walk(src, sink, off, len);
                },
                [&](uint32_t b, uint64_t woff, uint64_t wlen) {
                    WaveSrc<kWbWindow, kWbRound> src(A.payload, s_win[wave], woff + wlen, lane);
                    WbNoSink sink;
                    const WbRes wr = wb_walk(src, sink, woff, wlen);
                    if (lane == b) res = wr;
                });
            if (r < n) {
                A.cnt[r] = res.found;
                A.st[r] = res.status;
                ops += res.found;
                kb += res.key_bytes;
                vb += res.val_bytes;
                bad += res.status != LV_WB_OK;
                if (res.found) {
                    const uint64_t ls = res.seq + res.found - 1;  // wrapping
                    last = ls > last ? ls : last;
                }
            }
        }
        ops = wave_sum(ops);
        if (lane == 0 && ops) atomicAdd(&s_tile, static_cast<unsigned long long>(ops));
        __syncthreads();
        if (tid == 0) A.tsum[tile] = s_tile;
        __syncthreads();
    }
    kb = wave_sum(kb);
    vb = wave_sum(vb);
    bad = wave_sum(bad);
    last = wave_max(last);
    if (lane == 0) {
        if (kb) atomicAdd(&A.head->key_bytes, static_cast<unsigned long long>(kb));
        if (vb) atomicAdd(&A.head->val_bytes, static_cast<unsigned long long>(vb));
        if (bad) atomicAdd(&A.head->bad, static_cast<unsigned long long>(bad));
        if (last) atomicMax(&A.head->last_seq, static_cast<unsigned long long>(last));
    }
}

// Kernel 2 (one workgroup): the exclusive scan of the tile counts in place,
// the totals and the status.
__global__ __launch_bounds__(kWbScanThreads) void wb_tiles(const WbArgs A) {
    __shared__ uint64_t s_scan[kWbScanThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t n = records_to_walk(A.records, A.upstream, A.rec_cap);
    const uint64_t ntiles = (n + kWbTile - 1) / kWbTile;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < ntiles; base += kWbScanThreads) {
        const uint64_t tile = base + t;
        const uint64_t v = tile < ntiles ? A.tsum[tile] : 0ull;
        uint64_t total;
        const uint64_t ex = wb_scan<kWbScanThreads>(v, s_scan, &total);
        if (tile < ntiles) A.tsum[tile] = carry + ex;
        carry += total;
    }
    if (t == 0) {
        uint64_t status = 0;
        const bool up = A.upstream && *A.upstream;
        if (up) status |= LV_WB_DECODE_UPSTREAM;
        if (!up && *A.records > A.rec_cap) status |= LV_WB_DECODE_REC_OVER;
        if (carry > A.out.op_cap) status |= LV_WB_DECODE_OP_OVER;
        lv_wb_totals tot;
        tot.records = up ? 0ull : *A.records;
        tot.ops = carry;
        tot.key_bytes = A.head->key_bytes;
        tot.value_bytes = A.head->val_bytes;
        tot.bad_records = A.head->bad;
        tot.last_sequence = A.head->last_seq;
        tot.status = status;
        *A.out.d_totals = tot;
        A.head->n = n;
        A.head->status = status;
        if (!status) A.out.d_rec_op[n] = carry;
    }
}

// Kernel 3: the emit walk.  The scan of a tile's counts gives each record's
// base; the records with ops are walked again, as in wb_count.
__global__ __launch_bounds__(kWbThreads) void wb_emit(const WbArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[kWbWaves][kWbWindow + kWinPad];
    __shared__ uint64_t s_scan[kWbThreads];
    __shared__ uint64_t s_base[kWbTile];
    if (A.head->status) return;  // only the totals are written
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t n = A.head->n;
    const uint64_t ntiles = (n + kWbTile - 1) / kWbTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t first = tile * kWbTile + static_cast<uint64_t>(tid) * kWbPer;
        uint64_t c[kWbPer], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < kWbPer; ++j) {
            c[j] = first + j < n ? A.cnt[first + j] : 0ull;
            sum += c[j];
        }
        uint64_t total;
        uint64_t at = A.tsum[tile] + wb_scan<kWbThreads>(sum, s_scan, &total);
#pragma unroll
        for (uint32_t j = 0; j < kWbPer; ++j) {
            s_base[tid * kWbPer + j] = at;
            if (first + j < n) {
                A.out.d_rec_op[first + j] = at;
                A.out.d_rec_status[first + j] = A.st[first + j];
            }
            at += c[j];
        }
        __syncthreads();
        for (uint32_t ch = wave; ch < kWbChunks; ch += kWbWaves) {
            const uint64_t r = tile * kWbTile + ch * 64u + lane;
            uint64_t off, len;
            uint32_t cls = record_class<kWbSmall>(A.rec_off, A.rec_len, A.payload_bytes, r, n, &off, &len);
            if (cls && A.cnt[r] == 0) cls = kRecNone;  // nothing to write
            const uint64_t base = s_base[ch * 64u + lane];
            // lvk::dispatch, spelled out: through the template this kernel takes 92 VGPRs, not 90 (DESIGN)
            if (cls == kRecLane) {
                LaneSrc src(A.payload);
                WbLaneSink sink{A.out.d_ops, base, A.out.op_cap};
                wb_walk(src, sink, off, len);
            }
            uint64_t m = __ballot(cls == kRecWave);
            while (m) {  // wave-uniform
                const uint32_t b = static_cast<uint32_t>(__builtin_ctzll(m));
                m &= m - 1;
                const uint64_t woff = shfl64(off, b), wlen = shfl64(len, b), wbase = shfl64(base, b);
                WaveSrc<kWbWindow, kWbRound> src(A.payload, s_win[wave], woff + wlen, lane);
                WbWaveSink sink{A.out.d_ops, wbase, A.out.op_cap, lane, 0, 0, 0, 0, 0};
                wb_walk(src, sink, woff, wlen);
            }
        }
        __syncthreads();  // s_base is rewritten by the next tile
    }
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxRecCap = 0xfffffffeull;
constexpr uint64_t kMaxOpCap = 1ull << 58;  // op_cap * sizeof(lv_wb_op) stays far from 2^64

constexpr uint64_t wb_tiles_of(uint64_t cap) { return (cap + lvk::kWbTile - 1) / lvk::kWbTile; }

// The workspace for rec_cap = cap, region by region: fills A's workspace pointers.
void wb_carve(Carve &C, uint64_t cap, lvk::WbArgs &A) {
    A.head = C.take<lvk::WbHead>(1);
    A.cnt = C.take<uint64_t>(cap);
    A.st = C.take<uint32_t>(cap);
    A.tsum = C.take<uint64_t>(wb_tiles_of(cap));
}

}  // namespace

// wb_count / wb_emit: a workgroup takes a tile of kWbTile records a trip.
uint64_t lvgpu_internal::wb_grid(uint64_t rec_cap, uint64_t cus, uint64_t *per_trip) {
    if (per_trip) *per_trip = lvk::kWbTile;
    return std::min<uint64_t>(wb_tiles_of(rec_cap), 16 * cus);
}
// wb_tiles scans kWbScanThreads tile counts a round.
uint64_t lvgpu_internal::wb_tiles_round() { return static_cast<uint64_t>(lvk::kWbScanThreads) * lvk::kWbTile; }

extern "C" {

size_t lv_write_batch_decode_workspace_bytes(size_t rec_cap) {
    lvk::WbArgs A{};
    Carve C{nullptr};
    wb_carve(C, rec_cap, A);
    return C.at;
}

int lv_write_batch_decode_device(const uint8_t *d_payload, size_t payload_bytes, const uint64_t *d_rec_off,
                                 const uint64_t *d_rec_len, const uint64_t *d_records,
                                 const uint64_t *d_upstream_status, size_t rec_cap, const lv_wb_decode_out *out,
                                 uint32_t flags, void *d_workspace, size_t workspace_bytes, void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (!out) return set_err(LV_ERR_INVALID, "null output descriptor");
    if (!out->d_totals) return set_err(LV_ERR_INVALID, "null d_totals");
    if (misaligned(out->d_totals, 8)) return set_err(LV_ERR_INVALID, "d_totals must be 8-byte aligned");
    if (!d_records) return set_err(LV_ERR_INVALID, "null d_records");
    if (!d_payload && payload_bytes) return set_err(LV_ERR_INVALID, "null d_payload");
    if (rec_cap > kMaxRecCap) return set_err(LV_ERR_INVALID, "rec_cap too large for one decode (at most 2^32 - 2)");
    if (out->op_cap > kMaxOpCap) return set_err(LV_ERR_INVALID, "op_cap too large (at most 2^58)");
    if (rec_cap && (!d_rec_off || !d_rec_len)) return set_err(LV_ERR_INVALID, "null record array (d_rec_off / d_rec_len)");
    if (!out->d_rec_op) return set_err(LV_ERR_INVALID, "null d_rec_op");
    if (misaligned(out->d_rec_op, 8)) return set_err(LV_ERR_INVALID, "d_rec_op must be 8-byte aligned");
    if (rec_cap && !out->d_rec_status) return set_err(LV_ERR_INVALID, "null d_rec_status");
    if (out->op_cap && !out->d_ops) return set_err(LV_ERR_INVALID, "null d_ops");
    if (misaligned(out->d_ops, 16)) return set_err(LV_ERR_INVALID, "d_ops must be 16-byte aligned");
    if (!d_workspace) return set_err(LV_ERR_INVALID, "null workspace");
    if (misaligned(d_workspace, 16)) return set_err(LV_ERR_INVALID, "workspace must be 16-byte aligned");
    lvk::WbArgs A{};
    Carve C{static_cast<uint8_t *>(d_workspace)};
    wb_carve(C, rec_cap, A);
    if (workspace_bytes < C.at) return set_err(LV_ERR_INVALID, "workspace too small");
    if (overlaps(out->d_ops, static_cast<uint64_t>(out->op_cap) * sizeof(lv_wb_op), d_payload, payload_bytes))
        return set_err(LV_ERR_INVALID, "d_ops overlaps d_payload");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    A.payload = d_payload;
    A.payload_bytes = payload_bytes;
    A.rec_off = d_rec_off;
    A.rec_len = d_rec_len;
    A.records = d_records;
    A.upstream = d_upstream_status;
    A.rec_cap = rec_cap;
    A.out = *out;

    const uint64_t cus = static_cast<uint64_t>(c->cus > 0 ? c->cus : 1);
    const dim3 b(lvk::kWbThreads);
    const uint32_t grid = static_cast<uint32_t>(lvgpu_internal::wb_grid(rec_cap, cus));
    hipLaunchKernelGGL(lvk::wb_init, dim3(1), dim3(1), 0, s, A.head);
    if (grid) hipLaunchKernelGGL(lvk::wb_count, dim3(grid), b, 0, s, A);
    hipLaunchKernelGGL(lvk::wb_tiles, dim3(1), dim3(lvk::kWbScanThreads), 0, s, A);
    if (grid) hipLaunchKernelGGL(lvk::wb_emit, dim3(grid), b, 0, s, A);
    g_kernel = "wb_count+wb_tiles+wb_emit";
    return check_launch();
}

}  // extern "C"
