// lv_write_batch_encode_device: an op table over a key/value arena in HBM to
// WriteBatch records (include/lvgpu/write_batch.h, "The inverse";
// csrc/write_batch.cc holds the serial twin).  The inverse of write_batch.hip:
// WriteBatch::put / delete / set_sequence (write_batch.rs:57-78) for every
// record of a commit group at once.
//
// An entry's place is the sum of the sizes before it, so the call is a size,
// scan and emit pass, all or nothing:
//
//   we_validate  a lane per record: UPSTREAM and REC_OVER (one thread), then
//                d_rec_op[r] <= d_rec_op[r + 1] <= op_cap; the lowest record
//                that fails (BAD_BOUNDS).
//   we_size      a lane per op, a tile of kWeTile ops per workgroup: the op,
//                its type and extents (the lowest op that fails: BAD_OP), the
//                entry's size; the tile-local scan in LDS leaves each op's
//                exclusive prefix and the tile's sum, and the tile's key and
//                value bytes.
//   we_carry     one wave: the exclusive scan of the tiles' sums, the sums of
//                their key and value bytes, the totals and the status, final
//                before any byte of the outputs.
//   we_records   a lane per record: d_rec_off, d_rec_len, the 12-byte header.
//   we_emit      a lane per op: its record (a bounded binary search of
//                d_rec_op between the records of the workgroup's first and
//                last op), the type byte and the varints, the op of
//                d_ops_out; the key and the value are lvk::group_copy's -- one
//                of fewer than kWeWaveCopy bytes the lane copies, a longer one
//                kWeCopyLanes lanes of the wave share, 64 / kWeCopyLanes such
//                copies at a time, in 16-byte stores of the destination's
//                alignment.
//
// Every grid is sized by the work its capacity allows, one workgroup per tile;
// the launch sequence depends only on op_cap == 0.  No workgroup waits on
// another.  The only loop whose trip count grows with the input is the
// carry's, 64 tiles a round; the searches are bounded by the 32 bits of a
// record index.  All sizes and positions are u64.  The op loads and stores,
// the extent check, both levels of the scan and the shared copy are
// lvk/stage.h's (load_op, store_op, extent_ok, tile_scan, carry_scan,
// group_copy), and so are the wave's sums, the varint store and the search
// (wave_sum, put_varint, record_of).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/write_batch.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/stage.h"

namespace lvk {

constexpr uint32_t kWeThreads = 256;
constexpr uint32_t kWeTile = 1024;      // ops per scan tile
constexpr uint32_t kWeWaveCopy = 64;    // bytes from which a copy is the wave's
constexpr uint32_t kWeCopyLanes = 16;   // lanes of a wave that share one such copy
constexpr uint32_t kWePer = kWeTile / kWeThreads;
static_assert(kWeTile % kWeThreads == 0, "a tile is whole rounds of a workgroup");
static_assert(kWeWaveCopy >= 16, "a wave copy has at least one granule");
static_assert(kWeCopyLanes >= 16 && 64 % kWeCopyLanes == 0, "a copy's lanes cover a ragged head or tail of 15 bytes");

struct WeHead {  // workspace, zeroed by we_init
    uint64_t st0;      // we_validate: UPSTREAM or REC_OVER
    uint64_t n;        // the records to encode (0 with st0)
    uint64_t go;       // we_carry: status 0, the outputs are written
    uint64_t entries;  // we_carry: the bytes of all entries (out_bytes - 12 n)
    // the lowest failing record / op index as the maximum of its complement (0: none)
    unsigned long long bad_rec, bad_op;
    uint64_t pad[2];
};

struct WeArgs {
    const uint8_t *src;
    uint64_t src_bytes;
    const lv_wb_op *ops;
    uint64_t op_cap;
    const uint64_t *rec_op, *records, *upstream;
    uint64_t rec_cap, first_seq;
    lv_wb_encode_out out;
    // workspace
    WeHead *head;
    uint64_t *pre;   // [op_cap] the bytes of the entries before op j in its tile
    uint64_t *tsum;  // [tiles] the tiles' bytes, then (we_carry) the bytes before the tile
    uint64_t *tkey, *tval;  // [tiles] the tiles' key and value bytes
};

// lvk::varint_len of a u32 as a compare ladder: with the shared loop we_size grows
// from 1,269 to 1,297 lines of assembly and from 52 to 55 SGPRs (DESIGN)
__device__ __forceinline__ uint32_t we_varint_len(uint32_t v) {
    return v < (1u << 7) ? 1u : v < (1u << 14) ? 2u : v < (1u << 21) ? 3u : v < (1u << 28) ? 4u : 5u;
}

// The bytes of all entries before op j (j <= ops; behind we_carry).
__device__ __forceinline__ uint64_t we_before(const WeArgs &A, uint64_t j, uint64_t nops) {
    return j < nops ? A.pre[j] + A.tsum[j / kWeTile] : A.head->entries;
}

// Kernel 0 (one thread): the head.  A kernel, not a memset: a memset node inside a longer captured graph does not
// replay reliably (DESIGN, mt_init), and a chain of kernels does.
__global__ void we_init(WeHead *h) { *h = WeHead{}; }

// Kernel 1: the record bounds.
__global__ __launch_bounds__(kWeThreads) void we_validate(const WeArgs A) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kWeThreads + threadIdx.x;
    uint64_t st0 = 0, n = 0;
    if (A.upstream && *A.upstream) {
        st0 = LV_WB_ENCODE_UPSTREAM;
    } else {
        n = *A.records;
        if (n > A.rec_cap) {
            st0 = LV_WB_ENCODE_REC_OVER;
            n = 0;
        }
    }
    if (r == 0) {  // (nobody reads these during this launch)
        A.head->st0 = st0;
        A.head->n = n;
    }
    if (r < n) {
        const uint64_t a = A.rec_op[r], b = A.rec_op[r + 1];
        if (!(a <= b && b <= A.op_cap)) atomicMax(&A.head->bad_rec, static_cast<unsigned long long>(~r));
    }
}

// Kernel 2: the ops' checks and sizes, the tile-local scan.
__global__ __launch_bounds__(kWeThreads) void we_size(const WeArgs A) {
    __shared__ uint64_t s[kWeTile];
    __shared__ uint64_t s_kv[2][kWeThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const WeHead *h = A.head;
    const uint64_t n = h->n;
    if (!n || h->bad_rec) return;  // no op is read
    const uint64_t first = A.rec_op[0], nops = A.rec_op[n] - first;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kWeTile;
    if (base >= nops) return;
    const uint32_t cnt = static_cast<uint32_t>(nops - base < kWeTile ? nops - base : kWeTile);
    uint64_t own[kWePer], kb = 0, vb = 0;
#pragma unroll
    for (uint32_t k = 0; k < kWePer; ++k) {
        const uint32_t j = tid + k * kWeThreads;
        uint64_t v = 0;
        if (j < cnt) {
            const uint64_t i = first + base + j;
            const lv_wb_op o = load_op(A.ops + i);
            const uint32_t type = static_cast<uint32_t>(o.tag & 0xffu);
            if (type > LV_WB_TYPE_VALUE || !extent_ok(o.key_off, o.key_len, A.src_bytes) ||
                (type == LV_WB_TYPE_VALUE && !extent_ok(o.val_off, o.val_len, A.src_bytes))) {
                atomicMax(&A.head->bad_op, static_cast<unsigned long long>(~i));
            } else {
                v = 1 + we_varint_len(o.key_len) + static_cast<uint64_t>(o.key_len);
                kb += o.key_len;
                if (type == LV_WB_TYPE_VALUE) {
                    v += we_varint_len(o.val_len) + static_cast<uint64_t>(o.val_len);
                    vb += o.val_len;
                }
            }
        }
        own[k] = v;
        s[j] = v;
    }
    __syncthreads();
    tile_scan<kWeTile, kWeThreads>(s, 1, tid);
#pragma unroll
    for (uint32_t k = 0; k < kWePer; ++k) {
        const uint32_t j = tid + k * kWeThreads;
        if (j < cnt) A.pre[base + j] = s[j] - own[k];
    }
    // the tile's key and value bytes: the waves' sums (every lane is here), then theirs
    kb = wave_sum(kb);
    vb = wave_sum(vb);
    if (lane == 0) {
        s_kv[0][tid >> 6] = kb;
        s_kv[1][tid >> 6] = vb;
    }
    __syncthreads();
    if (tid == 0) {
        uint64_t k = 0, v = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWeThreads / 64; ++w) {
            k += s_kv[0][w];
            v += s_kv[1][w];
        }
        A.tsum[blockIdx.x] = s[cnt - 1];
        A.tkey[blockIdx.x] = k;
        A.tval[blockIdx.x] = v;
    }
}

// Kernel 3 (one wave): the tiles' sums become their exclusive scan; the totals
// and the status, once, before any byte of the outputs is written.
__global__ __launch_bounds__(64) void we_carry(const WeArgs A) {
    WeHead *h = A.head;
    const uint32_t lane = threadIdx.x;
    lv_wb_encode_totals t{};
    t.bad_record = t.bad_op = ~0ull;
    t.last_sequence = A.first_seq - 1;
    const uint64_t n = h->n;  // (wave-uniform, like every branch below)
    if (h->st0) {
        t.status = h->st0;
        if (h->st0 == LV_WB_ENCODE_REC_OVER) t.records = *A.records;
    } else if (h->bad_rec) {
        t.status = LV_WB_ENCODE_BAD_BOUNDS;
        t.records = n;
        t.bad_record = ~static_cast<uint64_t>(h->bad_rec);
    } else if (h->bad_op) {
        t.status = LV_WB_ENCODE_BAD_OP;
        t.records = n;
        t.bad_op = ~static_cast<uint64_t>(h->bad_op);
        t.bad_record = record_of(A.rec_op, t.bad_op, 0, n - 1);  // (an op of a record: n > 0)
    } else {
        const uint64_t nops = n ? A.rec_op[n] - A.rec_op[0] : 0;
        const uint64_t tiles = (nops + kWeTile - 1) / kWeTile;
        const uint64_t entries = carry_scan(A.tsum, 1, tiles, lane);
        uint64_t kb = 0, vb = 0;
        for (uint64_t i = lane; i < tiles; i += 64) {
            kb += A.tkey[i];
            vb += A.tval[i];
        }
        t.records = n;
        t.ops = nops;
        t.key_bytes = wave_sum(kb);  // (every lane is here)
        t.value_bytes = wave_sum(vb);
        t.out_bytes = LV_WB_HEADER_SIZE * n + entries;
        t.last_sequence = A.first_seq - 1 + nops;
        if (t.out_bytes > A.out.out_cap) t.status = LV_WB_ENCODE_OUT_OVER;
        if (lane == 0) {
            h->entries = entries;
            h->go = !t.status;
        }
    }
    if (lane == 0) *A.out.d_totals = t;
}

// Kernel 4: the records' extents and headers.
__global__ __launch_bounds__(kWeThreads) void we_records(const WeArgs A) {
    const WeHead *h = A.head;
    if (!h->go) return;
    const uint64_t n = h->n, r = static_cast<uint64_t>(blockIdx.x) * kWeThreads + threadIdx.x;
    if (r >= n) return;
    const uint64_t first = A.rec_op[0], nops = A.rec_op[n] - first;
    const uint64_t a = A.rec_op[r] - first, b = A.rec_op[r + 1] - first;
    const uint64_t off = LV_WB_HEADER_SIZE * r + we_before(A, a, nops);
    const uint64_t len = LV_WB_HEADER_SIZE + we_before(A, b, nops) - we_before(A, a, nops);
    A.out.d_rec_off[r] = off;
    A.out.d_rec_len[r] = len;
    const uint64_t seq = A.first_seq + a;
    const uint32_t count = static_cast<uint32_t>(b - a);  // (<= op_cap <= 2^30)
    uint8_t hdr[LV_WB_HEADER_SIZE];  // fixed64 and fixed32, little-endian
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) hdr[i] = static_cast<uint8_t>(seq >> (8 * i));
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) hdr[8 + i] = static_cast<uint8_t>(count >> (8 * i));
    __builtin_memcpy(A.out.d_out + off, hdr, LV_WB_HEADER_SIZE);  // any alignment
}

// Kernel 5: the entries.  Every lane of a wave stays to the end: the long
// copies are the wave's.
__global__ __launch_bounds__(kWeThreads) void we_emit(const WeArgs A) {
    __shared__ uint64_t s_rec[2];  // the records of the workgroup's first and last op
    const WeHead *h = A.head;
    if (!h->go) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t n = h->n;
    const uint64_t blk = static_cast<uint64_t>(blockIdx.x) * kWeThreads;
    if (!n) return;
    const uint64_t first = A.rec_op[0], nops = A.rec_op[n] - first;
    if (blk >= nops) return;  // the whole workgroup
    if (tid < 2) {
        const uint64_t last = nops - blk < kWeThreads ? nops - 1 : blk + kWeThreads - 1;
        s_rec[tid] = record_of(A.rec_op, first + (tid ? last : blk), 0, n - 1);
    }
    __syncthreads();
    const uint64_t j = blk + tid;
    uint8_t *kd = nullptr, *vd = nullptr;
    const uint8_t *ks = nullptr, *vs = nullptr;
    uint64_t kn = 0, vn = 0;
    if (j < nops) {
        const uint64_t i = first + j;
        const lv_wb_op o = load_op(A.ops + i);
        const uint32_t type = static_cast<uint32_t>(o.tag & 0xffu);
        const uint64_t r = record_of(A.rec_op, i, s_rec[0], s_rec[1]);
        const uint64_t at = LV_WB_HEADER_SIZE * (r + 1) + A.pre[j] + A.tsum[j / kWeTile];
        uint8_t *p = A.out.d_out + at;
        *p++ = static_cast<uint8_t>(type);
        p = put_varint(p, o.key_len);
        lv_wb_op w;
        w.tag = ((A.first_seq + j) << 8) | type;
        w.key_off = static_cast<uint64_t>(p - A.out.d_out);
        w.key_len = o.key_len;
        kd = p;
        ks = A.src + o.key_off;
        kn = o.key_len;
        p += kn;
        w.val_off = w.key_off + kn;
        w.val_len = 0;
        if (type == LV_WB_TYPE_VALUE) {
            p = put_varint(p, o.val_len);
            w.val_off = static_cast<uint64_t>(p - A.out.d_out);
            w.val_len = o.val_len;
            vd = p;
            vs = A.src + o.val_off;
            vn = o.val_len;
        }
        if (A.out.d_ops_out) store_op(A.out.d_ops_out + j, w);
    }
    group_copy<kWeCopyLanes, kWeWaveCopy>(kd, ks, kn, lane);
    group_copy<kWeCopyLanes, kWeWaveCopy>(vd, vs, vn, lane);
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxRecCap = 0xfffffffeull;
constexpr uint64_t kMaxOpCap = 1ull << 30;  // a count is a fixed32; no sum of sizes leaves u64 (write_batch.h)

constexpr uint64_t we_tiles(uint64_t cap) { return (cap + lvk::kWeTile - 1) / lvk::kWeTile; }

// The workspace for op_cap = cap, region by region: fills A's workspace pointers.
void we_carve(Carve &C, uint64_t cap, lvk::WeArgs &A) {
    A.head = C.take<lvk::WeHead>(1);
    A.pre = C.take<uint64_t>(cap);
    A.tsum = C.take<uint64_t>(we_tiles(cap));
    A.tkey = C.take<uint64_t>(we_tiles(cap));
    A.tval = C.take<uint64_t>(we_tiles(cap));
}

}  // namespace

extern "C" {

size_t lv_write_batch_encode_workspace_bytes(size_t rec_cap, size_t op_cap) {
    if (rec_cap > kMaxRecCap || op_cap > kMaxOpCap) return 0;
    lvk::WeArgs A{};
    Carve C{nullptr};
    we_carve(C, op_cap, A);
    return C.at;
}

int lv_write_batch_encode_device(const uint8_t *d_src, size_t src_bytes, const lv_wb_op *d_ops, size_t op_cap,
                                 const uint64_t *d_rec_op, const uint64_t *d_records,
                                 const uint64_t *d_upstream_status, size_t rec_cap, uint64_t first_sequence,
                                 const lv_wb_encode_out *out, uint32_t flags, void *d_workspace,
                                 size_t workspace_bytes, void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (!out) return set_err(LV_ERR_INVALID, "null output descriptor");
    if (!out->d_totals) return set_err(LV_ERR_INVALID, "null d_totals");
    if (misaligned(out->d_totals, 8)) return set_err(LV_ERR_INVALID, "d_totals must be 8-byte aligned");
    if (!d_records) return set_err(LV_ERR_INVALID, "null d_records");
    if (!d_src && src_bytes) return set_err(LV_ERR_INVALID, "null d_src");
    if (rec_cap > kMaxRecCap) return set_err(LV_ERR_INVALID, "rec_cap too large for one encode (at most 2^32 - 2)");
    if (op_cap > kMaxOpCap) return set_err(LV_ERR_INVALID, "op_cap too large for one encode (at most 2^30)");
    if (!d_rec_op) return set_err(LV_ERR_INVALID, "null d_rec_op");
    if (misaligned(d_rec_op, 8)) return set_err(LV_ERR_INVALID, "d_rec_op must be 8-byte aligned");
    if (rec_cap && (!out->d_rec_off || !out->d_rec_len))
        return set_err(LV_ERR_INVALID, "null record array (d_rec_off / d_rec_len)");
    if (misaligned(out->d_rec_off, 8) || misaligned(out->d_rec_len, 8))
        return set_err(LV_ERR_INVALID, "d_rec_off and d_rec_len must be 8-byte aligned");
    if (op_cap && !d_ops) return set_err(LV_ERR_INVALID, "null d_ops");
    if (misaligned(d_ops, 16) || misaligned(out->d_ops_out, 16))
        return set_err(LV_ERR_INVALID, "d_ops and d_ops_out must be 16-byte aligned");
    if (out->out_cap && !out->d_out) return set_err(LV_ERR_INVALID, "null d_out");
    if (!d_workspace) return set_err(LV_ERR_INVALID, "null workspace");
    if (misaligned(d_workspace, 16)) return set_err(LV_ERR_INVALID, "workspace must be 16-byte aligned");
    lvk::WeArgs A{};
    Carve C{static_cast<uint8_t *>(d_workspace)};
    we_carve(C, op_cap, A);
    if (workspace_bytes < C.at) return set_err(LV_ERR_INVALID, "workspace too small");
    const uint64_t table_bytes = static_cast<uint64_t>(op_cap) * sizeof(lv_wb_op);
    if (overlaps(out->d_out, out->out_cap, d_src, src_bytes)) return set_err(LV_ERR_INVALID, "d_out overlaps d_src");
    if (overlaps(out->d_out, out->out_cap, d_ops, table_bytes)) return set_err(LV_ERR_INVALID, "d_out overlaps d_ops");
    if (out->d_ops_out && overlaps(out->d_out, out->out_cap, out->d_ops_out, table_bytes))
        return set_err(LV_ERR_INVALID, "d_out overlaps d_ops_out");
    if (out->d_ops_out && overlaps(out->d_ops_out, table_bytes, d_ops, table_bytes))
        return set_err(LV_ERR_INVALID, "d_ops_out overlaps d_ops");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    A.src = d_src;
    A.src_bytes = src_bytes;
    A.ops = d_ops;
    A.op_cap = op_cap;
    A.rec_op = d_rec_op;
    A.records = d_records;
    A.upstream = d_upstream_status;
    A.rec_cap = rec_cap;
    A.first_seq = first_sequence;
    A.out = *out;

    const dim3 b(lvk::kWeThreads);
    // a lane per record, at least one workgroup: its first thread judges UPSTREAM and REC_OVER
    const uint32_t rec_grid =
        static_cast<uint32_t>(rec_cap ? (static_cast<uint64_t>(rec_cap) + lvk::kWeThreads - 1) / lvk::kWeThreads : 1);
    const uint32_t op_grid = static_cast<uint32_t>((static_cast<uint64_t>(op_cap) + lvk::kWeThreads - 1) / lvk::kWeThreads);
    hipLaunchKernelGGL(lvk::we_init, dim3(1), dim3(1), 0, s, A.head);
    hipLaunchKernelGGL(lvk::we_validate, dim3(rec_grid), b, 0, s, A);
    if (op_cap) hipLaunchKernelGGL(lvk::we_size, dim3(static_cast<uint32_t>(we_tiles(op_cap))), b, 0, s, A);
    hipLaunchKernelGGL(lvk::we_carry, dim3(1), dim3(64), 0, s, A);
    hipLaunchKernelGGL(lvk::we_records, dim3(rec_grid), b, 0, s, A);
    if (op_cap) hipLaunchKernelGGL(lvk::we_emit, dim3(op_grid), b, 0, s, A);
    g_kernel = "we_validate+we_size+we_carry+we_records+we_emit";
    return check_launch();
}

}  // extern "C"
