// lv_memtable_build_device / lv_memtable_get_device: the op table of
// lv_write_batch_decode_device sorted into memtable order (internal-key order,
// include/lvgpu/memtable.h) and a batched MemTable::get over the result.
//
// The keys are variable-length byte strings at arbitrary byte offsets of
// d_payload, so the sort is a comparison sort over fixed-size entries
// {prefix, klen, idx}: the first kMtPrefix key bytes as big-endian words
// (zero-padded), which decide most comparisons by integer compares, the key
// length and the op index.  Only when two prefixes tie and both keys are
// longer than the prefix does a comparison go to d_payload for the remainders,
// and to d_ops for the tags.  The order is a strict total order (user key
// ascending, tag descending, op index descending), so no stability is needed.
//
//   mt_init       one thread zeroes the call's head in the workspace.
//   mt_tile_sort  a workgroup builds the entries of one tile of kMtTile ops
//                 (checking every extent: LV_MT_BUILD_BAD_OP), sorts them in
//                 LDS with a bitonic network and writes them to buffer 0.
//   mt_merge      pass p merges the sorted runs of kMtTile << p entries in
//                 pairs, from buffer p & 1 to the other.  A workgroup owns one
//                 output tile: two threads find its merge-path diagonals by
//                 binary search, the inputs are staged in LDS, every thread
//                 merges its share of the outputs and the tile leaves in
//                 coalesced stores (the network and the tile merge are
//                 lvk/merge_sort.h's, shared with version_set.hip).  A pass
//                 whose run width covers *d_n_ops exits.
//   mt_order      reads the buffer the last effective pass wrote (the parity
//                 is computed from *d_n_ops), writes d_order and counts the
//                 distinct user keys by comparing neighbours.
//   mt_totals     one thread writes *d_totals.
//   mt_get        one lane per query: a binary search over d_order.
//
// The launch sequence depends only on op_cap.  No workgroup waits on another
// inside a launch: the phases are ordered by launch boundaries alone, and every
// search loop is bounded.  All entry positions are u64, the lengths u32.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/memtable.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/knobs.h"
#include "lvk/merge_sort.h"
#include "lvk/stage.h"

namespace lvk {

constexpr uint32_t kMtTile = LVK_MT_TILE;      // entries per tile (sorted in LDS; one merge output tile)
constexpr uint32_t kMtPrefix = LVK_MT_PREFIX;  // key bytes held in an entry
constexpr uint32_t kMtWords = kMtPrefix / 8;
constexpr uint32_t kMtThreads = 256;
constexpr uint32_t kMtNone = 0xffffffffu;          // idx of a padding entry: after every op (op_cap <= 2^32 - 2)
static_assert(kMtPrefix == 8 || kMtPrefix == 16, "the prefix is one or two 8-byte words");
static_assert(kMtTile >= kMtThreads && (kMtTile & (kMtTile - 1)) == 0, "a tile is a power of two, a thread's share whole");

struct alignas(16) MtEnt {
    uint64_t p[kMtWords];  // key bytes [0, kMtPrefix) as big-endian words, zero-padded
    uint32_t klen, idx;
};
static_assert(sizeof(MtEnt) == (kMtWords == 1 ? 16 : 32), "entry size");
static_assert(sizeof(MtEnt) * kMtTile <= 65536, "a tile fits the LDS a workgroup may declare");

struct MtHead {  // workspace, zeroed by mt_init
    uint32_t bad, pad;
    unsigned long long user_keys;
};

struct MtArgs {
    const uint8_t *payload;
    uint64_t payload_bytes;
    const lv_wb_op *ops;
    const uint64_t *n_ops, *upstream;
    uint64_t op_cap;
    uint32_t *order;
    lv_mt_totals *totals;
    // workspace
    MtHead *head;
    MtEnt *buf[2];
};

// Entries to sort, and the status the inputs alone decide.
__device__ __forceinline__ uint64_t mt_entries(const MtArgs &A, uint32_t *status) {
    *status = 0;
    if (A.upstream && *A.upstream) {
        *status = LV_MT_BUILD_UPSTREAM;
        return 0;
    }
    const uint64_t n = *A.n_ops;
    if (n > A.op_cap) {
        *status = LV_MT_BUILD_OP_OVER;
        return 0;
    }
    return n;
}

// -1 / 0 / +1 over the user keys of two entries (the byte compares are
// lvk/stage.h's load_be64 and cmp_bytes).
__device__ __forceinline__ int mt_cmp_keys(const MtArgs &A, const MtEnt &a, const MtEnt &b) {
#pragma unroll
    for (uint32_t w = 0; w < kMtWords; ++w)
        if (a.p[w] != b.p[w]) return a.p[w] < b.p[w] ? -1 : 1;
    // equal prefixes.  A key no longer than the prefix is then a prefix of the
    // other (zero padding: "a", "a\0" and "a\0\0" share a prefix): the length decides.
    if (a.klen <= kMtPrefix || b.klen <= kMtPrefix) return a.klen < b.klen ? -1 : a.klen > b.klen ? 1 : 0;
    const uint64_t ka = A.ops[a.idx].key_off, kb = A.ops[b.idx].key_off;
    return cmp_bytes(A.payload + ka + kMtPrefix, a.klen - kMtPrefix, A.payload + kb + kMtPrefix, b.klen - kMtPrefix);
}

// The strict total order.  Padding entries come after every op.
__device__ __forceinline__ bool mt_less(const MtArgs &A, const MtEnt &a, const MtEnt &b) {
    if (b.idx == kMtNone) return a.idx != kMtNone;
    if (a.idx == kMtNone) return false;
    const int c = mt_cmp_keys(A, a, b);
    if (c) return c < 0;
    const uint64_t ta = A.ops[a.idx].tag, tb = A.ops[b.idx].tag;
    if (ta != tb) return ta > tb;  // tag descending, unsigned
    return a.idx > b.idx;          // an exact duplicate: the later op first
}
// The order as lvk/merge_sort.h takes it.
struct MtLess {
    const MtArgs &A;
    __device__ __forceinline__ bool operator()(const MtEnt &a, const MtEnt &b) const { return mt_less(A, a, b); }
};

// Kernel 0 (one thread): the head.  A kernel, not a memset: the call is then
// a chain of kernel launches only, which is also what a captured graph replays.
__global__ void mt_init(const MtArgs A) {
    A.head->bad = 0;
    A.head->pad = 0;
    A.head->user_keys = 0;
}

// Kernel 1: entries, extent checks and the sort of one tile.
__global__ __launch_bounds__(kMtThreads) void mt_tile_sort(const MtArgs A) {
    __shared__ MtEnt s[kMtTile];
    const uint32_t tid = threadIdx.x;
    uint32_t status;
    const uint64_t n = mt_entries(A, &status);
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kMtTile;
    if (base >= n) return;
    const uint32_t cnt = static_cast<uint32_t>(n - base < kMtTile ? n - base : kMtTile);
    uint32_t m = 2;  // the network's size: the power of two that holds the tile's entries
    while (m < cnt) m <<= 1;
    int bad = 0;
    for (uint32_t j = tid; j < m; j += kMtThreads) {
        MtEnt e;
#pragma unroll
        for (uint32_t w = 0; w < kMtWords; ++w) e.p[w] = ~0ull;
        e.klen = kMtNone;
        e.idx = kMtNone;
        if (j < cnt) {
            const lv_wb_op o = load_op(A.ops + base + j);
            if (!extent_ok(o.key_off, o.key_len, A.payload_bytes) ||
                !extent_ok(o.val_off, o.val_len, A.payload_bytes)) {
                bad = 1;
            } else {
                const uint8_t *k = A.payload + o.key_off;
                const uint32_t have = o.key_len < kMtPrefix ? o.key_len : kMtPrefix;
#pragma unroll
                for (uint32_t w = 0; w < kMtWords; ++w) {
                    uint64_t v = 0;
                    if (have >= 8 * w + 8) {
                        v = load_be64(k + 8 * w);
                    } else {
                        for (uint32_t b = 8 * w; b < have; ++b) v |= static_cast<uint64_t>(k[b]) << (56 - 8 * (b & 7u));
                    }
                    e.p[w] = v;
                }
                e.klen = o.key_len;
                e.idx = static_cast<uint32_t>(base + j);
            }
        }
        s[j] = e;
    }
    if (__syncthreads_or(bad)) {  // nothing of this tile is compared: a bad extent is never read
        if (tid == 0) atomicOr(&A.head->bad, 1u);
        return;
    }
    lds_bitonic_sort<kMtThreads>(s, m, tid, MtLess{A});
    MtEnt *out = A.buf[0];
    for (uint32_t j = tid; j < cnt; j += kMtThreads) out[base + j] = s[j];
}

// Kernel 2: one merge pass.  Runs of w = kMtTile << pass entries, in pairs
// (lvk::merge_tile: merge-path diagonals, the inputs staged in LDS).
__global__ __launch_bounds__(kMtThreads) void mt_merge(const MtArgs A, uint32_t pass) {
    __shared__ MtEnt s[kMtTile];
    __shared__ uint64_t s_split[2];
    const uint32_t tid = threadIdx.x;
    uint32_t status;
    const uint64_t n = mt_entries(A, &status);
    const uint64_t w = static_cast<uint64_t>(kMtTile) << pass;
    const uint64_t o0 = static_cast<uint64_t>(blockIdx.x) * kMtTile;
    if (w >= n || o0 >= n || A.head->bad) return;  // one run already, beyond the entries, or no table
    const MtEnt *in = pass & 1u ? A.buf[1] : A.buf[0];
    MtEnt *out = pass & 1u ? A.buf[0] : A.buf[1];
    merge_tile<kMtTile, kMtThreads>(MtLess{A}, in, out, n, w, o0, s, s_split, tid);
}

// Kernel 3: d_order and the distinct user keys.
__global__ __launch_bounds__(kMtThreads) void mt_order(const MtArgs A) {
    __shared__ uint32_t s_keys;
    const uint32_t tid = threadIdx.x;
    uint32_t status;
    const uint64_t n = mt_entries(A, &status);
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kMtThreads + tid;
    if (static_cast<uint64_t>(blockIdx.x) * kMtThreads >= n || A.head->bad) return;
    uint32_t par = 0;  // the passes that ran: those whose run width is below n
    for (uint64_t w = kMtTile; w < n; w <<= 1) par ^= 1u;
    const MtEnt *src = par ? A.buf[1] : A.buf[0];
    if (tid == 0) s_keys = 0;
    __syncthreads();
    uint32_t differs = 0;
    if (i < n) {
        const MtEnt e = src[i];
        A.order[i] = e.idx;
        differs = i == 0 ? 1u : mt_cmp_keys(A, src[i - 1], e) != 0;
    }
    const uint32_t c = static_cast<uint32_t>(__builtin_popcountll(__ballot(differs)));
    if ((tid & 63u) == 0 && c) atomicAdd(&s_keys, c);
    __syncthreads();
    if (tid == 0 && s_keys) atomicAdd(&A.head->user_keys, static_cast<unsigned long long>(s_keys));
}

// Kernel 4 (one thread): the totals.
__global__ void mt_totals(const MtArgs A) {
    uint32_t status;
    const uint64_t n = mt_entries(A, &status);
    if (!status && A.head->bad) status = LV_MT_BUILD_BAD_OP;
    lv_mt_totals t;
    t.entries = status & LV_MT_BUILD_UPSTREAM ? 0ull : status & LV_MT_BUILD_OP_OVER ? *A.n_ops : n;
    t.user_keys = status ? 0ull : A.head->user_keys;
    t.status = status;
    *A.totals = t;
}

struct MtGetArgs {
    const uint8_t *payload;
    uint64_t payload_bytes;
    const lv_wb_op *ops;
    const uint32_t *order;
    const lv_mt_totals *totals;
    const uint8_t *qkeys;
    uint64_t qkeys_bytes;
    const uint64_t *q_off;
    const uint32_t *q_len;
    const uint64_t *q_seq;
    uint64_t nq;
    lv_mt_get_result *results;
};

// MemTable::get, one lane per query.
__global__ __launch_bounds__(kMtThreads) void mt_get(const MtGetArgs G) {
    const uint64_t q = static_cast<uint64_t>(blockIdx.x) * kMtThreads + threadIdx.x;
    if (q >= G.nq) return;
    lv_mt_get_result r;
    r.val_off = 0;
    r.val_len = 0;
    r.op = 0;
    r.status = LV_MT_GET_ABSENT;
    r.reserved = 0;
    const uint64_t entries = G.totals->entries, seq = G.q_seq[q];
    const uint64_t qo = G.q_off[q];
    const uint32_t ql = G.q_len[q];
    if (G.totals->status || (entries && !G.ops)) {
        r.status = LV_MT_GET_NO_TABLE;
    } else if (seq > LV_MT_MAX_SEQUENCE) {
        r.status = LV_MT_GET_BAD_SEQ;
    } else if (!extent_ok(qo, ql, G.qkeys_bytes)) {
        r.status = LV_MT_GET_BAD_QUERY;
    } else {
        const uint8_t *qk = G.qkeys + qo;
        const uint64_t qtag = (seq << 8) | LV_WB_TYPE_VALUE;
        uint64_t lo = 0, hi = entries;  // the first entry not less than (qk, qtag)
        bool ok = true;
        for (uint32_t it = 0; it < 64 && lo < hi; ++it) {
            const uint64_t mid = lo + (hi - lo) / 2;
            const lv_wb_op o = load_op(G.ops + G.order[mid]);
            if (!extent_ok(o.key_off, o.key_len, G.payload_bytes)) {  // not the build's arguments
                ok = false;
                break;
            }
            const int c = cmp_bytes(G.payload + o.key_off, o.key_len, qk, ql);
            if (c < 0 || (c == 0 && o.tag > qtag))
                lo = mid + 1;
            else
                hi = mid;
        }
        if (!ok) {
            r.status = LV_MT_GET_NO_TABLE;
        } else if (lo < entries) {
            const uint32_t idx = G.order[lo];
            const lv_wb_op o = load_op(G.ops + idx);
            if (extent_ok(o.key_off, o.key_len, G.payload_bytes) &&
                cmp_bytes(G.payload + o.key_off, o.key_len, qk, ql) == 0) {
                r.op = idx;
                if ((o.tag & 0xffu) == LV_WB_TYPE_VALUE) {
                    r.status = LV_MT_GET_FOUND;
                    r.val_off = o.val_off;
                    r.val_len = o.val_len;
                } else {
                    r.status = LV_MT_GET_DELETED;
                }
            }
        }
    }
    G.results[q] = r;
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxOpCap = 0xfffffffeull;

// The workspace for op_cap = cap, region by region: fills A's workspace pointers.
void mt_carve(Carve &C, uint64_t cap, lvk::MtArgs &A) {
    A.head = C.take<lvk::MtHead>(1);
    A.buf[0] = C.take<lvk::MtEnt>(cap);
    A.buf[1] = C.take<lvk::MtEnt>(cap);
}

}  // namespace

extern "C" {

size_t lv_memtable_build_workspace_bytes(size_t op_cap) {
    if (op_cap > kMaxOpCap) return 0;
    lvk::MtArgs A{};
    Carve C{nullptr};
    mt_carve(C, op_cap, A);
    return C.at;
}

int lv_memtable_build_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops,
                             const uint64_t *d_n_ops, const uint64_t *d_upstream_status, size_t op_cap,
                             uint32_t *d_order, lv_mt_totals *d_totals, uint32_t flags, void *d_workspace,
                             size_t workspace_bytes, void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (!d_totals) return set_err(LV_ERR_INVALID, "null d_totals");
    if (misaligned(d_totals, 8)) return set_err(LV_ERR_INVALID, "d_totals must be 8-byte aligned");
    if (!d_n_ops) return set_err(LV_ERR_INVALID, "null d_n_ops");
    if (misaligned(d_n_ops, 8)) return set_err(LV_ERR_INVALID, "d_n_ops must be 8-byte aligned");
    if (misaligned(d_upstream_status, 8)) return set_err(LV_ERR_INVALID, "d_upstream_status must be 8-byte aligned");
    if (!d_payload && payload_bytes) return set_err(LV_ERR_INVALID, "null d_payload");
    if (op_cap > kMaxOpCap) return set_err(LV_ERR_INVALID, "op_cap too large for one build (at most 2^32 - 2)");
    if (op_cap && !d_ops) return set_err(LV_ERR_INVALID, "null d_ops");
    if (misaligned(d_ops, 16)) return set_err(LV_ERR_INVALID, "d_ops must be 16-byte aligned");
    if (op_cap && !d_order) return set_err(LV_ERR_INVALID, "null d_order");
    if (misaligned(d_order, 4)) return set_err(LV_ERR_INVALID, "d_order must be 4-byte aligned");
    if (!d_workspace) return set_err(LV_ERR_INVALID, "null workspace");
    if (misaligned(d_workspace, 16)) return set_err(LV_ERR_INVALID, "workspace must be 16-byte aligned");
    lvk::MtArgs A{};
    Carve C{static_cast<uint8_t *>(d_workspace)};
    mt_carve(C, op_cap, A);
    if (workspace_bytes < C.at) return set_err(LV_ERR_INVALID, "workspace too small");
    const uint64_t order_bytes = static_cast<uint64_t>(op_cap) * sizeof(uint32_t);
    if (overlaps(d_order, order_bytes, d_ops, static_cast<uint64_t>(op_cap) * sizeof(lv_wb_op)))
        return set_err(LV_ERR_INVALID, "d_order overlaps d_ops");
    if (overlaps(d_order, order_bytes, d_payload, payload_bytes))
        return set_err(LV_ERR_INVALID, "d_order overlaps d_payload");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    A.payload = d_payload;
    A.payload_bytes = payload_bytes;
    A.ops = d_ops;
    A.n_ops = d_n_ops;
    A.upstream = d_upstream_status;
    A.op_cap = op_cap;
    A.order = d_order;
    A.totals = d_totals;

    const dim3 b(lvk::kMtThreads);
    const uint32_t tiles = static_cast<uint32_t>((static_cast<uint64_t>(op_cap) + lvk::kMtTile - 1) / lvk::kMtTile);
    uint32_t passes = 0;  // the run widths below op_cap
    for (uint64_t run = lvk::kMtTile; run < op_cap; run <<= 1) ++passes;
    hipLaunchKernelGGL(lvk::mt_init, dim3(1), dim3(1), 0, s, A);
    if (tiles) {
        hipLaunchKernelGGL(lvk::mt_tile_sort, dim3(tiles), b, 0, s, A);
        for (uint32_t p = 0; p < passes; ++p) hipLaunchKernelGGL(lvk::mt_merge, dim3(tiles), b, 0, s, A, p);
        const uint32_t og = static_cast<uint32_t>((static_cast<uint64_t>(op_cap) + lvk::kMtThreads - 1) / lvk::kMtThreads);
        hipLaunchKernelGGL(lvk::mt_order, dim3(og), b, 0, s, A);
    }
    hipLaunchKernelGGL(lvk::mt_totals, dim3(1), dim3(1), 0, s, A);
    g_kernel = "mt_init+mt_tile_sort+mt_merge+mt_order+mt_totals";
    return check_launch();
}

int lv_memtable_get_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops,
                           const uint32_t *d_order, const lv_mt_totals *d_totals, const uint8_t *d_qkeys,
                           size_t qkeys_bytes, const uint64_t *d_q_off, const uint32_t *d_q_len,
                           const uint64_t *d_q_seq, size_t nq, lv_mt_get_result *d_results, uint32_t flags,
                           void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (!d_totals) return set_err(LV_ERR_INVALID, "null d_totals");
    if (misaligned(d_totals, 8)) return set_err(LV_ERR_INVALID, "d_totals must be 8-byte aligned");
    if (!d_payload && payload_bytes) return set_err(LV_ERR_INVALID, "null d_payload");
    if (!d_qkeys && qkeys_bytes) return set_err(LV_ERR_INVALID, "null d_qkeys");
    if (misaligned(d_ops, 16)) return set_err(LV_ERR_INVALID, "d_ops must be 16-byte aligned");
    if (misaligned(d_order, 4)) return set_err(LV_ERR_INVALID, "d_order must be 4-byte aligned");
    if (!d_ops != !d_order) return set_err(LV_ERR_INVALID, "null d_ops or d_order (both or neither)");
    if (nq > kMaxOpCap) return set_err(LV_ERR_INVALID, "nq too large for one call (at most 2^32 - 2)");
    if (nq && (!d_q_off || !d_q_len || !d_q_seq)) return set_err(LV_ERR_INVALID, "null query array");
    if (nq && !d_results) return set_err(LV_ERR_INVALID, "null d_results");
    if (misaligned(d_q_off, 8) || misaligned(d_q_seq, 8))
        return set_err(LV_ERR_INVALID, "d_q_off and d_q_seq must be 8-byte aligned");
    if (misaligned(d_q_len, 4)) return set_err(LV_ERR_INVALID, "d_q_len must be 4-byte aligned");
    if (misaligned(d_results, 8)) return set_err(LV_ERR_INVALID, "d_results must be 8-byte aligned");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    if (!nq) return LV_OK;
    lvk::MtGetArgs G{};
    G.payload = d_payload;
    G.payload_bytes = payload_bytes;
    G.ops = d_ops;
    G.order = d_order;
    G.totals = d_totals;
    G.qkeys = d_qkeys;
    G.qkeys_bytes = qkeys_bytes;
    G.q_off = d_q_off;
    G.q_len = d_q_len;
    G.q_seq = d_q_seq;
    G.nq = nq;
    G.results = d_results;
    const uint32_t grid = static_cast<uint32_t>((static_cast<uint64_t>(nq) + lvk::kMtThreads - 1) / lvk::kMtThreads);
    hipLaunchKernelGGL(lvk::mt_get, dim3(grid), dim3(lvk::kMtThreads), 0, static_cast<hipStream_t>(stream), G);
    g_kernel = "mt_get";
    return check_launch();
}

}  // extern "C"
