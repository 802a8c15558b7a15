// lv_memtable_range_device: DBIter's forward walk (Seek, Next*) for a batch of
// range queries over a sorted memtable quadruple (include/lvgpu/memtable.h,
// "Range").
//
//   mt_range   one wave64 per query, four queries per workgroup, the grid
//              ceil(nq / 4): no grid-stride loop, no LDS, no barrier.
//
// The seeks.  start and end are lower bounds over d_order.  A wave searches
// together: each step kMrFan lanes probe evenly spaced pivots of the interval,
// a ballot of "pivot < target" picks the run between two neighbouring pivots,
// and an interval of at most kMrFan entries is probed whole.  The interval
// shrinks (kMrFan + 1)-fold per step.  A larger fan means fewer dependent round
// trips and more cache lines per query (three per pivot: the order word, the
// op, the key); measured over 512 K entries, 8 pivots beat both the binary
// search (fan 1) and a pivot per lane (fan 64) wherever the seek matters
// (lvk/knobs.h, profiles/r18/mt_range/).  On a sorted order the "less" bits
// are a prefix of the pivots and the result is the partition point, the serial
// search's; on any order the interval only shrinks and the trips are bounded.
//
// The walk.  Windows of up to 64 consecutive positions, cut by end and by
// max_scan - examined; lane j owns position p + j.  With the ballots H (group
// starts: the user key differs from the predecessor's), U (type > 1),
// V (parsed and seq <= s) and T (type == 1), the serial loop's `seen` at lane
// j is "a V bit lies in [g, j)", g the last H bit at or below j, or, for a
// lane whose group began before the window, "a V bit lies in [0, j), or the
// carried seen".  A lane in V with seen false decides its group; it is a hit
// iff it is in T.  A hit's rank is count + popc(hits below it); the lane that
// holds the limit-th hit ends the walk.
//
// Every order index and key extent is checked before a byte is read; every
// store is a plain vector store, lane 0 writes the result.  Positions are u64.
#include <hip/hip_runtime.h>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/memtable.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/knobs.h"
#include "lvk/stage.h"

namespace lvk {

constexpr uint32_t kMrThreads = 256;
constexpr uint32_t kMrWaves = kMrThreads / 64;  // queries per workgroup
constexpr uint32_t kMrFan = LVK_MR_SEEK_FAN;    // pivots a wave probes per search step (1: a binary search)
constexpr uint32_t kMrSteps = 40;               // 2^33 > 2^32 entries: a search never needs more, whatever the fan
static_assert(kMrFan >= 1 && kMrFan <= 64, "a pivot per lane at most");

struct MrArgs {
    const uint8_t *payload;
    uint64_t payload_bytes;
    const lv_wb_op *ops;
    const uint32_t *order;
    const lv_mt_totals *totals;
    uint64_t op_cap;
    const uint8_t *qkeys;
    uint64_t qkeys_bytes;
    const lv_mt_range_query *queries;
    uint64_t nq;
    uint32_t limit;
    uint64_t max_scan;
    uint32_t *hits;
    lv_mt_range_result *results;
};

// The bits of lanes below j, and of lanes up to and including j (j < 64).
__device__ __forceinline__ uint64_t mr_below(uint32_t j) { return (1ull << j) - 1; }
__device__ __forceinline__ uint64_t mr_upto(uint32_t j) { return (2ull << j) - 1; }

// Entry `pos` of the order: its op index and op.  False if the index or the
// key extent is out of range (nothing behind either is then read).
__device__ __forceinline__ bool mr_entry(const MrArgs &A, uint64_t pos, uint32_t *idx, lv_wb_op *o) {
    *idx = A.order[pos];
    if (*idx >= A.op_cap) return false;
    *o = load_op(A.ops + *idx);
    return extent_ok(o->key_off, o->key_len, A.payload_bytes);
}

// The first position in [0, n) whose entry is not less than (key, tag), or,
// with kTag false, whose user key is >= key.  The whole wave calls it with
// wave-uniform arguments; *bad is set (wave-uniform) if a probe met an entry
// out of range.
template <bool kTag>
__device__ __forceinline__ uint64_t mr_lower(const MrArgs &A, uint64_t n, const uint8_t *key, uint32_t len, uint64_t tag,
                                             uint32_t lane, bool *bad) {
    uint64_t lo = 0, hi = n;
    for (uint32_t it = 0; it < kMrSteps && lo < hi; ++it) {
        // kMrFan pivots cut [lo, hi) into kMrFan + 1 runs of `step` entries (the last one shorter):
        // lane j's pivot is the last position of run j.  A span of at most kMrFan entries is probed whole.
        const uint64_t span = hi - lo;
        const uint64_t step = (span + kMrFan) / (kMrFan + 1);
        const uint64_t pv = lo + (static_cast<uint64_t>(lane) + 1) * step - 1;
        const bool live = lane < kMrFan && pv < hi;
        bool less = false, broken = false;
        if (live) {
            uint32_t idx;
            lv_wb_op o;
            if (!mr_entry(A, pv, &idx, &o)) {
                broken = true;
            } else {
                const int c = cmp_bytes(A.payload + o.key_off, o.key_len, key, len);
                less = c < 0 || (kTag && c == 0 && o.tag > tag);
            }
        }
        if (__ballot(broken)) {
            *bad = true;
            return 0;
        }
        const uint64_t live_m = __ballot(live);
        const uint64_t geq = live_m & ~__ballot(less);  // live pivots that are not less
        // c = the pivots in front of the first one that is not less
        const uint32_t c = geq ? static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(geq)) - 1)
                               : static_cast<uint32_t>(__popcll(live_m));
        const uint64_t nlo = lo + static_cast<uint64_t>(c) * step;                       // behind pivot c - 1
        const uint64_t nhi = geq ? lo + (static_cast<uint64_t>(c) + 1) * step - 1 : hi;  // pivot c itself
        lo = nlo;
        hi = nhi;
    }
    return lo;
}

__global__ __launch_bounds__(kMrThreads) void mt_range(const MrArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t q = static_cast<uint64_t>(blockIdx.x) * kMrWaves + (threadIdx.x >> 6);
    if (q >= A.nq) return;  // the whole wave
    const lv_mt_range_query Q = A.queries[q];
    const uint64_t n = A.totals->entries, s = Q.seq;
    const bool resume = Q.flags & LV_MT_RANGE_RESUME, has_hi = Q.flags & LV_MT_RANGE_HAS_HI;
    lv_mt_range_result r;
    r.seek_pos = r.next_pos = r.unparsed = 0;
    r.count = r.seen = r.reserved = 0;
    r.status = LV_MT_RANGE_DONE;
    if (A.totals->status || n > A.op_cap || (n && (!A.ops || !A.order))) {
        r.status = LV_MT_GET_NO_TABLE;
    } else if (s > LV_MT_MAX_SEQUENCE) {
        r.status = LV_MT_GET_BAD_SEQ;
    } else if ((Q.flags & ~(LV_MT_RANGE_HAS_HI | LV_MT_RANGE_RESUME | LV_MT_RANGE_SEEN)) ||
               ((Q.flags & LV_MT_RANGE_SEEN) && !resume) ||
               (!resume && !extent_ok(Q.lo_off, Q.lo_len, A.qkeys_bytes)) ||
               (has_hi && !extent_ok(Q.hi_off, Q.hi_len, A.qkeys_bytes)) || (resume && Q.pos > n)) {
        r.status = LV_MT_GET_BAD_QUERY;
    }
    if (r.status) {
        if (lane == 0) A.results[q] = r;
        return;
    }
    bool bad = false;
    uint64_t start = Q.pos, end = n;
    if (!resume) start = mr_lower<true>(A, n, A.qkeys + Q.lo_off, Q.lo_len, (s << 8) | LV_WB_TYPE_VALUE, lane, &bad);
    if (has_hi && !bad) end = mr_lower<false>(A, n, A.qkeys + Q.hi_off, Q.hi_len, 0, lane, &bad);

    uint32_t *slot = A.hits + q * A.limit;
    bool seen = resume && (Q.flags & LV_MT_RANGE_SEEN);
    uint64_t p = start, examined = 0, unparsed = 0;
    uint32_t count = 0, status = LV_MT_RANGE_DONE;
    while (!bad) {  // wave-uniform; at most ceil(max_scan / 64) + 1 trips
        if (count == A.limit) {
            status = LV_MT_RANGE_MORE_LIMIT;
            break;
        }
        if (p >= end) break;
        if (examined == A.max_scan) {
            status = LV_MT_RANGE_MORE_SCAN;
            break;
        }
        uint64_t w64 = end - p < A.max_scan - examined ? end - p : A.max_scan - examined;
        const uint32_t w = w64 < 64 ? static_cast<uint32_t>(w64) : 64u;  // >= 1
        const bool act = lane < w;
        uint32_t idx = 0;
        lv_wb_op o{};
        bool broken = false;
        if (act) broken = !mr_entry(A, p + lane, &idx, &o);
        // the predecessor: the lane below, or for lane 0 position p - 1
        uint64_t pk_off = __shfl(static_cast<unsigned long long>(o.key_off), (lane + 63u) & 63u, 64);
        uint32_t pk_len = __shfl(o.key_len, (lane + 63u) & 63u, 64);
        bool pbroken = __shfl(static_cast<int>(broken), (lane + 63u) & 63u, 64) != 0;
        bool first = false;  // position 0 has no predecessor
        if (lane == 0) {
            first = p == 0;
            pbroken = false;
            if (!first) {
                uint32_t pi;
                lv_wb_op po{};
                pbroken = !mr_entry(A, p - 1, &pi, &po);
                pk_off = po.key_off;
                pk_len = po.key_len;
            }
        }
        broken = act && (broken || pbroken);
        bool h = false;
        if (act && !broken)
            h = first || !same_bytes(A.payload + pk_off, pk_len, A.payload + o.key_off, o.key_len);
        const uint32_t type = static_cast<uint32_t>(o.tag & 0xffu);
        const bool u = act && type > LV_WB_TYPE_VALUE;
        const bool v = act && !u && (o.tag >> 8) <= s;
        const uint64_t B = __ballot(broken), H = __ballot(h), U = __ballot(u), V = __ballot(v);
        // seen in front of this lane: a V bit since its group's start, or the carry
        const uint64_t below = mr_below(lane);
        const uint64_t hb = H & (below | (1ull << lane));
        bool before;
        if (hb) {
            const uint32_t g = 63u - static_cast<uint32_t>(__clzll(static_cast<long long>(hb)));
            before = (V & below & ~mr_below(g)) != 0;
        } else {
            before = seen || (V & below) != 0;
        }
        const bool hit = v && !before && type == LV_WB_TYPE_VALUE;
        const uint64_t hits_m = __ballot(hit);
        const uint32_t rank = count + static_cast<uint32_t>(__popcll(hits_m & below));
        const uint32_t total = static_cast<uint32_t>(__popcll(hits_m));
        // the lane of the limit-th hit, if this window holds it (limit - count >= 1)
        const uint64_t last_m = __ballot(hit && rank == A.limit - 1);
        if (last_m) {
            const uint32_t L = static_cast<uint32_t>(__ffsll(static_cast<unsigned long long>(last_m)) - 1);
            if (B & mr_upto(L)) {
                bad = true;
                break;
            }
            if (hit && rank < A.limit) slot[rank] = idx;
            count = A.limit;
            p += static_cast<uint64_t>(L) + 1;
            unparsed += static_cast<uint64_t>(__popcll(U & mr_upto(L)));
            seen = true;
            continue;  // MORE_LIMIT at the top
        }
        if (B) {
            bad = true;
            break;
        }
        if (hit) slot[rank] = idx;  // rank < limit: the window holds fewer than limit - count hits
        count += total;
        unparsed += static_cast<uint64_t>(__popcll(U));
        if (H) {
            const uint32_t g = 63u - static_cast<uint32_t>(__clzll(static_cast<long long>(H)));
            seen = (V & ~mr_below(g)) != 0;
        } else {
            seen = seen || V != 0;
        }
        p += w;
        examined += w;
    }
    if (bad) {
        r.status = LV_MT_GET_NO_TABLE;
    } else {
        r.seek_pos = start;
        r.next_pos = p;
        r.unparsed = unparsed;
        r.count = count;
        r.status = status;
        r.seen = seen ? 1u : 0u;
    }
    if (lane == 0) A.results[q] = r;
}

}  // namespace lvk

using namespace lvh;

namespace {
constexpr uint64_t kMaxQueries = 0xfffffffeull;
constexpr uint64_t kMaxHits = 1ull << 40;
}  // namespace

extern "C" {

int lv_memtable_range_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops,
                             const uint32_t *d_order, const lv_mt_totals *d_totals, size_t op_cap,
                             const uint8_t *d_qkeys, size_t qkeys_bytes, const lv_mt_range_query *d_queries, size_t nq,
                             uint32_t limit, uint64_t max_scan, uint32_t *d_hits, lv_mt_range_result *d_results,
                             uint32_t flags, void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (!d_totals) return set_err(LV_ERR_INVALID, "null d_totals");
    if (misaligned(d_totals, 8)) return set_err(LV_ERR_INVALID, "d_totals must be 8-byte aligned");
    if (!d_payload && payload_bytes) return set_err(LV_ERR_INVALID, "null d_payload");
    if (!d_qkeys && qkeys_bytes) return set_err(LV_ERR_INVALID, "null d_qkeys");
    if (misaligned(d_ops, 16)) return set_err(LV_ERR_INVALID, "d_ops must be 16-byte aligned");
    if (misaligned(d_order, 4)) return set_err(LV_ERR_INVALID, "d_order must be 4-byte aligned");
    if (!d_ops != !d_order) return set_err(LV_ERR_INVALID, "null d_ops or d_order (both or neither)");
    if (op_cap > kMaxQueries) return set_err(LV_ERR_INVALID, "op_cap too large (at most 2^32 - 2)");
    if (!limit) return set_err(LV_ERR_INVALID, "limit must be at least 1");
    if (!max_scan) return set_err(LV_ERR_INVALID, "max_scan must be at least 1");
    if (nq > kMaxQueries) return set_err(LV_ERR_INVALID, "nq too large for one call (at most 2^32 - 2)");
    const uint64_t slots = static_cast<uint64_t>(nq) * limit;  // < 2^64: both factors are below 2^32
    if (slots > kMaxHits) return set_err(LV_ERR_INVALID, "nq * limit too large for one call (at most 2^40)");
    if (nq && !d_queries) return set_err(LV_ERR_INVALID, "null d_queries");
    if (nq && !d_hits) return set_err(LV_ERR_INVALID, "null d_hits");
    if (nq && !d_results) return set_err(LV_ERR_INVALID, "null d_results");
    if (misaligned(d_queries, 8)) return set_err(LV_ERR_INVALID, "d_queries must be 8-byte aligned");
    if (misaligned(d_hits, 4)) return set_err(LV_ERR_INVALID, "d_hits must be 4-byte aligned");
    if (misaligned(d_results, 8)) return set_err(LV_ERR_INVALID, "d_results must be 8-byte aligned");
    const uint64_t hit_bytes = slots * sizeof(uint32_t), res_bytes = static_cast<uint64_t>(nq) * sizeof(lv_mt_range_result);
    if (overlaps(d_hits, hit_bytes, d_results, res_bytes)) return set_err(LV_ERR_INVALID, "d_hits overlaps d_results");
    const struct {
        const void *p;
        uint64_t bytes;
        const char *name;
    } in[] = {{d_payload, payload_bytes, "d_payload"},
              {d_ops, d_ops ? static_cast<uint64_t>(op_cap) * sizeof(lv_wb_op) : 0, "d_ops"},
              {d_order, d_order ? static_cast<uint64_t>(op_cap) * sizeof(uint32_t) : 0, "d_order"},
              {d_totals, sizeof(lv_mt_totals), "d_totals"},
              {d_qkeys, qkeys_bytes, "d_qkeys"},
              {d_queries, static_cast<uint64_t>(nq) * sizeof(lv_mt_range_query), "d_queries"}};
    for (const auto &x : in) {
        if (overlaps(d_hits, hit_bytes, x.p, x.bytes))
            return set_err(LV_ERR_INVALID, std::string("d_hits overlaps ") + x.name);
        if (overlaps(d_results, res_bytes, x.p, x.bytes))
            return set_err(LV_ERR_INVALID, std::string("d_results overlaps ") + x.name);
    }
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    if (!nq) return LV_OK;
    lvk::MrArgs A{};
    A.payload = d_payload;
    A.payload_bytes = payload_bytes;
    A.ops = d_ops;
    A.order = d_order;
    A.totals = d_totals;
    A.op_cap = op_cap;
    A.qkeys = d_qkeys;
    A.qkeys_bytes = qkeys_bytes;
    A.queries = d_queries;
    A.nq = nq;
    A.limit = limit;
    A.max_scan = max_scan;
    A.hits = d_hits;
    A.results = d_results;
    const uint32_t grid = static_cast<uint32_t>((static_cast<uint64_t>(nq) + lvk::kMrWaves - 1) / lvk::kMrWaves);
    hipLaunchKernelGGL(lvk::mt_range, dim3(grid), dim3(lvk::kMrThreads), 0, static_cast<hipStream_t>(stream), A);
    g_kernel = "mt_range";
    return check_launch();
}

}  // extern "C"
