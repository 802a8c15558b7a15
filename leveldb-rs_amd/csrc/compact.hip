// lv_compact_filter_device: the entries of a sorted memtable quadruple that a
// compaction keeps, as a second order array (include/lvgpu/compact.h;
// csrc/compact.cc is the serial twin, upstream's loop with its state).
//
// Whether an entry is dropped depends on the entry and its predecessor in
// d_order alone (compact.h, "The same, entry by entry"), so the call is a flag,
// scan and compact pass:
//
//   cf_init     one thread: *d_mt_totals (UPSTREAM, entries > op_cap), the
//               ranges (BAD_RANGE), the call's head in the workspace (a kernel,
//               not a memset: the call is a chain of kernel launches, which a
//               graph replays).  With a status the head's n is 0 and every
//               later launch returns at once.
//   cf_flag     a lane per entry, a tile of kCfTile entries per workgroup:
//               d_order[i - 1] and d_order[i] (coalesced), the two ops, both
//               key extents, then the decision: kept, hidden (rule A), a
//               deletion at the base level (rule B) or unparsed.  The four are
//               one word of 16-bit counts, so one tile-local scan in LDS gives
//               the entry's position among the tile's kept ones and the tile's
//               four sums.  A tile that holds a bad index or extent compares
//               nothing.
//   cf_carry    one wave: the exclusive scan of the tiles' kept counts; the
//               status is now final (go), before any byte of d_order_out.
//   cf_scatter  a lane per entry: a kept one writes its op index.
//   cf_keys     a lane per kept entry: its user key against the kept entry
//               before it, as the memtable build counts user_keys.
//   cf_finish   one thread: both totals.
//
// The launch sequence depends only on op_cap.  No workgroup waits on another;
// the only loops are over a key's bytes and the ranges.  Positions are u64.
// The op loads, the extent check, the byte compares and both levels of the
// scan are lvk/stage.h's (load_op, extent_ok, same_bytes, cmp_bytes,
// tile_scan, carry_scan).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lvgpu/compact.h"
#include "../../include/lvgpu/crc32c.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/knobs.h"
#include "lvk/stage.h"

namespace lvk {

constexpr uint32_t kCfTile = LVK_CF_TILE;  // entries per scan tile
constexpr uint32_t kCfThreads = 256;
constexpr uint32_t kCfPer = kCfTile / kCfThreads;
static_assert(kCfTile % kCfThreads == 0, "a tile is whole rounds of a workgroup");
static_assert(kCfTile <= 32768, "a tile's counts fit the 16-bit fields of one scanned word");

// An entry's decision as the word the tile scan sums: four 16-bit counts.
constexpr uint64_t kCfKept = 1ull, kCfHidden = 1ull << 16, kCfDeletion = 1ull << 32, kCfUnparsed = 1ull << 48;

struct CfHead {  // workspace, every field written by cf_init
    uint32_t st0;  // the bits the init decides: UPSTREAM, BAD_RANGE, entries > op_cap
    uint32_t bad;  // cf_flag: an order index or a key extent out of range
    uint32_t go, pad;
    uint64_t entries_in, n;  // as reported; the entries to examine (0 with st0)
    uint64_t kept;           // cf_carry
    unsigned long long hidden, deletions, unparsed, user_keys;
};

struct CfArgs {
    const uint8_t *payload;
    uint64_t payload_bytes;
    const lv_wb_op *ops;
    const uint32_t *order;
    const lv_mt_totals *mt;
    uint64_t op_cap, snapshot;
    const lv_compact_range *ranges;
    uint64_t n_ranges;
    const uint8_t *range_keys;
    uint64_t range_keys_bytes;
    uint32_t *order_out;
    lv_mt_totals *mt_out;
    lv_compact_totals *totals;
    uint32_t flags;
    // workspace
    CfHead *head;
    uint32_t *Kl;  // [op_cap] the kept flags' tile-local inclusive scan
    uint64_t *cK;  // [tiles] the tiles' kept counts, then their exclusive scan
};

__global__ void cf_init(const CfArgs A) {
    CfHead h{};
    h.entries_in = A.mt->entries;
    if (A.mt->status) {
        h.st0 = LV_COMPACT_UPSTREAM;
    } else {
        for (uint64_t r = 0; r < A.n_ranges; ++r) {
            const lv_compact_range g = A.ranges[r];
            if (!extent_ok(g.lo_off, g.lo_len, A.range_keys_bytes) || !extent_ok(g.hi_off, g.hi_len, A.range_keys_bytes) ||
                cmp_bytes(A.range_keys + g.lo_off, g.lo_len, A.range_keys + g.hi_off, g.hi_len) > 0) {
                h.st0 |= LV_COMPACT_BAD_RANGE;
                break;
            }
        }
        if (h.entries_in > A.op_cap) h.st0 |= LV_COMPACT_BAD_INPUT;
    }
    if (!h.st0) h.n = h.entries_in;
    *A.head = h;
}

// IsBaseLevelForKey: no range holds k.  The ranges are cf_init's: in bounds.
__device__ __forceinline__ bool cf_base_level(const CfArgs &A, const uint8_t *k, uint32_t klen) {
    if (!(A.flags & LV_COMPACT_BASE_LEVEL)) return false;
    for (uint64_t r = 0; r < A.n_ranges; ++r) {
        const lv_compact_range g = A.ranges[r];
        if (cmp_bytes(k, klen, A.range_keys + g.lo_off, g.lo_len) >= 0 &&
            cmp_bytes(k, klen, A.range_keys + g.hi_off, g.hi_len) <= 0)
            return false;
    }
    return true;
}

__global__ __launch_bounds__(kCfThreads) void cf_flag(const CfArgs A) {
    __shared__ uint64_t s[kCfTile];
    const uint32_t tid = threadIdx.x;
    CfHead *h = A.head;
    const uint64_t n = h->n, base = static_cast<uint64_t>(blockIdx.x) * kCfTile;
    if (base >= n) return;
    const uint32_t cnt = static_cast<uint32_t>(n - base < kCfTile ? n - base : kCfTile);
    int bad = 0;
#pragma unroll
    for (uint32_t k = 0; k < kCfPer; ++k) {
        const uint32_t j = tid + k * kCfThreads;
        uint64_t v = 0;
        if (j < cnt) {
            const uint64_t i = base + j;
            const uint32_t idx = A.order[i], pidx = i ? A.order[i - 1] : 0;
            if (idx >= A.op_cap || pidx >= A.op_cap) {  // (i > 0 here or n > 0: op_cap > 0, so pidx = 0 passes)
                bad = 1;
            } else {
                const lv_wb_op e = load_op(A.ops + idx);
                const uint32_t type = static_cast<uint32_t>(e.tag & 0xffu);
                if (!extent_ok(e.key_off, e.key_len, A.payload_bytes)) {
                    bad = 1;
                } else if (type > 1) {
                    v = kCfKept | kCfUnparsed;
                } else {
                    const uint8_t *key = A.payload + e.key_off;
                    uint64_t prev_seq = LV_MT_MAX_SEQUENCE;
                    if (i) {
                        const lv_wb_op p = load_op(A.ops + pidx);
                        if ((p.tag & 0xffu) <= 1) {
                            if (!extent_ok(p.key_off, p.key_len, A.payload_bytes))
                                bad = 1;  // (its own lane says so too)
                            else if (same_bytes(A.payload + p.key_off, p.key_len, key, e.key_len))
                                prev_seq = p.tag >> 8;
                        }
                    }
                    if (bad)
                        v = 0;
                    else if (prev_seq <= A.snapshot)
                        v = kCfHidden;
                    else if (type == 0 && (e.tag >> 8) <= A.snapshot && cf_base_level(A, key, e.key_len))
                        v = kCfDeletion;
                    else
                        v = kCfKept;
                }
            }
        }
        s[j] = v;
    }
    if (__syncthreads_or(bad)) {  // the status: this tile's counts go nowhere
        if (tid == 0) atomicOr(&h->bad, 1u);  // (nobody reads it during this launch)
        return;
    }
    tile_scan<kCfTile, kCfThreads>(s, 1, tid);
#pragma unroll
    for (uint32_t k = 0; k < kCfPer; ++k) {
        const uint32_t j = tid + k * kCfThreads;
        if (j < cnt) A.Kl[base + j] = static_cast<uint32_t>(s[j] & 0xffffu);
    }
    if (tid == 0) {
        const uint64_t sum = s[cnt - 1];
        A.cK[blockIdx.x] = sum & 0xffffu;
        if ((sum >> 16) & 0xffffu) atomicAdd(&h->hidden, static_cast<unsigned long long>((sum >> 16) & 0xffffu));
        if ((sum >> 32) & 0xffffu) atomicAdd(&h->deletions, static_cast<unsigned long long>((sum >> 32) & 0xffffu));
        if (sum >> 48) atomicAdd(&h->unparsed, static_cast<unsigned long long>(sum >> 48));
    }
}

// One wave: the tiles' kept counts become their exclusive scan; the status is final.
__global__ __launch_bounds__(64) void cf_carry(const CfArgs A) {
    CfHead *h = A.head;
    if (h->st0 || h->bad) return;  // (wave-uniform)
    const uint32_t lane = threadIdx.x;
    const uint64_t kept = carry_scan(A.cK, 1, (h->n + kCfTile - 1) / kCfTile, lane);
    if (lane == 0) {
        h->kept = kept;
        h->go = 1;
    }
}

__global__ __launch_bounds__(kCfThreads) void cf_scatter(const CfArgs A) {
    const CfHead *h = A.head;
    if (!h->go) return;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCfThreads + threadIdx.x;
    if (i >= h->n) return;
    const uint32_t at = A.Kl[i], before = i % kCfTile ? A.Kl[i - 1] : 0;
    if (at != before) A.order_out[A.cK[i / kCfTile] + at - 1] = A.order[i];  // kept: position < kept <= n <= op_cap
}

// The kept entries' user keys: adjacent ones that differ, plus one for the first.
__global__ __launch_bounds__(kCfThreads) void cf_keys(const CfArgs A) {
    CfHead *h = A.head;
    if (!h->go) return;
    const uint64_t kept = h->kept, j = static_cast<uint64_t>(blockIdx.x) * kCfThreads + threadIdx.x;
    if (static_cast<uint64_t>(blockIdx.x) * kCfThreads >= kept) return;  // the whole workgroup
    bool fresh = false;
    if (j < kept) {
        fresh = j == 0;
        if (j) {  // (cf_flag accepted every index and key extent)
            const lv_wb_op p = load_op(A.ops + A.order_out[j - 1]), e = load_op(A.ops + A.order_out[j]);
            fresh = !same_bytes(A.payload + p.key_off, p.key_len, A.payload + e.key_off, e.key_len);
        }
    }
    const uint64_t f = __ballot(fresh);
    if ((threadIdx.x & 63u) == 0 && f) atomicAdd(&h->user_keys, static_cast<unsigned long long>(__popcll(f)));
}

__global__ void cf_finish(const CfArgs A) {
    const CfHead *h = A.head;
    lv_compact_totals t{};
    t.entries_in = h->entries_in;
    if (h->go) {
        t.kept = h->kept;
        t.dropped_hidden = h->hidden;
        t.dropped_deletions = h->deletions;
        t.unparsed = h->unparsed;
        t.user_keys = h->user_keys;
        *A.mt_out = lv_mt_totals{t.kept, t.user_keys, 0};
    } else {
        t.status = h->st0 ? h->st0 : LV_COMPACT_BAD_INPUT;
        *A.mt_out = lv_mt_totals{0, 0, LV_MT_BUILD_UPSTREAM};
    }
    *A.totals = t;
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxOpCap = 0xfffffffeull;

// The workspace for op_cap = cap, region by region: fills A's workspace
// pointers; returns the tiles.
uint64_t cf_carve(Carve &C, uint64_t cap, lvk::CfArgs &A) {
    const uint64_t tiles = (cap + lvk::kCfTile - 1) / lvk::kCfTile;
    A.head = C.take<lvk::CfHead>(1);
    A.Kl = C.take<uint32_t>(cap);
    A.cK = C.take<uint64_t>(tiles);
    return tiles;
}

}  // namespace

// cf_carry scans 64 tile sums a round (lvk::carry_scan).
uint64_t lvgpu_internal::cf_carry_round() { return 64ull * lvk::kCfTile; }

extern "C" {

size_t lv_compact_filter_workspace_bytes(size_t op_cap) {
    if (op_cap > kMaxOpCap) return 0;
    lvk::CfArgs A{};
    Carve C{nullptr};
    cf_carve(C, op_cap, A);
    return C.at;
}

int lv_compact_filter_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops,
                             const uint32_t *d_order, const lv_mt_totals *d_mt_totals, size_t op_cap,
                             uint64_t smallest_snapshot, const lv_compact_range *d_ranges, size_t n_ranges,
                             const uint8_t *d_range_keys, size_t range_keys_bytes, uint32_t *d_order_out,
                             lv_mt_totals *d_mt_totals_out, lv_compact_totals *d_totals, uint32_t flags,
                             void *d_workspace, size_t workspace_bytes, void *stream) {
    g_err.clear();
    if (flags & ~LV_COMPACT_BASE_LEVEL) return set_err(LV_ERR_INVALID, "unknown flag bits (LV_COMPACT_BASE_LEVEL is defined)");
    if (smallest_snapshot >= LV_MT_MAX_SEQUENCE)
        return set_err(LV_ERR_INVALID, "smallest_snapshot must be below LV_MT_MAX_SEQUENCE");
    if (n_ranges > LV_COMPACT_MAX_RANGES) return set_err(LV_ERR_INVALID, "n_ranges too large (at most 4096)");
    if (n_ranges && !(flags & LV_COMPACT_BASE_LEVEL))
        return set_err(LV_ERR_INVALID, "ranges need LV_COMPACT_BASE_LEVEL");
    if (!d_mt_totals) return set_err(LV_ERR_INVALID, "null d_mt_totals");
    if (!d_mt_totals_out) return set_err(LV_ERR_INVALID, "null d_mt_totals_out");
    if (!d_totals) return set_err(LV_ERR_INVALID, "null d_totals");
    if (misaligned(d_mt_totals, 8) || misaligned(d_mt_totals_out, 8) || misaligned(d_totals, 8))
        return set_err(LV_ERR_INVALID, "d_mt_totals, d_mt_totals_out and d_totals must be 8-byte aligned");
    if (!d_payload && payload_bytes) return set_err(LV_ERR_INVALID, "null d_payload");
    if (op_cap > kMaxOpCap) return set_err(LV_ERR_INVALID, "op_cap too large for one call (at most 2^32 - 2)");
    if (op_cap && !d_ops) return set_err(LV_ERR_INVALID, "null d_ops");
    if (misaligned(d_ops, 16)) return set_err(LV_ERR_INVALID, "d_ops must be 16-byte aligned");
    if (op_cap && (!d_order || !d_order_out)) return set_err(LV_ERR_INVALID, "null d_order or d_order_out");
    if (misaligned(d_order, 4) || misaligned(d_order_out, 4))
        return set_err(LV_ERR_INVALID, "d_order and d_order_out must be 4-byte aligned");
    if (n_ranges && !d_ranges) return set_err(LV_ERR_INVALID, "null d_ranges");
    if (misaligned(d_ranges, 8)) return set_err(LV_ERR_INVALID, "d_ranges must be 8-byte aligned");
    if (!d_range_keys && range_keys_bytes) return set_err(LV_ERR_INVALID, "null d_range_keys");
    if (!d_workspace) return set_err(LV_ERR_INVALID, "null workspace");
    if (misaligned(d_workspace, 16)) return set_err(LV_ERR_INVALID, "workspace must be 16-byte aligned");
    lvk::CfArgs A{};
    Carve C{static_cast<uint8_t *>(d_workspace)};
    const uint64_t tiles = cf_carve(C, op_cap, A);
    if (workspace_bytes < C.at) return set_err(LV_ERR_INVALID, "workspace too small");
    const uint64_t order_bytes = static_cast<uint64_t>(op_cap) * sizeof(uint32_t);
    if (overlaps(d_order_out, order_bytes, d_order, order_bytes))
        return set_err(LV_ERR_INVALID, "d_order_out overlaps d_order");
    if (overlaps(d_order_out, order_bytes, d_ops, static_cast<uint64_t>(op_cap) * sizeof(lv_wb_op)))
        return set_err(LV_ERR_INVALID, "d_order_out overlaps d_ops");
    if (overlaps(d_order_out, order_bytes, d_payload, payload_bytes))
        return set_err(LV_ERR_INVALID, "d_order_out overlaps d_payload");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    A.payload = d_payload;
    A.payload_bytes = payload_bytes;
    A.ops = d_ops;
    A.order = d_order;
    A.mt = d_mt_totals;
    A.op_cap = op_cap;
    A.snapshot = smallest_snapshot;
    A.ranges = d_ranges;
    A.n_ranges = n_ranges;
    A.range_keys = d_range_keys;
    A.range_keys_bytes = range_keys_bytes;
    A.order_out = d_order_out;
    A.mt_out = d_mt_totals_out;
    A.totals = d_totals;
    A.flags = flags;

    const dim3 b(lvk::kCfThreads);
    const uint32_t lanes = static_cast<uint32_t>((static_cast<uint64_t>(op_cap) + lvk::kCfThreads - 1) / lvk::kCfThreads);
    hipLaunchKernelGGL(lvk::cf_init, dim3(1), dim3(1), 0, s, A);
    if (op_cap) hipLaunchKernelGGL(lvk::cf_flag, dim3(static_cast<uint32_t>(tiles)), b, 0, s, A);
    hipLaunchKernelGGL(lvk::cf_carry, dim3(1), dim3(64), 0, s, A);  // (op_cap == 0: go with kept = 0)
    if (op_cap) {
        hipLaunchKernelGGL(lvk::cf_scatter, dim3(lanes), b, 0, s, A);
        hipLaunchKernelGGL(lvk::cf_keys, dim3(lanes), b, 0, s, A);
    }
    hipLaunchKernelGGL(lvk::cf_finish, dim3(1), dim3(1), 0, s, A);
    g_kernel = "cf_init+cf_flag+cf_carry+cf_scatter+cf_keys+cf_finish";
    return check_launch();
}

}  // extern "C"
