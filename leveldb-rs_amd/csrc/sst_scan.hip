// lv_sst_scan_device: an SSTable image in HBM back to an op table with its keys
// and values in an arena: Table::NewIterator walked to the end, every entry at
// once (include/lvgpu/table.h, "Scan"; csrc/sst_scan.cc is the serial twin).
//
// The serial walks are lvk/sst_scan.h, the text the host twin compiles too; this
// file gives them lanes.  The problem is ragged on two levels, blocks x restart
// runs x entries, with a serial chain only inside a run (prefix compression),
// so a block gets a lane, then a run gets a lane:
//
//   ss_header  one thread: *d_prev, *d_table, the index block's header; zeroes
//              the call's head in the workspace (a kernel, not a memset: the
//              call is a chain of kernel launches, which a graph replays).
//   ss_blocks  a lane per data block, a tile of kSsTile blocks per workgroup:
//              the block's handle from its index entry, its type byte and
//              header; the handle goes to the workspace, the run count into a
//              tile-local scan in LDS.
//   ss_carry   the exclusive scan of the tiles' sums, a wave per column: first
//              the run counts (their sum is the table's runs), later the two
//              columns of ss_count.
//   ss_count   a lane per run, a tile of kSsTile runs per workgroup in a
//              grid-stride loop over the tiles: the run's block by binary
//              search over the scanned run counts, the run walked keeping only
//              lengths; entry count and arena bytes into two tile-local scans.
//              The table's totals are atomic sums of the tiles' sums, so they
//              are the true ones even when the runs outnumber the workspace's
//              op_cap + block_cap slots (that table is OP_OVER: a run but an
//              empty block's holds an entry).
//   ss_plan    one thread: every status and every total, once, before any
//              byte of d_arena, d_ops or d_order is written.
//   ss_emit    a lane per run walks it again and writes: the op, the bytes that
//              cross between key and tag, and three copies per entry (the
//              shared prefix from the lane's previous key in the arena, the
//              key suffix and the value from the block).  A copy of
//              kSsWaveCopy bytes or more is the wave's: kSsCopyLanes lanes
//              share it in 16-byte granules of the destination's alignment,
//              64 / kSsCopyLanes such copies at a time (lvk/stage.h's
//              group_copy, which sst_build.hip uses too, with fewer lanes per
//              copy: the values that reach it here are mostly short, and more
//              of them are then in flight).
//              The lanes of a wave step through their runs together, and a
//              workgroup-scope fence closes every step: the next entry's
//              prefix is read from bytes that other lanes of the wave may
//              have stored.
//   ss_order   (d_order) a lane per entry: d_order[i] = i, the entry against
//              its predecessor.
//   ss_finish  (d_order) one thread: *d_mt_totals.
//
// The launch sequence depends only on host values (op_cap, block_cap, whether
// d_order is NULL).  No workgroup waits on another; every loop is bounded by
// the block it walks.  All sizes and positions are u64.
// The tile scans, the carries' wave scan and the op loads and stores are
// lvk/stage.h's too (tile_scan, carry_scan, load_op, store_op).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/table.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/knobs.h"
#include "lvk/sst_scan.h"
#include "lvk/stage.h"

namespace lvk {

constexpr uint32_t kSsTile = LVK_SS_TILE;             // blocks, and runs, per scan tile
constexpr uint32_t kSsWaveCopy = LVK_SS_WAVE_COPY;    // bytes from which a copy is the wave's
constexpr uint32_t kSsCopyLanes = LVK_SS_COPY_LANES;  // lanes of a wave that share one such copy
constexpr uint32_t kSsThreads = 256;
constexpr uint32_t kSsPer = kSsTile / kSsThreads;
constexpr uint32_t kSsMaxGrid = 4096;  // ss_count: the rest is the grid-stride loop's
static_assert(kSsTile % kSsThreads == 0, "a tile is whole rounds of a workgroup");
static_assert(kSsTile * 16 <= 65536, "two u64 scan arrays fit the LDS a workgroup may declare");
static_assert(kSsWaveCopy >= 16, "a wave copy has at least one granule");
static_assert(kSsCopyLanes >= 1 && 64 % kSsCopyLanes == 0, "a wave is whole groups of copy lanes");

struct SsHead {  // workspace, every field written by ss_header
    uint32_t st0;  // the bits the header decides: UPSTREAM, NO_TABLE, CORRUPT, BLOCK_OVER
    uint32_t bad_blocks, bad_runs, go;
    uint64_t fb, io;            // the table's file_bytes and index offset
    uint64_t nblocks, iarr;     // the index block's restarts (0 blocks when there is nothing to examine)
    uint64_t data_blocks;       // as reported
    uint64_t base_e, base_b;
    unsigned long long runs, entries, bytes;  // the table's: ss_carry, ss_count
    unsigned long long unordered, user_keys;  // ss_order
};

struct SsArgs {
    const uint8_t *file;
    uint64_t file_cap;
    const lv_sst_table *table;
    const lv_sst_scan_totals *prev;
    uint8_t *arena;
    uint64_t arena_cap;
    lv_wb_op *ops;
    uint64_t op_cap, block_cap, run_cap, run_tiles;
    uint32_t *order;
    lv_mt_totals *mt;
    lv_sst_scan_totals *totals;
    // workspace
    SsHead *head;
    uint64_t *boff, *bsize;  // [block_cap] the data blocks' handles
    uint64_t *Rl, *cR;       // [block_cap], [tiles]: the run counts' tile-local inclusive scan and carries
    uint64_t *El, *Bl;       // [run_cap] the same of the runs' entry counts and arena bytes
    uint64_t *cE, *cB;       // [run_tiles]
};

__global__ void ss_header(const SsArgs A) {
    SsHead h{};
    if (A.prev) {
        h.base_e = A.prev->entries;
        h.base_b = A.prev->arena_bytes;
        if (A.prev->status) h.st0 |= LV_SST_SCAN_UPSTREAM;
    }
    const uint64_t fb = A.table->file_bytes, io = A.table->index_offset;
    if (A.table->status || fb > A.file_cap) h.st0 |= LV_SST_SCAN_NO_TABLE;
    if (!h.st0 && fb) {
        lvr::Restarts ir;
        if (!lvs::index_header(A.file, fb, io, A.table->index_size, A.table->data_blocks, &ir)) {
            h.st0 = LV_SST_SCAN_CORRUPT;
        } else {
            h.data_blocks = ir.n;
            if (ir.n > A.block_cap) {
                h.st0 = LV_SST_SCAN_BLOCK_OVER;
            } else {
                h.fb = fb;
                h.io = io;
                h.nblocks = ir.n;
                h.iarr = ir.arr;
            }
        }
    }
    *A.head = h;
}

__global__ __launch_bounds__(kSsThreads) void ss_blocks(const SsArgs A) {
    __shared__ uint64_t s_r[kSsTile];
    const uint32_t tid = threadIdx.x;
    const SsHead *h = A.head;
    const uint64_t nb = h->nblocks, base = static_cast<uint64_t>(blockIdx.x) * kSsTile;
    if (base >= nb) return;
    const uint32_t cnt = static_cast<uint32_t>(nb - base < kSsTile ? nb - base : kSsTile);
    const lvr::Restarts ir{nb, h->iarr};
    const uint64_t fb = h->fb, io = h->io;
#pragma unroll
    for (uint32_t k = 0; k < kSsPer; ++k) {
        const uint32_t j = tid + k * kSsThreads;
        uint64_t v = 0;
        if (j < cnt) {
            lvs::Block blk{0, 0, 0, 0};
            if (lvs::block_header(A.file, fb, io, ir, base + j, &blk))
                v = blk.n;
            else
                atomicOr(&A.head->bad_blocks, 1u);  // (nobody reads it during this launch)
            A.boff[base + j] = blk.off;
            A.bsize[base + j] = blk.size;
        }
        s_r[j] = v;
    }
    __syncthreads();
    tile_scan<kSsTile, kSsThreads>(s_r, 1, tid);
#pragma unroll
    for (uint32_t k = 0; k < kSsPer; ++k) {
        const uint32_t j = tid + k * kSsThreads;
        if (j < cnt) A.Rl[base + j] = s_r[j];
    }
    if (tid == 0) A.cR[blockIdx.x] = s_r[cnt - 1];
}

// The exclusive scan over the tiles of a column, in place; one wave per
// column.  which 0: the run counts (their sum is head->runs); 1: the runs'
// entry counts and arena bytes, over the tiles the workspace holds.
__global__ __launch_bounds__(kSsThreads) void ss_carry(const SsArgs A, uint32_t which) {
    const uint32_t lane = threadIdx.x & 63u, c = threadIdx.x >> 6;
    SsHead *h = A.head;
    if (h->bad_blocks) return;
    uint64_t *col;
    uint64_t tiles;
    if (which == 0) {
        if (c > 0) return;
        col = A.cR;
        tiles = (h->nblocks + kSsTile - 1) / kSsTile;
    } else {
        if (c > 1) return;
        col = c ? A.cB : A.cE;
        tiles = (h->runs + kSsTile - 1) / kSsTile;
        if (tiles > A.run_tiles) tiles = A.run_tiles;
    }
    const uint64_t run = carry_scan(col, 1, tiles, lane);
    if (which == 0 && lane == 0) h->runs = run;
}

// Run r < head->runs: its block and its index there.
__device__ __forceinline__ void ss_find(const SsArgs &A, uint64_t nb, uint64_t r, lvs::Block *blk, uint64_t *rl) {
    uint64_t lo = 0, hi = nb - 1;  // the first block whose inclusive run count is above r
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (A.Rl[mid] + A.cR[mid / kSsTile] > r)
            hi = mid;
        else
            lo = mid + 1;
    }
    blk->off = A.boff[lo];
    blk->size = A.bsize[lo];
    lvr::Restarts rs{0, 0};
    lvr::restarts(A.file + blk->off, blk->size, &rs);  // (ss_blocks accepted it)
    blk->n = rs.n;
    blk->arr = rs.arr;
    *rl = r - (A.Rl[lo] + A.cR[lo / kSsTile] - rs.n);
}

__global__ __launch_bounds__(kSsThreads) void ss_count(const SsArgs A) {
    __shared__ uint64_t s_e[kSsTile], s_b[kSsTile];
    const uint32_t tid = threadIdx.x;
    SsHead *h = A.head;
    if (h->bad_blocks) return;
    const uint64_t runs = h->runs, nb = h->nblocks, tiles = (runs + kSsTile - 1) / kSsTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {  // uniform in the workgroup
        const uint64_t base = t * kSsTile;
        const uint32_t cnt = static_cast<uint32_t>(runs - base < kSsTile ? runs - base : kSsTile);
#pragma unroll
        for (uint32_t k = 0; k < kSsPer; ++k) {
            const uint32_t j = tid + k * kSsThreads;
            uint64_t e = 0, b = 0;
            if (j < cnt) {
                lvs::Block blk;
                uint64_t rl;
                ss_find(A, nb, base + j, &blk, &rl);
                if (!lvs::run_count(A.file + blk.off, blk, rl, &e, &b)) {
                    e = b = 0;
                    atomicOr(&h->bad_runs, 1u);  // (nobody reads it during this launch)
                }
            }
            s_e[j] = e;
            s_b[j] = b;
        }
        __syncthreads();
        tile_scan<kSsTile, kSsThreads>(s_e, 1, tid);
        tile_scan<kSsTile, kSsThreads>(s_b, 1, tid);
#pragma unroll
        for (uint32_t k = 0; k < kSsPer; ++k) {
            const uint32_t j = tid + k * kSsThreads;
            if (j < cnt && base + j < A.run_cap) {
                A.El[base + j] = s_e[j];
                A.Bl[base + j] = s_b[j];
            }
        }
        if (tid == 0) {
            if (t < A.run_tiles) {
                A.cE[t] = s_e[cnt - 1];
                A.cB[t] = s_b[cnt - 1];
            }
            atomicAdd(&h->entries, static_cast<unsigned long long>(s_e[cnt - 1]));
            atomicAdd(&h->bytes, static_cast<unsigned long long>(s_b[cnt - 1]));
        }
        __syncthreads();  // the next tile reuses the arrays
    }
}

__global__ void ss_plan(const SsArgs A) {
    SsHead *h = A.head;
    lv_sst_scan_totals t{};
    uint64_t st = h->st0;
    if (!st && (h->bad_blocks || h->bad_runs)) st = LV_SST_SCAN_CORRUPT;
    t.data_blocks = h->data_blocks;
    t.entries = h->base_e;
    t.arena_bytes = h->base_b;
    if (!st) {
        t.table_entries = h->entries;
        t.table_bytes = h->bytes;
        t.runs = h->runs;
        t.entries += t.table_entries;
        t.arena_bytes += t.table_bytes;
        if (lvs::over(h->base_e, t.table_entries, A.op_cap)) st |= LV_SST_SCAN_OP_OVER;
        if (lvs::over(h->base_b, t.table_bytes, A.arena_cap)) st |= LV_SST_SCAN_ARENA_OVER;
    }
    t.status = st;
    if (!st) h->go = 1;
    *A.totals = t;
    if (A.mt && st) *A.mt = lv_mt_totals{0, 0, LV_MT_BUILD_UPSTREAM};
}

// Every lane of a wave stays to the end: the long copies are the wave's.
__global__ __launch_bounds__(kSsThreads) void ss_emit(const SsArgs A) {
    const SsHead *h = A.head;
    if (!h->go) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t runs = h->runs, r = static_cast<uint64_t>(blockIdx.x) * kSsThreads + threadIdx.x;
    if (r - lane >= runs) return;  // the whole wave
    // go: the runs fit the workspace, base_e + entries <= op_cap, base_b + bytes <= arena_cap
    lvs::Walk w{0, 0, 0};
    lvs::Prev p;
    const uint8_t *raw = A.file;
    uint64_t ei = 0, koff = 0;
    if (r < runs) {
        lvs::Block blk;
        uint64_t rl;
        ss_find(A, h->nblocks, r, &blk, &rl);
        raw += blk.off;
        lvs::run_begin(raw, blk, rl, &w);
        const uint64_t t = r / kSsTile;
        ei = h->base_e + A.cE[t] + (r % kSsTile ? A.El[r - 1] : 0);
        koff = h->base_b + A.cB[t] + (r % kSsTile ? A.Bl[r - 1] : 0);
    }
    while (__ballot(!w.done())) {  // wave-uniform
        lvs::Copy jobs[3] = {{nullptr, nullptr, 0}, {nullptr, nullptr, 0}, {nullptr, nullptr, 0}};
        if (!w.done()) {
            lvr::Entry e;
            lv_wb_op op;
            if (lvs::step(raw, &w, &e)) {  // (ss_count accepted the run)
                koff = lvs::emit_entry(raw, e, w.klen, A.arena, koff, &p, &op, jobs);
                store_op(A.ops + ei++, op);
            } else {
                w.at = w.end;  // (an image that changed under the call: the loop still ends)
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j)
            group_copy<kSsCopyLanes, kSsWaveCopy>(jobs[j].dst, jobs[j].src, jobs[j].len, lane);
        __threadfence_block();  // the next entry's prefix: bytes this wave's lanes have just stored
    }
}

__global__ __launch_bounds__(kSsThreads) void ss_order(const SsArgs A) {
    SsHead *h = A.head;
    if (!h->go) return;
    const uint64_t n = h->entries, i = static_cast<uint64_t>(blockIdx.x) * kSsThreads + threadIdx.x;
    bool fresh = false, bad = false;
    if (i < n) {
        A.order[i] = static_cast<uint32_t>(i);
        fresh = i == 0;
        if (i) {
            bool same;
            bad = lvs::op_compare(A.arena, load_op(A.ops + i - 1), load_op(A.ops + i), &same) > 0;
            fresh = !same;
        }
    }
    const uint64_t f = __ballot(fresh), b = __ballot(bad);
    if ((threadIdx.x & 63u) == 0) {
        if (f) atomicAdd(&h->user_keys, static_cast<unsigned long long>(__popcll(f)));
        if (b) atomicAdd(&h->unordered, 1ull);
    }
}

__global__ void ss_finish(const SsArgs A) {
    const SsHead *h = A.head;
    if (!h->go) return;  // (the plan wrote *d_mt_totals)
    *A.mt = h->unordered ? lv_mt_totals{h->entries, 0, LV_SST_SCAN_MT_UNORDERED} : lv_mt_totals{h->entries, h->user_keys, 0};
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxOpCap = 0xfffffffeull;
constexpr uint64_t kMaxBlockCap = 0xfffffffcull;

// The workspace for op_cap and block_cap = bc, region by region: fills A's
// run_cap, run_tiles and workspace pointers; returns the block tiles.
uint64_t ss_carve(Carve &C, uint64_t op_cap, uint64_t bc, lvk::SsArgs &A) {
    const uint64_t btiles = (bc + lvk::kSsTile - 1) / lvk::kSsTile;
    A.run_cap = bc ? op_cap + bc : 0;  // a run but an empty block's holds an entry; no block, no run
    A.run_tiles = (A.run_cap + lvk::kSsTile - 1) / lvk::kSsTile;
    A.head = C.take<lvk::SsHead>(1);
    A.boff = C.take<uint64_t>(bc);
    A.bsize = C.take<uint64_t>(bc);
    A.Rl = C.take<uint64_t>(bc);
    A.cR = C.take<uint64_t>(btiles);
    A.El = C.take<uint64_t>(A.run_cap);
    A.Bl = C.take<uint64_t>(A.run_cap);
    A.cE = C.take<uint64_t>(A.run_tiles);
    A.cB = C.take<uint64_t>(A.run_tiles);
    return btiles;
}

}  // namespace

// ss_count: a workgroup takes a tile of kSsTile restart runs a trip (runs <= run_cap = op_cap + block_cap).
uint64_t lvgpu_internal::ss_count_grid(uint64_t runs, uint64_t *per_trip) {
    if (per_trip) *per_trip = lvk::kSsTile;
    return std::min<uint64_t>((runs + lvk::kSsTile - 1) / lvk::kSsTile, lvk::kSsMaxGrid);
}

// ss_carry scans 64 tile sums a round (lvk::carry_scan).
uint64_t lvgpu_internal::ss_carry_round() { return 64ull * lvk::kSsTile; }

extern "C" {

size_t lv_sst_scan_workspace_bytes(size_t op_cap, size_t block_cap) {
    if (op_cap > kMaxOpCap || block_cap > kMaxBlockCap) return 0;
    lvk::SsArgs A{};
    Carve C{nullptr};
    ss_carve(C, op_cap, block_cap, A);
    return C.at;
}

int lv_sst_scan_device(const uint8_t *d_file, uint64_t file_cap, const lv_sst_table *d_table,
                       const lv_sst_scan_totals *d_prev, uint8_t *d_arena, uint64_t arena_cap, lv_wb_op *d_ops,
                       size_t op_cap, size_t block_cap, uint32_t *d_order, lv_mt_totals *d_mt_totals,
                       lv_sst_scan_totals *d_totals, uint32_t flags, void *d_workspace, size_t workspace_bytes,
                       void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (!d_table) return set_err(LV_ERR_INVALID, "null d_table");
    if (misaligned(d_table, 8)) return set_err(LV_ERR_INVALID, "d_table must be 8-byte aligned");
    if (!d_totals) return set_err(LV_ERR_INVALID, "null d_totals");
    if (misaligned(d_totals, 8)) return set_err(LV_ERR_INVALID, "d_totals must be 8-byte aligned");
    if (misaligned(d_prev, 8)) return set_err(LV_ERR_INVALID, "d_prev must be 8-byte aligned");
    if (d_prev == d_totals) return set_err(LV_ERR_INVALID, "d_prev must not be d_totals");
    if (!d_order != !d_mt_totals) return set_err(LV_ERR_INVALID, "d_order and d_mt_totals go together");
    if (d_order && d_prev) return set_err(LV_ERR_INVALID, "d_order needs a NULL d_prev (an appended table is not sorted)");
    if (misaligned(d_order, 4)) return set_err(LV_ERR_INVALID, "d_order must be 4-byte aligned");
    if (misaligned(d_mt_totals, 8)) return set_err(LV_ERR_INVALID, "d_mt_totals must be 8-byte aligned");
    if (!d_file && file_cap) return set_err(LV_ERR_INVALID, "null d_file");
    if (!d_arena && arena_cap) return set_err(LV_ERR_INVALID, "null d_arena");
    if (op_cap > kMaxOpCap) return set_err(LV_ERR_INVALID, "op_cap too large for one scan (at most 2^32 - 2)");
    if (block_cap > kMaxBlockCap) return set_err(LV_ERR_INVALID, "block_cap too large for one scan (at most 2^32 - 4)");
    if (op_cap && !d_ops) return set_err(LV_ERR_INVALID, "null d_ops");
    if (misaligned(d_ops, 16)) return set_err(LV_ERR_INVALID, "d_ops must be 16-byte aligned");
    if (!d_workspace) return set_err(LV_ERR_INVALID, "null workspace");
    if (misaligned(d_workspace, 16)) return set_err(LV_ERR_INVALID, "workspace must be 16-byte aligned");
    lvk::SsArgs A{};
    Carve C{static_cast<uint8_t *>(d_workspace)};
    const uint64_t btiles = ss_carve(C, op_cap, block_cap, A);
    if (workspace_bytes < C.at) return set_err(LV_ERR_INVALID, "workspace too small");
    const struct {
        const void *p;
        uint64_t bytes;
        const char *name;
    } bufs[4] = {{d_file, file_cap, "d_file"},
                 {d_arena, arena_cap, "d_arena"},
                 {d_ops, static_cast<uint64_t>(op_cap) * sizeof(lv_wb_op), "d_ops"},
                 {d_order, d_order ? static_cast<uint64_t>(op_cap) * sizeof(uint32_t) : 0, "d_order"}};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (overlaps(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes))
                return set_err(LV_ERR_INVALID, std::string(bufs[j].name) + " overlaps " + bufs[i].name);
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    A.file = d_file;
    A.file_cap = file_cap;
    A.table = d_table;
    A.prev = d_prev;
    A.arena = d_arena;
    A.arena_cap = arena_cap;
    A.ops = d_ops;
    A.op_cap = op_cap;
    A.block_cap = block_cap;
    A.order = d_order;
    A.mt = d_mt_totals;
    A.totals = d_totals;

    const dim3 b(lvk::kSsThreads);
    hipLaunchKernelGGL(lvk::ss_header, dim3(1), dim3(1), 0, s, A);
    if (block_cap) {  // (no block: a table with entries is BLOCK_OVER)
        hipLaunchKernelGGL(lvk::ss_blocks, dim3(static_cast<uint32_t>(btiles)), b, 0, s, A);
        hipLaunchKernelGGL(lvk::ss_carry, dim3(1), b, 0, s, A, 0u);
        hipLaunchKernelGGL(lvk::ss_count, dim3(static_cast<uint32_t>(lvgpu_internal::ss_count_grid(A.run_cap))), b, 0, s, A);
        hipLaunchKernelGGL(lvk::ss_carry, dim3(1), b, 0, s, A, 1u);
    }
    hipLaunchKernelGGL(lvk::ss_plan, dim3(1), dim3(1), 0, s, A);
    if (block_cap && op_cap) {
        const uint64_t eg = (A.run_cap + lvk::kSsThreads - 1) / lvk::kSsThreads;
        hipLaunchKernelGGL(lvk::ss_emit, dim3(static_cast<uint32_t>(eg)), b, 0, s, A);
    }
    if (d_order) {
        if (block_cap && op_cap) {
            const uint64_t og = (static_cast<uint64_t>(op_cap) + lvk::kSsThreads - 1) / lvk::kSsThreads;
            hipLaunchKernelGGL(lvk::ss_order, dim3(static_cast<uint32_t>(og)), b, 0, s, A);
        }
        hipLaunchKernelGGL(lvk::ss_finish, dim3(1), dim3(1), 0, s, A);
    }
    g_kernel = d_order ? "ss_header+ss_blocks+ss_carry+ss_count+ss_plan+ss_emit+ss_order+ss_finish"
                       : "ss_header+ss_blocks+ss_carry+ss_count+ss_plan+ss_emit";
    return check_launch();
}

}  // extern "C"
