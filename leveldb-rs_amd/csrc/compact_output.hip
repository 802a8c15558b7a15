// lv_compact_output_device: the output of a compaction, the sorted (and
// filtered) memtable quadruple, written as a run of table images in one arena
// in HBM, with the lv_sst_table, lv_sst_bloom and lv_version_file records of
// every image (include/lvgpu/compact.h has the contract; csrc/compact_output.cc
// is the serial twin).
//
// A file is cut directly after an add that flushed a block, so a file's first
// block starts with an empty builder as every block does: the block starts of
// the run are those of the one-file build, and the call begins as
// lv_sst_build_device does (sst_build.hip: sb_init ... sb_layout and its
// carry, launched from here as they are).  Behind them:
//
//   co_blocks  a lane per entry: a block start stores its first entry and B,
//              the inclusive scan of raw + 5, by block id.
//   co_fnext   fnext(b) for every block b: the file that starts at b ends with
//              the first block e >= b with B[e] - B[b - 1] >= max_file_bytes (a
//              bounded binary search), fnext(b) = e + 1.
//   co_freach  one doubling pass over the blocks (sb_reach's, lvk/sst_build.h):
//              the true file starts are the blocks reachable from block 0.
//   co_fscan   the tile scan of the file-start flags: a block's file; sb_carry.
//   co_fmark   a file's first block, by file.
//   co_index   per block: its offset in its file, the index entry's size (the
//              last block of a file takes short_successor) and, with a filter
//              policy, whether it is the first block of a 2 KiB window of its
//              file's offsets, the window's keys and its filter's size -> tile
//              scans by block id; sb_carry.
//   co_files   per file: its blocks, entries, and the sizes of everything
//              behind its data blocks (BLOCK_LARGE) -> tile scans of the bytes
//              rounded up to 16, the bound keys' bytes and the windows;
//              sb_carry.
//   co_plan    one thread: the totals and the status, once, before any byte of
//              any output but the totals is written.
//   co_emit    sb_emit's body with a block's place taken through its file.
//   sb_bloom_emit, sb_bloom_big, sb_bloom_offsets  as in the build, a filter's
//              and a window's place taken through its file.
//   co_handles a lane per handle pair: d_handles (file-relative) and the
//              workspace copy the seal reads (absolute in the arena: every data
//              block, then a metaindex block per file, padded with {2^64 - 1, 0}).
//   co_file_tail  a lane per file: the filter block's end, the metaindex block,
//              the index's count, the footer, the file's last handle pairs, its
//              records and bound keys, and its two buffers of the CRC batch.
//   the seal, then one batch of the offsets API over the index and filter blocks
//   of all files, and co_trailer, a lane per file.
//
// The launch sequence and every grid depend only on op_cap, block_cap,
// files_cap, arena_cap == 0, restart_interval and whether there is a filter
// policy.  No workgroup waits on another inside a launch, no lane loops over a
// count of entries, blocks or files, and every search is bounded.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lvgpu/compact.h"
#include "../../include/lvgpu/crc32c.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/sst_build.h"

namespace lvk {

struct CoOut {
    lv_compact_output_file *files;
    lv_sst_table *tables;
    lv_sst_bloom *blooms;
    lv_version_file *vfiles;
    uint8_t *bound_keys;
    uint64_t bound_cap;
    uint64_t *bound_used;
    lv_compact_output_totals *totals;
    uint64_t first_number, images_off;
    uint32_t level;
};

// The blocks, or 0 when there is nothing to lay out.
__device__ __forceinline__ uint64_t co_nblocks(const SbArgs &A) {
    return sb_entries(A) && !A.head->bad ? static_cast<uint64_t>(A.head->nblocks) : 0;
}
__device__ __forceinline__ uint64_t co_raw(const SbArgs &A, uint64_t b) {
    return A.Binc[b] - co_Bbefore(A, b) - LV_SST_TRAILER_SIZE;
}

__global__ __launch_bounds__(kSbThreads) void co_blocks(const SbArgs A) {
    const uint64_t n = sb_entries(A);
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x;
    if (i >= n || A.head->bad || !A.F[i]) return;
    const uint64_t t = i / kSbTile, b = A.Cl[i] + A.cC[t] - 1;  // < n <= op_cap
    A.bstart[b] = static_cast<uint32_t>(i);
    A.Binc[b] = A.Bl[i] + A.cB[t];
}

__global__ __launch_bounds__(kSbThreads) void co_fnext(const SbArgs A) {
    const uint64_t nb = co_nblocks(A);
    const uint64_t b = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x;
    if (b >= nb) return;
    const uint64_t base = co_Bbefore(A, b);
    uint64_t lo = b, hi = nb - 1;
    for (uint32_t it = 0; it < 40 && lo < hi; ++it) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (A.Binc[mid] - base >= A.mf)
            hi = mid;
        else
            lo = mid + 1;
    }
    A.fnx[b] = static_cast<uint32_t>(lo + 1);
    A.FF[b] = b == 0;
}

__global__ __launch_bounds__(kSbThreads) void co_freach(const SbArgs A, uint32_t pass) {
    const uint64_t b = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x;
    sb_reach_pass(co_nblocks(A), b, pass, A.fnx, A.J, A.FF);
}

__global__ __launch_bounds__(kSbThreads) void co_fscan(const SbArgs A) {
    __shared__ uint64_t s_k[kSbTile];
    const uint32_t tid = threadIdx.x;
    const uint64_t nb = co_nblocks(A);
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSbTile;
    if (base >= nb) return;
    const uint32_t cnt = static_cast<uint32_t>(nb - base < kSbTile ? nb - base : kSbTile);
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        s_k[j] = j < cnt && A.FF[base + j] ? 1 : 0;
    }
    __syncthreads();
    tile_scan<kSbTile, kSbThreads>(s_k, 1, tid);
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        if (j < cnt) A.Kl[base + j] = s_k[j];
    }
    if (tid == 0) A.cK[blockIdx.x] = s_k[cnt - 1];
}

__global__ __launch_bounds__(kSbThreads) void co_fmark(const SbArgs A) {
    const uint64_t b = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x;
    if (b >= co_nblocks(A) || !A.FF[b]) return;
    A.fstart[co_file_of(A, b)] = static_cast<uint32_t>(b);
}

__global__ __launch_bounds__(kSbThreads) void co_index(const SbArgs A) {
    __shared__ uint64_t s_i[kSbTile], s_f[kSbTile];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = sb_entries(A), nb = co_nblocks(A);
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSbTile;
    if (base >= nb) return;
    const uint32_t cnt = static_cast<uint32_t>(nb - base < kSbTile ? nb - base : kSbTile);
    uint64_t own[kSbPer];
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        uint64_t v = 0, f = 0;
        if (j < cnt) {
            const uint64_t b = base + j, fb = A.fstart[co_file_of(A, b)], fe = A.fnx[fb];
            const uint64_t fbase = co_Bbefore(A, fb), off = co_Bbefore(A, b) - fbase;
            const uint64_t e = static_cast<uint64_t>(A.nxt[A.bstart[b]]) - 1;
            v = sb_index_entry(A, e, b + 1 == fe, load_op(A.ops + A.order[e]), off, co_raw(A, b)).size;
            if (A.bpk) {
                const uint64_t w = off >> LV_SST_FILTER_BASE_LG;
                uint32_t keys = 0;
                if (b == fb || ((co_Bbefore(A, b - 1) - fbase) >> LV_SST_FILTER_BASE_LG) != w) {
                    const uint64_t lim = (w + 1) << LV_SST_FILTER_BASE_LG;
                    uint64_t lo = b + 1, hi = fe;
                    for (uint32_t it = 0; it < 40 && lo < hi; ++it) {
                        const uint64_t mid = lo + (hi - lo) / 2;
                        if (co_Bbefore(A, mid) - fbase >= lim)
                            hi = mid;
                        else
                            lo = mid + 1;
                    }
                    keys = static_cast<uint32_t>((lo < nb ? A.bstart[lo] : n) - A.bstart[b]);
                    f = sb_bloom_bytes(keys, A.bpk) + 1;  // (sb_bloom_emit tells sb_bloom_big of one beyond its LDS)
                }
                A.Fn[b] = keys;
            }
        }
        own[k] = f;
        s_i[j] = v;
        s_f[j] = f;
    }
    __syncthreads();
    tile_scan<kSbTile, kSbThreads>(s_i, 1, tid);
    if (A.bpk) tile_scan<kSbTile, kSbThreads>(s_f, 1, tid);
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        if (j < cnt) {
            A.Il[base + j] = s_i[j];
            if (A.bpk) A.Fl[base + j] = s_f[j] - own[k];
        }
    }
    if (tid == 0) {
        A.cI[blockIdx.x] = s_i[cnt - 1];
        if (A.bpk) A.cF[blockIdx.x] = s_f[cnt - 1];
    }
}

__global__ __launch_bounds__(kSbThreads) void co_files(const SbArgs A) {
    __shared__ uint64_t s_a[kSbTile], s_u[kSbTile], s_w[kSbTile];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = sb_entries(A), nb = co_nblocks(A);
    const uint64_t nf = nb ? static_cast<uint64_t>(A.ch->nfiles) : 0;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSbTile;
    if (base >= nf) return;
    const uint32_t cnt = static_cast<uint32_t>(nf - base < kSbTile ? nf - base : kSbTile);
    CoFile own[kSbPer];
    uint32_t large = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        CoFile c{};
        uint64_t a = 0;
        if (j < cnt) {
            c.fb = A.fstart[base + j];
            c.fe = A.fnx[c.fb];
            c.first = A.bstart[c.fb];
            const uint64_t end = c.fe < nb ? A.bstart[c.fe] : n, fbase = co_Bbefore(A, c.fb);
            c.entries = static_cast<uint32_t>(end - c.first);
            c.data_bytes = A.Binc[c.fe - 1] - fbase;
            c.idx_bytes = co_Ibefore(A, c.fe) - co_Ibefore(A, c.fb);
            if (A.bpk) {
                const uint64_t last = (co_Bbefore(A, c.fe - 1) - fbase) >> LV_SST_FILTER_BASE_LG;
                const uint64_t ends = c.data_bytes >> LV_SST_FILTER_BASE_LG;
                c.filt_bytes = co_Fbefore(A, c.fe, nb) - co_Fbefore(A, c.fb, nb);
                c.filters = last + 1 > ends ? last + 1 : ends;
            }
            const CoLayout L = co_sizes(A.bpk, c.data_bytes, c.fe - c.fb, c.idx_bytes, c.filt_bytes, c.filters);
            large |= L.index_size >= kSbLarge || (A.bpk && L.filter_size >= kSbLarge);
            a = (L.file_bytes + 15) & ~15ull;
            if (base + j + 1 == nf) A.ch->last_pad = a - L.file_bytes;
            c.small_len = static_cast<uint64_t>(A.ops[A.order[c.first]].key_len) + 8;
            c.large_len = static_cast<uint64_t>(A.ops[A.order[end - 1]].key_len) + 8;
        }
        own[k] = c;
        s_a[j] = a;
        s_u[j] = c.small_len + c.large_len;
        s_w[j] = c.filters;
    }
    if (large) atomicOr(&A.ch->large, 1u);
    __syncthreads();
    tile_scan<kSbTile, kSbThreads>(s_a, 1, tid);
    tile_scan<kSbTile, kSbThreads>(s_u, 1, tid);
    tile_scan<kSbTile, kSbThreads>(s_w, 1, tid);
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        if (j < cnt && base + j < A.files_cap) {
            own[k].Al = s_a[j];
            own[k].Kl = s_u[j];
            own[k].Wl = s_w[j];
            A.cf[base + j] = own[k];
        }
    }
    if (tid == 0) {
        A.cA[blockIdx.x] = s_a[cnt - 1];
        A.cU[blockIdx.x] = s_u[cnt - 1];
        A.cW[blockIdx.x] = s_w[cnt - 1];
    }
}

// One thread: the totals and the status, before any other output is written.
__global__ void co_plan(const SbArgs A, const CoOut O) {
    lv_compact_output_totals t{};
    const uint64_t n = A.mt->entries;
    if (A.mt->status || n > A.op_cap || A.head->bad) {
        t.status = LV_COMPACT_OUT_NO_TABLE;
        *O.totals = t;
        return;
    }
    t.entries = n;
    if (n) {
        const uint64_t extra = A.bpk ? 3 : 2;
        t.files = A.ch->nfiles;
        t.data_blocks = A.head->nblocks;
        t.arena_bytes = A.ch->arena_al - A.ch->last_pad;
        t.handle_pairs = t.data_blocks + extra * t.files;
        if (A.head->large || A.ch->large) t.status |= LV_COMPACT_OUT_BLOCK_LARGE;
        if (t.data_blocks > A.block_cap) t.status |= LV_COMPACT_OUT_HANDLE_OVER;
        if (t.arena_bytes > A.file_cap) t.status |= LV_COMPACT_OUT_ARENA_OVER;
        if (t.files > A.files_cap) t.status |= LV_COMPACT_OUT_FILES_OVER;
        if (O.vfiles) {
            const uint64_t used = *O.bound_used;
            t.bound_bytes = A.ch->bound_bytes;
            A.ch->bound_at = used;
            if (used > O.bound_cap || t.bound_bytes > O.bound_cap - used) t.status |= LV_COMPACT_OUT_BOUND_OVER;
        }
        if (!t.status) A.head->go = 1;
    }
    *O.totals = t;
}

// Several files in one arena: a block's place goes through its file.
struct CoManyFiles {
    const SbArgs &A;
    __device__ __forceinline__ SbBlockAt block(uint64_t i) const {
        const uint64_t b = A.Cl[i] + A.cC[i / kSbTile] - 1, k = co_file_of(A, b);
        const uint64_t off = co_Bbefore(A, b) - co_Bbefore(A, A.cf[k].fb);
        return SbBlockAt{A.bstart[b], co_layout(A, k).file_off + off, off, co_raw(A, b)};
    }
    __device__ __forceinline__ SbIndexAt index(uint64_t i, const SbBlockAt &) const {
        const uint64_t b = A.Cl[i] + A.cC[i / kSbTile] - 1, k = co_file_of(A, b);
        const CoFile &c = A.cf[k];
        const CoLayout L = co_layout(A, k);
        return SbIndexAt{A.file + L.file_off + L.index_off, c.idx_bytes, b - c.fb,
                         co_Ibefore(A, b + 1) - co_Ibefore(A, c.fb), b + 1 == c.fe};
    }
};

__global__ __launch_bounds__(kSbThreads) void co_emit(const SbArgs A) {
    if (!A.head->go) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n = sb_entries(A);
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x;
    if (static_cast<uint64_t>(blockIdx.x) * kSbThreads >= n) return;
    sb_emit_entry(A, i, i < n, lane, CoManyFiles{A});
}

// A lane per handle pair of the workspace copy: the data blocks by id, then a
// metaindex block per file.  The data blocks' pairs of d_handles too.
__global__ __launch_bounds__(kSbThreads) void co_handles(const SbArgs A) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x;
    if (j >= A.block_cap + A.files_cap) return;
    const bool go = A.head->go;
    uint64_t off = ~0ull, size = 0;  // the seal skips a handle out of range without touching the arena
    if (j < A.block_cap) {
        if (go && j < A.head->nblocks) {
            const uint64_t k = co_file_of(A, j), rel = co_Bbefore(A, j) - co_Bbefore(A, A.cf[k].fb);
            const uint64_t at = j + k * (A.bpk ? 3 : 2);
            size = co_raw(A, j);
            off = co_layout(A, k).file_off + rel;
            A.handles[2 * at] = rel;
            A.handles[2 * at + 1] = size;
        }
    } else if (go && j - A.block_cap < A.ch->nfiles) {
        const CoLayout L = co_layout(A, j - A.block_cap);
        off = L.file_off + L.meta_off;
        size = L.meta_size;
    }
    A.wsh[2 * j] = off;
    A.wsh[2 * j + 1] = size;
}

// An internal key at dst: the user key (its copy is the wave's), then the tag.
__device__ __forceinline__ void co_put_tag(uint8_t *dst, uint64_t tag) {
    for (uint32_t t = 0; t < 8; ++t) dst[t] = static_cast<uint8_t>(tag >> (8 * t));
}

// A lane per file, every lane of a wave to the end: the bound keys' copies are
// the wave's.
__global__ __launch_bounds__(kSbThreads) void co_file_tail(const SbArgs A, const CoOut O) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x;
    const bool go = A.head->go;
    const uint32_t per = A.bpk ? 2 : 1;
    const bool on = go && k < A.ch->nfiles;  // (nfiles <= files_cap: the plan checked)
    uint8_t *d0 = nullptr, *d1 = nullptr;
    const uint8_t *s0 = nullptr, *s1 = nullptr;
    uint64_t n0 = 0, n1 = 0;
    if (k < A.files_cap && !on)
        for (uint32_t t = 0; t < per; ++t) {
            A.idx_off[per * k + t] = 0;
            A.idx_len[per * k + t] = 0;
        }
    if (on) {
        const CoFile c = A.cf[k];
        const CoLayout L = co_layout(A, k);
        const uint64_t blocks = c.fe - c.fb, extra = A.bpk ? 3 : 2;
        uint8_t *file = A.file + L.file_off;
        file[L.index_off + L.index_size] = LV_SST_NO_COMPRESSION;
        uint8_t *m = file + L.meta_off;
        uint64_t *h = A.handles + 2 * (c.fb + blocks + k * extra);
        A.idx_off[per * k] = L.file_off + L.index_off;
        A.idx_len[per * k] = static_cast<uint32_t>(L.index_size + 1);  // (< 2^32 - 1: the plan checked)
        if (A.bpk) {
            // the filter block's end: array_offset, the base, the type byte
            uint8_t *e = file + L.filter_off + L.filter_size;
            sb_put_fixed32(e - 5, static_cast<uint32_t>(c.filt_bytes));
            e[-1] = LV_SST_FILTER_BASE_LG;
            e[0] = LV_SST_NO_COMPRESSION;
            // the metaindex block's one entry: shared 0, the name, the filter block's handle
            constexpr char name[] = LV_SST_BLOOM_NAME;
            m = put_varint(m, 0);
            m = put_varint(m, kSbBloomName);
            m = put_varint(m, L.meta_size - 3 - kSbBloomName - 8);
            for (uint32_t t = 0; t < kSbBloomName; ++t) *m++ = static_cast<uint8_t>(name[t]);
            m = put_varint(m, L.filter_off);
            m = put_varint(m, L.filter_size);
            *h++ = L.filter_off;
            *h++ = L.filter_size;
            A.idx_off[per * k + 1] = L.file_off + L.filter_off;
            A.idx_len[per * k + 1] = static_cast<uint32_t>(L.filter_size + 1);
        }
        sb_put_fixed32(m, 0);  // (an empty BlockBuilder: 00 00 00 00 01 00 00 00)
        sb_put_fixed32(m + 4, 1);
        *h++ = L.meta_off;
        *h++ = L.meta_size;
        *h++ = L.index_off;
        *h++ = L.index_size;
        sb_put_fixed32(file + L.index_off + c.idx_bytes + 4 * blocks, static_cast<uint32_t>(blocks));
        uint8_t *f = file + L.index_off + L.index_size + LV_SST_TRAILER_SIZE, *q = f;
        q = put_varint(q, L.meta_off);
        q = put_varint(q, L.meta_size);
        q = put_varint(q, L.index_off);
        q = put_varint(q, L.index_size);
        while (q < f + 40) *q++ = 0;
        for (uint32_t t = 0; t < 8; ++t) *q++ = static_cast<uint8_t>(LV_SST_MAGIC >> (8 * t));
        // the records: what the opens and lv_version_file_device find in the image
        lv_compact_output_file r{};
        r.first_entry = c.first;
        r.entries = c.entries;
        r.file_off = L.file_off;
        r.file_bytes = L.file_bytes;
        r.data_blocks = blocks;
        r.first_handle = c.fb + k * extra;
        r.filter_keys = A.bpk ? c.entries : 0;
        O.files[k] = r;
        lv_sst_table tb{};
        tb.file_bytes = L.file_bytes;
        tb.metaindex_offset = L.meta_off;
        tb.metaindex_size = L.meta_size;
        tb.index_offset = L.index_off;
        tb.index_size = L.index_size;
        tb.data_blocks = blocks;
        O.tables[k] = tb;
        if (O.blooms) {
            lv_sst_bloom bl{};
            if (A.bpk) {
                bl.filter_offset = L.filter_off;
                bl.filter_size = L.filter_size;
                bl.array_offset = c.filt_bytes;
                bl.num = c.filters;
                bl.base_lg = LV_SST_FILTER_BASE_LG;
                bl.present = 1;
            } else {
                bl.why = LV_SST_BLOOM_NO_ENTRY;  // an empty metaindex block
            }
            O.blooms[k] = bl;
        }
        if (O.vfiles) {
            const lv_wb_op a = load_op(A.ops + A.order[c.first]);
            const lv_wb_op z = load_op(A.ops + A.order[c.first + c.entries - 1]);
            const uint64_t at = A.ch->bound_at + c.Kl + A.cU[k / kSbTile] - c.small_len - c.large_len;
            lv_version_file v{};
            v.number = O.first_number + k;
            v.file_off = O.images_off + L.file_off;
            v.file_cap = L.file_bytes;
            v.smallest_off = at;
            v.largest_off = at + c.small_len;
            v.smallest_len = static_cast<uint32_t>(c.small_len);  // (< 2^32: a key that long makes its block LARGE,
            v.largest_len = static_cast<uint32_t>(c.large_len);   //  and the plan has let nothing through)
            v.level = O.level;
            O.vfiles[k] = v;
            d0 = O.bound_keys + at;
            s0 = A.payload + a.key_off;
            n0 = a.key_len;
            co_put_tag(d0 + n0, a.tag);
            d1 = d0 + c.small_len;
            s1 = A.payload + z.key_off;
            n1 = z.key_len;
            co_put_tag(d1 + n1, z.tag);
            if (k == 0) *O.bound_used = A.ch->bound_at + A.ch->bound_bytes;
        }
    }
    if (O.vfiles) {
        group_copy<kSbCopyLanes, kSbWaveCopy>(d0, s0, n0, lane);
        group_copy<kSbCopyLanes, kSbWaveCopy>(d1, s1, n1, lane);
    }
}

// A lane per file: the index block's (and the filter block's) trailer from
// the batch's masked crcs.
__global__ __launch_bounds__(kSbThreads) void co_trailer(const SbArgs A) {
    const uint64_t k = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x;
    if (!A.head->go || k >= A.ch->nfiles) return;
    const uint32_t per = A.bpk ? 2 : 1;
    const CoLayout L = co_layout(A, k);
    uint8_t *file = A.file + L.file_off;
    sb_put_fixed32(file + L.index_off + L.index_size + 1, A.idx_crc[per * k]);
    if (A.bpk) sb_put_fixed32(file + L.filter_off + L.filter_size + 1, A.idx_crc[per * k + 1]);
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxOpCap = 0xfffffffeull;
constexpr uint64_t kMaxBlockCap = 0xfffffffcull;

constexpr uint64_t co_tiles(uint64_t cap) { return (cap + lvk::kSbTile - 1) / lvk::kSbTile; }

// The workspace for op_cap = cap, block_cap = bc and files_cap = fc, region by
// region (the same with and without a filter policy); returns the CRC batch's
// sub-workspace (lv_crc32c_workspace_bytes(2 fc) bytes).
uint8_t *co_carve(Carve &C, uint64_t cap, uint64_t bc, uint64_t fc, lvk::SbArgs &A) {
    const uint64_t tiles = co_tiles(cap);
    A.head = C.take<lvk::SbHead>(1);
    A.bh = C.take<lvk::SbBloomHead>(1);
    A.ch = C.take<lvk::CoHead>(1);
    A.shared = C.take<uint64_t>(cap);
    A.Pl = C.take<uint64_t>(cap);
    A.Sl = C.take<uint64_t>(cap);
    A.cP = C.take<uint64_t>(tiles);
    A.cS = C.take<uint64_t>(tiles * lvk::kSbMaxR);
    A.nxt = C.take<uint32_t>(cap);
    A.J[0] = C.take<uint32_t>(cap);
    A.J[1] = C.take<uint32_t>(cap);
    A.F = C.take<uint8_t>(cap);
    A.Cl = C.take<uint64_t>(cap);
    A.Bl = C.take<uint64_t>(cap);
    A.Il = C.take<uint64_t>(cap);
    A.cC = C.take<uint64_t>(tiles);
    A.cB = C.take<uint64_t>(tiles);
    A.cI = C.take<uint64_t>(tiles);
    A.bstart = C.take<uint32_t>(cap);
    A.Fn = C.take<uint32_t>(cap);
    A.Fl = C.take<uint64_t>(cap);
    A.cF = C.take<uint64_t>(tiles);
    A.Binc = C.take<uint64_t>(cap);
    A.fnx = C.take<uint32_t>(cap);
    A.FF = C.take<uint8_t>(cap);
    A.Kl = C.take<uint64_t>(cap);
    A.cK = C.take<uint64_t>(tiles);
    A.fstart = C.take<uint32_t>(cap);
    A.cA = C.take<uint64_t>(tiles);
    A.cU = C.take<uint64_t>(tiles);
    A.cW = C.take<uint64_t>(tiles);
    A.cf = C.take<lvk::CoFile>(fc);
    A.wsh = C.take<uint64_t>(2 * (bc + fc));
    A.idx_off = C.take<uint64_t>(2 * fc);
    A.idx_len = C.take<uint32_t>(2 * fc);
    A.idx_crc = C.take<uint32_t>(2 * fc);
    return C.take<uint8_t>(lv_crc32c_workspace_bytes(2 * fc));
}

}  // namespace

extern "C" {

size_t lv_compact_output_workspace_bytes(size_t op_cap, size_t block_cap, size_t files_cap) {
    if (op_cap > kMaxOpCap || block_cap > kMaxBlockCap || files_cap > LV_VERSION_MAX_FILES) return 0;
    lvk::SbArgs A{};
    Carve C{nullptr};
    co_carve(C, op_cap, block_cap, files_cap, A);
    return C.at;
}

int lv_compact_output_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops,
                             const uint32_t *d_order, const lv_mt_totals *d_mt_totals, size_t op_cap,
                             const lv_sst_build_options *opt, const lv_sst_bloom_options *bloom, uint64_t max_file_bytes,
                             uint64_t first_number, uint32_t level, uint64_t images_off, uint8_t *d_arena,
                             uint64_t arena_cap, uint64_t *d_handles, size_t block_cap, lv_compact_output_file *d_files,
                             lv_sst_table *d_tables, lv_sst_bloom *d_blooms, lv_version_file *d_version_files,
                             size_t files_cap, uint8_t *d_bound_keys, uint64_t bound_keys_cap, uint64_t *d_bound_used,
                             lv_compact_output_totals *d_totals, uint32_t flags, void *d_workspace,
                             size_t workspace_bytes, void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    const uint32_t bs = opt ? opt->block_size : LV_SST_DEFAULT_BLOCK_SIZE;
    const uint32_t ri = opt ? opt->restart_interval : LV_SST_DEFAULT_RESTART_INTERVAL;
    if (bs < 1 || bs > LV_SST_MAX_BLOCK_SIZE) return set_err(LV_ERR_INVALID, "block_size must be in [1, 2^30]");
    if (ri < 1 || ri > LV_SST_MAX_RESTART_INTERVAL)
        return set_err(LV_ERR_INVALID, "restart_interval must be in [1, 1024]");
    if (bloom && (bloom->bits_per_key < 1 || bloom->bits_per_key > 64))
        return set_err(LV_ERR_INVALID, "bits_per_key must be in [1, 64]");
    if (bloom && bloom->reserved) return set_err(LV_ERR_INVALID, "bloom options: reserved must be 0");
    if (!max_file_bytes) return set_err(LV_ERR_INVALID, "max_file_bytes must be at least 1");
    if (level < 1 || level >= LV_NUM_LEVELS) return set_err(LV_ERR_INVALID, "level must be in [1, 6]");
    if (files_cap > LV_VERSION_MAX_FILES) return set_err(LV_ERR_INVALID, "files_cap above LV_VERSION_MAX_FILES");
    if (first_number + files_cap < first_number) return set_err(LV_ERR_INVALID, "first_number + files_cap wraps");
    if (!d_totals) return set_err(LV_ERR_INVALID, "null d_totals");
    if (misaligned(d_totals, 8)) return set_err(LV_ERR_INVALID, "d_totals must be 8-byte aligned");
    if (!d_mt_totals) return set_err(LV_ERR_INVALID, "null d_mt_totals");
    if (misaligned(d_mt_totals, 8)) return set_err(LV_ERR_INVALID, "d_mt_totals must be 8-byte aligned");
    if (!d_payload && payload_bytes) return set_err(LV_ERR_INVALID, "null d_payload");
    if (op_cap > kMaxOpCap) return set_err(LV_ERR_INVALID, "op_cap too large for one build (at most 2^32 - 2)");
    if (block_cap > kMaxBlockCap) return set_err(LV_ERR_INVALID, "block_cap too large for one build (at most 2^32 - 4)");
    if (op_cap && !d_ops) return set_err(LV_ERR_INVALID, "null d_ops");
    if (misaligned(d_ops, 16)) return set_err(LV_ERR_INVALID, "d_ops must be 16-byte aligned");
    if (op_cap && !d_order) return set_err(LV_ERR_INVALID, "null d_order");
    if (misaligned(d_order, 4)) return set_err(LV_ERR_INVALID, "d_order must be 4-byte aligned");
    if (arena_cap && !d_arena) return set_err(LV_ERR_INVALID, "null d_arena");
    if (misaligned(d_arena, 16)) return set_err(LV_ERR_INVALID, "d_arena must be 16-byte aligned");
    if (!d_handles) return set_err(LV_ERR_INVALID, "null d_handles");
    if (misaligned(d_handles, 8)) return set_err(LV_ERR_INVALID, "d_handles must be 8-byte aligned");
    if (files_cap && !d_files) return set_err(LV_ERR_INVALID, "null d_files");
    if (files_cap && !d_tables) return set_err(LV_ERR_INVALID, "null d_tables");
    if (misaligned(d_files, 8) || misaligned(d_tables, 8) || misaligned(d_blooms, 8) || misaligned(d_version_files, 8))
        return set_err(LV_ERR_INVALID, "d_files, d_tables, d_blooms and d_version_files must be 8-byte aligned");
    if (d_version_files && !d_bound_used) return set_err(LV_ERR_INVALID, "null d_bound_used");
    if (d_version_files && bound_keys_cap && !d_bound_keys) return set_err(LV_ERR_INVALID, "null d_bound_keys");
    if (misaligned(d_bound_used, 8)) return set_err(LV_ERR_INVALID, "d_bound_used must be 8-byte aligned");
    if (!d_workspace) return set_err(LV_ERR_INVALID, "null workspace");
    if (misaligned(d_workspace, 16)) return set_err(LV_ERR_INVALID, "workspace must be 16-byte aligned");
    lvk::SbArgs A{};
    Carve C{static_cast<uint8_t *>(d_workspace)};
    uint8_t *crc_ws = co_carve(C, op_cap, block_cap, files_cap, A);
    if (workspace_bytes < C.at) return set_err(LV_ERR_INVALID, "workspace too small");
    const bool bounds = d_version_files != nullptr;
    const struct Range {
        const void *p;
        uint64_t bytes;
        const char *name;
    } ins[3] = {{d_payload, payload_bytes, "d_payload"},
                {d_ops, static_cast<uint64_t>(op_cap) * sizeof(lv_wb_op), "d_ops"},
                {d_order, static_cast<uint64_t>(op_cap) * sizeof(uint32_t), "d_order"}},
      outs[9] = {{d_arena, arena_cap, "d_arena"},
                 {d_handles, (static_cast<uint64_t>(block_cap) + 3 * static_cast<uint64_t>(files_cap)) * 16, "d_handles"},
                 {d_files, static_cast<uint64_t>(files_cap) * sizeof(lv_compact_output_file), "d_files"},
                 {d_tables, static_cast<uint64_t>(files_cap) * sizeof(lv_sst_table), "d_tables"},
                 {d_blooms, static_cast<uint64_t>(files_cap) * sizeof(lv_sst_bloom), "d_blooms"},
                 {d_version_files, static_cast<uint64_t>(files_cap) * sizeof(lv_version_file), "d_version_files"},
                 {bounds ? d_bound_keys : nullptr, bounds ? bound_keys_cap : 0, "d_bound_keys"},
                 {bounds ? d_bound_used : nullptr, bounds ? 8u : 0u, "d_bound_used"},
                 {d_totals, sizeof(lv_compact_output_totals), "d_totals"}};
    for (size_t i = 0; i < 9; ++i) {
        if (!outs[i].p) continue;
        for (const auto &in : ins)
            if (overlaps(outs[i].p, outs[i].bytes, in.p, in.bytes))
                return set_err(LV_ERR_INVALID, std::string(outs[i].name) + " overlaps " + in.name);
        if (overlaps(outs[i].p, outs[i].bytes, d_mt_totals, sizeof(lv_mt_totals)))
            return set_err(LV_ERR_INVALID, std::string(outs[i].name) + " overlaps d_mt_totals");
        for (size_t j = 0; j < i; ++j)
            if (outs[j].p && overlaps(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return set_err(LV_ERR_INVALID, std::string(outs[j].name) + " overlaps " + outs[i].name);
    }
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    A.payload = d_payload;
    A.payload_bytes = payload_bytes;
    A.ops = d_ops;
    A.order = d_order;
    A.mt = d_mt_totals;
    A.op_cap = op_cap;
    A.bs = bs;
    A.R = ri;
    A.file = d_arena;
    A.file_cap = arena_cap;
    A.handles = d_handles;
    A.block_cap = block_cap;
    A.bpk = bloom ? bloom->bits_per_key : 0;
    A.mf = max_file_bytes;
    A.files_cap = files_cap;
    const lvk::CoOut O{d_files,       d_tables, d_blooms,     d_version_files, d_bound_keys, bound_keys_cap,
                       d_bound_used, d_totals, first_number, images_off,      level};

    const dim3 b(lvk::kSbThreads);
    const uint32_t tiles = static_cast<uint32_t>(co_tiles(op_cap));
    const uint32_t eg = static_cast<uint32_t>((static_cast<uint64_t>(op_cap) + lvk::kSbThreads - 1) / lvk::kSbThreads);
    constexpr uint32_t kWaves = lvk::kSbThreads / 64;
    hipLaunchKernelGGL(lvk::sb_init, dim3(1), dim3(1), 0, s, A);
    if (tiles) {
        // the block starts: the one-file build's chain
        hipLaunchKernelGGL(lvk::sb_sizes, dim3(tiles), b, 0, s, A);
        hipLaunchKernelGGL(lvk::sb_carry, dim3((ri + 1 + kWaves - 1) / kWaves), b, 0, s, A, 0u);
        hipLaunchKernelGGL(lvk::sb_next, dim3(eg), b, 0, s, A);
        for (uint32_t p = 0; (1ull << p) < op_cap; ++p) hipLaunchKernelGGL(lvk::sb_reach, dim3(eg), b, 0, s, A, p);
        hipLaunchKernelGGL(lvk::sb_layout, dim3(tiles), b, 0, s, A);
        hipLaunchKernelGGL(lvk::sb_carry, dim3(1), b, 0, s, A, 1u);
        // the file starts: the same chain over blocks
        hipLaunchKernelGGL(lvk::co_blocks, dim3(eg), b, 0, s, A);
        hipLaunchKernelGGL(lvk::co_fnext, dim3(eg), b, 0, s, A);
        for (uint32_t p = 0; (1ull << p) < op_cap; ++p) hipLaunchKernelGGL(lvk::co_freach, dim3(eg), b, 0, s, A, p);
        hipLaunchKernelGGL(lvk::co_fscan, dim3(tiles), b, 0, s, A);
        hipLaunchKernelGGL(lvk::sb_carry, dim3(1), b, 0, s, A, 4u);
        hipLaunchKernelGGL(lvk::co_fmark, dim3(eg), b, 0, s, A);
        hipLaunchKernelGGL(lvk::co_index, dim3(tiles), b, 0, s, A);
        hipLaunchKernelGGL(lvk::sb_carry, dim3(1), b, 0, s, A, 5u);
        hipLaunchKernelGGL(lvk::co_files, dim3(tiles), b, 0, s, A);
        hipLaunchKernelGGL(lvk::sb_carry, dim3(1), b, 0, s, A, 6u);
    }
    hipLaunchKernelGGL(lvk::co_plan, dim3(1), dim3(1), 0, s, A, O);
    const bool write = tiles && files_cap && arena_cap;
    if (write) {
        hipLaunchKernelGGL(lvk::co_emit, dim3(eg), b, 0, s, A);
        if (bloom) {
            // a wave per data block, a lane per window: grid-stride loops over capped grids
            const uint32_t wg = static_cast<uint32_t>(lvgpu_internal::sb_bloom_grid(op_cap));
            const uint32_t og = static_cast<uint32_t>(
                lvgpu_internal::sb_bloom_offsets_grid((arena_cap >> LV_SST_FILTER_BASE_LG) + files_cap));
            hipLaunchKernelGGL(lvk::sb_bloom_emit, dim3(wg), b, 0, s, A);
            hipLaunchKernelGGL(lvk::sb_bloom_big, dim3(wg), b, 0, s, A);
            hipLaunchKernelGGL(lvk::sb_bloom_offsets, dim3(og), b, 0, s, A);
        }
        const uint64_t pairs = static_cast<uint64_t>(block_cap) + files_cap;
        hipLaunchKernelGGL(lvk::co_handles, dim3(static_cast<uint32_t>((pairs + lvk::kSbThreads - 1) / lvk::kSbThreads)), b,
                           0, s, A);
        const uint32_t fg = static_cast<uint32_t>((static_cast<uint64_t>(files_cap) + lvk::kSbThreads - 1) / lvk::kSbThreads);
        hipLaunchKernelGGL(lvk::co_file_tail, dim3(fg), b, 0, s, A, O);
        if (int rc = check_launch()) return rc;
        // the trailers: the seal's own kernel over the padded absolute handles (data blocks and
        // metaindex blocks) ...
        if (int rc = lvgpu_internal::launch_sst_blocks(true, d_arena, arena_cap, A.wsh, nullptr,
                                                       static_cast<size_t>(pairs), nullptr, nullptr, stream))
            return rc;
        // ... and every file's index block (with a filter policy, its filter block too) as one batch
        // of the offsets API (empty buffers where nothing was written)
        const size_t nbuf = (bloom ? 2 : 1) * files_cap;
        if (int rc = lv_crc32c_batch_device_ws(d_arena, A.idx_off, A.idx_len, nullptr, A.idx_crc, nbuf, LV_CRC_MASK,
                                               crc_ws, lv_crc32c_workspace_bytes(2 * files_cap), stream))
            return rc;
        hipLaunchKernelGGL(lvk::co_trailer, dim3(fg), b, 0, s, A);
    }
    if (int rc = check_launch()) return rc;
    // (the batch's own kernels depend on 2 files_cap: one launch up to 1,024 buffers, the length sort above)
    static thread_local std::string name;
    name = "sb_init+sb_sizes+sb_carry+sb_next+sb_reach+sb_layout+co_blocks+co_fnext+co_freach+co_fscan+co_fmark+"
           "co_index+co_files+co_plan";
    if (write) {
        name += bloom ? "+co_emit+sb_bloom_emit+sb_bloom_big+sb_bloom_offsets" : "+co_emit";
        name += std::string("+co_handles+co_file_tail+sst_blocks_kernel<seal>+") + (g_kernel ? g_kernel : "") + "+co_trailer";
    }
    g_kernel = name.c_str();
    return LV_OK;
}

}  // extern "C"
