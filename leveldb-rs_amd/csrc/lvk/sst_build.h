// What the SSTable build (sst_build.hip) shares with the compaction output
// (compact_output.hip): the call's arguments and workspace heads, the size
// algebra of a block (P, S, the estimate), the separator, the index entry, the
// filter's size, the body of the entry emit, and the declarations of the build's
// kernels, which the compaction output launches as they are up to the layout's
// carry.  sst_build.hip's head comment explains the chain.
//
// Several files in one arena (SbArgs::mf != 0, lv_compact_output_device): the
// block starts are the single-file build's; a second chain over blocks cuts
// them into files, and everything behind a block's id goes through its file
// (co_file_of, CoFile).  The four capped kernels sb_carry, sb_bloom_emit,
// sb_bloom_big and sb_bloom_offsets serve both calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../../include/lvgpu/compact.h"
#include "../../../include/lvgpu/table.h"
#include "knobs.h"
#include "sst_read.h"
#include "stage.h"

namespace lvk {

constexpr uint32_t kSbTile = LVK_SB_TILE;            // entries per scan tile
constexpr uint32_t kSbWaveCopy = LVK_SB_WAVE_COPY;   // bytes from which a copy is the wave's
constexpr uint32_t kSbCopyLanes = LVK_SB_COPY_LANES; // lanes of a wave that share one such copy
constexpr uint32_t kSbThreads = 256;
constexpr uint32_t kSbPer = kSbTile / kSbThreads;
constexpr uint32_t kSbMaxR = LV_SST_MAX_RESTART_INTERVAL;
constexpr uint64_t kSbLarge = 0xffffffffull;  // raw sizes from here on: sst_in_range refuses them
constexpr uint32_t kSbBloomName = sizeof(LV_SST_BLOOM_NAME) - 1;
static_assert(kSbBloomName == 34, "the metaindex key");
static_assert(kSbTile % kSbThreads == 0 && kSbTile >= kSbMaxR, "a tile holds every residue of a restart interval");
static_assert(kSbTile * 16 <= 65536, "two u64 scan arrays fit the LDS a workgroup may declare");
static_assert(kSbWaveCopy >= 16, "a wave copy has at least one granule");
static_assert(kSbCopyLanes >= 16 && 64 % kSbCopyLanes == 0, "a copy's lanes cover a ragged head or tail of 15 bytes");

struct SbHead {  // workspace, zeroed by sb_init
    uint32_t bad, large, go, pad;
    unsigned long long nblocks, data_bytes, idx_bytes, meta_off, index_off, index_size;
};

struct SbBloomHead {  // workspace, zeroed by sb_init
    unsigned long long filt_bytes, filter_off, filter_size, filters, meta_size;
    unsigned long long big;  // some filter is beyond the LDS budget of sb_bloom_emit: sb_bloom_big has work
    unsigned long long pad[2];
};

struct CoHead {  // workspace, zeroed by sb_init (several files)
    unsigned long long nfiles;
    unsigned long long arena_al;     // the sum of the files' bytes, each rounded up to 16
    unsigned long long bound_bytes;  // the sum of the files' two bound keys
    unsigned long long windows;      // the sum of the files' filter windows
    unsigned long long bound_at;     // the cursor the plan read
    uint32_t large, pad;
    unsigned long long last_pad;     // what rounding up added to the last file
};

struct CoFile {  // workspace, one per output file below files_cap
    uint32_t fb, fe;              // its blocks [fb, fe)
    uint32_t first, entries;      // its entries [first, first + entries)
    uint64_t data_bytes, idx_bytes, filt_bytes, filters;
    uint64_t Al, Kl, Wl;          // tile-local inclusive scans: bytes rounded up to 16, bound bytes, windows
    uint64_t small_len, large_len;  // the bound keys' lengths (internal keys: key_len + 8 may pass 2^32)
};

struct SbArgs {
    const uint8_t *payload;
    uint64_t payload_bytes;
    const lv_wb_op *ops;
    const uint32_t *order;
    const lv_mt_totals *mt;
    uint64_t op_cap;
    uint32_t bs, R;
    uint8_t *file;
    uint64_t file_cap;
    uint64_t *handles;
    uint64_t block_cap;
    lv_sst_build_totals *totals;
    // workspace
    SbHead *head;
    uint64_t *shared;        // [cap] common prefix with the entry before, over internal-key bytes
    uint64_t *Pl, *Sl;       // [cap] tile-local inclusive scans
    uint64_t *cP, *cS;       // [tiles], [tiles * R]: the tiles' sums, then their exclusive scans
    uint32_t *nxt, *J[2];    // [cap] next(s); the doubling's jump arrays
    uint8_t *F;              // [cap] block-start flags
    uint64_t *Cl, *Bl, *Il;  // [cap] tile-local scans: block count, file bytes, index bytes
    uint64_t *cC, *cB, *cI;  // [tiles]
    uint32_t *blk_start;     // [block_cap]
    uint64_t *wsh;           // [2 (block_cap + 2)] the handles the seal reads
    uint64_t *idx_off;       // [1] the index block as a one-buffer batch of the offsets API:
    uint32_t *idx_len;       // [1] contents || type
    uint32_t *idx_crc;       // [1] its masked crc
    // lv_sst_build_bloom_device (bpk != 0; table.h, "Bloom filter blocks").  The
    // arrays are by block id and hold op_cap entries: a table has no more
    // blocks than entries, whatever block_cap is.  With a filter the batch
    // above has two buffers, the index block and the filter block, and wsh
    // 2 (block_cap + 3) words.
    uint32_t bpk;
    lv_sst_bloom_totals *btotals;
    SbBloomHead *bh;
    uint64_t *boff;          // [cap] the block's file offset
    uint32_t *bstart;        // [cap] its first entry
    uint32_t *Fn;            // [cap] the keys of the window it is the first block of, or 0
    uint64_t *Fl;            // [cap] tile-local exclusive scan of the filters' bytes
    uint64_t *cF;            // [tiles]
    // lv_compact_output_device (mf != 0; compact.h).  By block id, op_cap
    // entries each, as above; Il, cI, Fl, cF and bstart are by block id too, J
    // serves the file chain's doubling, wsh holds block_cap + files_cap pairs
    // (the data blocks by id, then a metaindex block per file) and the batch
    // 2 files_cap buffers (index block, filter block per file).
    uint64_t mf;             // max_file_bytes
    uint64_t files_cap;
    CoHead *ch;
    uint64_t *Binc;          // [cap] the inclusive scan of raw + 5
    uint32_t *fnx;           // [cap] fnext(b)
    uint8_t *FF;             // [cap] file-start flags
    uint64_t *Kl, *cK;       // [cap], [tiles] the scan of the file count over blocks
    uint32_t *fstart;        // [cap] by file: its first block
    uint64_t *cA, *cU, *cW;  // [tiles] by file tile: bytes rounded up to 16, bound bytes, windows
    CoFile *cf;              // [files_cap]
};

// The entries, or 0 when there is no table to read.
__device__ __forceinline__ uint64_t sb_entries(const SbArgs &A) {
    const uint64_t n = A.mt->entries;
    return (A.mt->status || n > A.op_cap) ? 0 : n;
}

__device__ __forceinline__ void sb_put_fixed32(uint8_t *p, uint32_t v) {
    p[0] = static_cast<uint8_t>(v);
    p[1] = static_cast<uint8_t>(v >> 8);
    p[2] = static_cast<uint8_t>(v >> 16);
    p[3] = static_cast<uint8_t>(v >> 24);
}

// The global scans from the tile-local ones and the scanned carries.
__device__ __forceinline__ uint64_t sb_P(const SbArgs &A, uint64_t i) { return A.Pl[i] + A.cP[i / kSbTile]; }
__device__ __forceinline__ uint64_t sb_S(const SbArgs &A, uint64_t i) {
    return A.Sl[i] + A.cS[(i / kSbTile) * A.R + i % A.R];
}
// len(buffer) of the block that starts at s after entry e >= s, and its restarts.
__device__ __forceinline__ uint64_t sb_buffer(const SbArgs &A, uint64_t s, uint64_t e, uint64_t *restarts) {
    const uint64_t k = (e - s) / A.R, last = s + k * A.R;
    *restarts = k + 1;
    return sb_P(A, e) - (s ? sb_P(A, s - 1) : 0) + sb_S(A, last) - (s >= A.R ? sb_S(A, s - A.R) : 0);
}
__device__ __forceinline__ uint64_t sb_estimate(const SbArgs &A, uint64_t s, uint64_t e) {
    uint64_t r;
    const uint64_t b = sb_buffer(A, s, e, &r);
    return b + 4 * r + 4;
}

// One doubling pass p over a chain of n nodes: F holds the first 2^p nodes
// reachable from node 0 (and maybe more of them: a flag set during this pass
// is a true one too), src is next^(2^p).  A pass with 2^p >= n has nothing
// left to mark.
__device__ __forceinline__ void sb_reach_pass(uint64_t n, uint64_t i, uint32_t pass, const uint32_t *nxt,
                                              uint32_t *const J[2], uint8_t *F) {
    if (i >= n || (1ull << pass) >= n) return;
    const uint32_t *src = pass == 0 ? nxt : J[(pass - 1) & 1u];
    uint32_t *dst = J[pass & 1u];
    const uint32_t j = src[i];
    if (j < n && F[i]) F[j] = 1;
    dst[i] = j < n ? src[j] : static_cast<uint32_t>(n);
}

// The index key of the block whose last entry is e (op o): `copy` bytes of
// its user key, then (bump) the byte after them plus one and MAXTAG, or its
// own tag.  shortest_separator against entry e + 1, short_successor for the
// last block of a file.
struct SbSep {
    uint64_t copy;
    bool bump;
};
__device__ __forceinline__ SbSep sb_separator(const SbArgs &A, uint64_t e, bool last, const lv_wb_op &o) {
    const uint8_t *ka = A.payload + o.key_off;
    const uint64_t la = o.key_len;
    if (!last) {
        const lv_wb_op b = load_op(A.ops + A.order[e + 1]);
        const uint64_t lb = b.key_len, m = la < lb ? la : lb;
        uint64_t d = A.shared[e + 1];  // over internal keys: the user keys' is no longer than either
        if (d > m) d = m;
        if (d >= m) return SbSep{la, false};
        const uint32_t c = ka[d];
        if (c < 0xffu && c + 1 < A.payload[b.key_off + d]) return SbSep{d, true};
        return SbSep{la, false};
    }
    uint64_t i = 0;
    while (i < la && ka[i] == 0xffu) ++i;
    if (i >= la || i + 1 >= la) return SbSep{la, false};
    return SbSep{i, true};
}

struct SbIndexEntry {
    uint64_t klen, hlen, size;
    SbSep sep;
};
__device__ __forceinline__ SbIndexEntry sb_index_entry(const SbArgs &A, uint64_t e, bool last, const lv_wb_op &o,
                                                       uint64_t off, uint64_t raw) {
    SbIndexEntry x;
    x.sep = sb_separator(A, e, last, o);
    x.klen = x.sep.copy + (x.sep.bump ? 1 : 0) + 8;
    x.hlen = varint_len(off) + varint_len(raw);
    x.size = 1 + varint_len(x.klen) + varint_len(x.hlen) + x.klen + x.hlen;
    return x;
}

// Bytes of the Bloom filter over `keys` keys, without its k byte.
__device__ __forceinline__ uint64_t sb_bloom_bytes(uint64_t keys, uint32_t bpk) {
    const uint64_t want = keys * bpk;  // keys < 2^32, bpk <= 64
    return ((want < 64 ? 64 : want) + 7) / 8;
}
__device__ __forceinline__ uint32_t sb_bloom_k(uint32_t bpk) {
    const uint32_t k = bpk * 69 / 100;
    return k < 1 ? 1 : k > 30 ? 30 : k;
}

// ---- several files: a block's file, a file's layout ----

// The file of block b and the scans by block id.
__device__ __forceinline__ uint64_t co_file_of(const SbArgs &A, uint64_t b) { return A.Kl[b] + A.cK[b / kSbTile] - 1; }
__device__ __forceinline__ uint64_t co_Bbefore(const SbArgs &A, uint64_t b) { return b ? A.Binc[b - 1] : 0; }
__device__ __forceinline__ uint64_t co_Ibefore(const SbArgs &A, uint64_t b) {
    return b ? A.Il[b - 1] + A.cI[(b - 1) / kSbTile] : 0;
}
// The exclusive scan of the filters' bytes at block b <= nb.
__device__ __forceinline__ uint64_t co_Fbefore(const SbArgs &A, uint64_t b, uint64_t nb) {
    return b < nb ? A.Fl[b] + A.cF[b / kSbTile] : A.bh->filt_bytes;
}

// A file's blocks behind its data blocks, as table.h lays them out.
struct CoLayout {
    uint64_t file_off;  // in the arena
    uint64_t filter_off, filter_size, meta_off, meta_size, index_off, index_size, file_bytes;
};
__device__ __forceinline__ CoLayout co_sizes(uint32_t bpk, uint64_t data_bytes, uint64_t blocks, uint64_t idx_bytes,
                                             uint64_t filt_bytes, uint64_t filters) {
    CoLayout L{};
    L.meta_off = data_bytes;
    L.meta_size = 8;
    if (bpk) {
        L.filter_off = data_bytes;
        L.filter_size = filt_bytes + 4 * filters + 5;
        L.meta_off = L.filter_off + L.filter_size + LV_SST_TRAILER_SIZE;
        L.meta_size = 3 + kSbBloomName + varint_len(L.filter_off) + varint_len(L.filter_size) + 8;
    }
    L.index_off = L.meta_off + L.meta_size + LV_SST_TRAILER_SIZE;
    L.index_size = idx_bytes + 4 * blocks + 4;
    L.file_bytes = L.index_off + L.index_size + LV_SST_TRAILER_SIZE + LV_SST_FOOTER_SIZE;
    return L;
}
// File k < files_cap once the files' carry has run.
__device__ __forceinline__ CoLayout co_layout(const SbArgs &A, uint64_t k) {
    const CoFile &f = A.cf[k];
    CoLayout L = co_sizes(A.bpk, f.data_bytes, f.fe - f.fb, f.idx_bytes, f.filt_bytes, f.filters);
    L.file_off = f.Al + A.cA[k / kSbTile] - ((L.file_bytes + 15) & ~15ull);
    return L;
}

// Where the filter of data block b (the first of its window) goes.
__device__ __forceinline__ uint8_t *sb_filter_at(const SbArgs &A, uint64_t b) {
    if (!A.mf) return A.file + A.bh->filter_off + A.Fl[b] + A.cF[b / kSbTile];
    const uint64_t k = co_file_of(A, b);
    const CoLayout L = co_layout(A, k);
    return A.file + L.file_off + L.filter_off + (co_Fbefore(A, b, ~0ull) - co_Fbefore(A, A.cf[k].fb, ~0ull));
}

// Window f of the call's windows, numbered file after file: the LE32 slot of
// its filter's start offset, and that offset.  The first block of the file at
// or beyond the window's first byte is the first of its own window, whose
// filter starts where this window's does; with no such block every filter of
// the file lies before.
__device__ __forceinline__ void co_window(const SbArgs &A, uint64_t f, uint8_t **slot, uint32_t *value) {
    const uint64_t nf = A.ch->nfiles, nb = A.head->nblocks;
    uint64_t lo = 0, hi = nf - 1;  // the last file whose first window is at or before f
    for (uint32_t it = 0; it < 40 && lo < hi; ++it) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (A.cf[mid].Wl + A.cW[mid / kSbTile] - A.cf[mid].filters <= f)
            lo = mid;
        else
            hi = mid - 1;
    }
    const uint64_t k = lo;
    const CoFile &c = A.cf[k];
    const CoLayout L = co_layout(A, k);
    const uint64_t local = f - (c.Wl + A.cW[k / kSbTile] - c.filters);
    const uint64_t lim = local << LV_SST_FILTER_BASE_LG, base = co_Bbefore(A, c.fb);
    uint64_t l = c.fb, h = c.fe;
    for (uint32_t it = 0; it < 40 && l < h; ++it) {
        const uint64_t mid = l + (h - l) / 2;
        if (co_Bbefore(A, mid) - base >= lim)
            h = mid;
        else
            l = mid + 1;
    }
    *slot = A.file + L.file_off + L.filter_off + c.filt_bytes + 4 * local;
    *value = static_cast<uint32_t>(l < c.fe ? co_Fbefore(A, l, nb) - co_Fbefore(A, c.fb, nb) : c.filt_bytes);
}

// ---- the entry emit ----

// Where entry i goes: its block's first entry, the block's place in A.file,
// the offset its handle names (relative to its file) and its raw size.
struct SbBlockAt {
    uint64_t s, at, off, raw;
};
// Where the index entry of that block goes: the file's index block, the bytes
// of its entries, the block's number in the file, the end of its entry among
// them, and whether it is the file's last block.
struct SbIndexAt {
    uint8_t *ix;
    uint64_t idx_bytes, b, end;
    bool last;
};

// Entry i (on: i < n) of sb_emit and co_emit: its varints, key suffix, tag
// bytes and value, its restart slot if it is one; a block's first entry also
// writes the restart count and the block's index entry.  Every lane of a wave
// calls it: the long copies are the wave's.  where.block(i) is an SbBlockAt,
// where.index(i, block) an SbIndexAt.
template <class Where>
__device__ __forceinline__ void sb_emit_entry(const SbArgs &A, uint64_t i, bool on, uint32_t lane, const Where &where) {
    // three copy jobs per lane: key suffix, value, index key
    uint8_t *kd = nullptr, *vd = nullptr, *xd = nullptr;
    const uint8_t *ks = nullptr, *vs = nullptr, *xs = nullptr;
    uint64_t kn = 0, vn = 0, xn = 0;
    if (on) {
        const lv_wb_op o = load_op(A.ops + A.order[i]);
        const SbBlockAt B = where.block(i);
        const uint64_t s = B.s, raw = B.raw;
        const bool restart = (i - s) % A.R == 0;
        uint64_t r;
        const uint64_t rel = i > s ? sb_buffer(A, s, i - 1, &r) : 0;
        const uint64_t ulen = o.key_len, klen = ulen + 8, sh = restart ? 0 : A.shared[i];
        uint8_t *p = A.file + B.at + rel;
        p = put_varint(p, sh);
        p = put_varint(p, klen - sh);
        p = put_varint(p, o.val_len);
        if (sh < ulen) {
            kd = p;
            ks = A.payload + o.key_off + sh;
            kn = ulen - sh;
            p += kn;
        }
        for (uint32_t t = sh > ulen ? static_cast<uint32_t>(sh - ulen) : 0; t < 8; ++t)
            *p++ = static_cast<uint8_t>(o.tag >> (8 * t));
        vd = p;
        vs = A.payload + o.val_off;
        vn = o.val_len;
        const uint64_t cnt = static_cast<uint64_t>(A.nxt[s]) - s, nrest = (cnt + A.R - 1) / A.R;
        uint8_t *arr = A.file + B.at + raw - 4 - 4 * nrest;  // the block's restart array
        if (restart) sb_put_fixed32(arr + 4 * ((i - s) / A.R), static_cast<uint32_t>(rel));
        if (i == s) {
            sb_put_fixed32(arr + 4 * nrest, static_cast<uint32_t>(nrest));
            // the block's index entry: shared = 0, the key, the handle
            const uint64_t e = s + cnt - 1;
            const lv_wb_op le = load_op(A.ops + A.order[e]);
            const SbIndexAt X = where.index(i, B);
            const SbIndexEntry x = sb_index_entry(A, e, X.last, le, B.off, raw);
            const uint64_t at = X.end - x.size;
            sb_put_fixed32(X.ix + X.idx_bytes + 4 * X.b, static_cast<uint32_t>(at));
            uint8_t *q = X.ix + at;
            q = put_varint(q, 0);
            q = put_varint(q, x.klen);
            q = put_varint(q, x.hlen);
            xd = q;
            xs = A.payload + le.key_off;
            xn = x.sep.copy;
            q += xn;
            uint64_t tg = le.tag;
            if (x.sep.bump) {
                *q++ = static_cast<uint8_t>(xs[xn] + 1);
                tg = (LV_MT_MAX_SEQUENCE << 8) | 1u;  // MAXTAG
            }
            for (uint32_t t = 0; t < 8; ++t) *q++ = static_cast<uint8_t>(tg >> (8 * t));
            q = put_varint(q, B.off);
            q = put_varint(q, raw);
        }
    }
    group_copy<kSbCopyLanes, kSbWaveCopy>(kd, ks, kn, lane);
    group_copy<kSbCopyLanes, kSbWaveCopy>(vd, vs, vn, lane);
    if (__ballot(xn != 0)) group_copy<kSbCopyLanes, kSbWaveCopy>(xd, xs, xn, lane);
}

// The build's kernels (sst_build.hip).
__global__ void sb_init(const SbArgs A);
__global__ void sb_sizes(const SbArgs A);
__global__ void sb_carry(const SbArgs A, uint32_t which);
__global__ void sb_next(const SbArgs A);
__global__ void sb_reach(const SbArgs A, uint32_t pass);
__global__ void sb_layout(const SbArgs A);
__global__ void sb_bloom_emit(const SbArgs A);
__global__ void sb_bloom_big(const SbArgs A);
__global__ void sb_bloom_offsets(const SbArgs A);

}  // namespace lvk
