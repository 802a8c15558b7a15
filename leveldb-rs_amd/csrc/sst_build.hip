// lv_sst_build_device: the sorted memtable of lv_memtable_build_device written
// as a complete SSTable image in HBM (include/lvgpu/table.h spells the format
// out; csrc/sst_build.cc is the serial twin).  lv_sst_build_bloom_device is
// the same call with a filter policy: the same kernels with SbArgs::bpk != 0,
// and the four sb_bloom_* kernels listed below.
//
// Block boundaries are a serial chain: where block b ends decides which
// entries of block b + 1 are restarts, and so their sizes.  The chain is cut
// like this.  With i a position in d_order:
//
//   nr[i]  the encoded size of entry i when it is not a restart (its shared
//          prefix with entry i - 1 over internal-key bytes taken off),
//   d[i]   what it costs more as a restart (shared = 0),
//   P      the inclusive scan of nr, S the scan of d with stride
//          restart_interval (S[i] = d[i] + S[i - R]).
//
// For a block that starts at s, the buffer after entry e is
// P[e] - P[s - 1] + S[last restart <= e] - S[s - R], its estimate that plus
// 4 per restart plus 4, monotone in e: next(s), the first entry after the
// block that would start at s, is a bounded binary search for every s at once.
// The true block starts are the entries reachable from 0 along next: pointer
// doubling marks them (a flag array extended, the jump array squared, per
// pass).  Two more scans over the start flags give every block its id and
// file offset, and every index entry (one per block, shared = 0) its place.
//
//   sb_init    one thread zeroes the call's head in the workspace.
//   sb_sizes   per tile of kSbTile entries: shared, nr, d (every order index
//              and extent checked: LV_SST_BUILD_NO_TABLE) and the tile-local
//              scans of P and S in LDS, with the tile's sums.
//   sb_carry   the exclusive scan of the tiles' sums, a wave per column (P,
//              and one column per residue of R for S); later the same kernel
//              over the layout's and the index's columns.
//   sb_next    next(s) for every s.
//   sb_reach   one doubling pass.
//   sb_layout  per block start: raw size (BLOCK_LARGE) -> tile scans of the
//              block count and of the bytes.
//   sb_index   per block start: id, offset, handle (into the workspace), the
//              separator's and so the index entry's size -> tile scan.
//   sb_plan    one thread: the totals and the status, decided once before
//              anything is written.
//   sb_emit    a lane per entry: its varints, key suffix, tag bytes, value,
//              its restart slot if it is one; a block's first entry also
//              writes the restart count and the block's index entry.  A key
//              suffix or value of kSbWaveCopy bytes or more is copied by
//              kSbCopyLanes lanes of the wave (64 / kSbCopyLanes such copies at
//              a time) in 16-byte granules of the destination's alignment.
//   sb_tail    d_handles and the padding of the workspace copy, the
//              metaindex block, the index's count, the footer.
//   with a filter policy (table.h, "Bloom filter blocks"), by block id:
//   sb_bloom_sizes    (before the plan) per data block whether it is the first
//              of its 2 KiB window of file offsets, the window's key count
//              (the entries up to the first block of a later window) and its
//              filter's size -> tile scan, and sb_carry once more.
//   sb_bloom_emit     (behind sb_emit) a wave per filter: bits zeroed in LDS,
//              the lanes hash the window's user keys and OR the k bits in
//              with LDS atomics, plain stores of the destination's alignment.
//              A filter beyond kSbBloomLds bytes is stored as zeros.
//   sb_bloom_big      the bits of those, by atomic OR on aligned dwords of
//              d_file; the launch stores nothing else.
//   sb_bloom_offsets  a lane per window: its filter's start offset.
//   sb_tail then also writes array_offset, the base byte and the metaindex
//   entry; the filter block joins the index block in the CRC batch.
//   the seal   sst_blocks_kernel<seal> (sst.hip) over the workspace handles of
//              the data blocks and the metaindex block, padded to
//              block_cap + 2 with {2^64 - 1, 0}, which it skips.  The index
//              block, which grows with the table, is a one-buffer batch of
//              the offsets API (its long-buffer split) and sb_index_trailer.
//
// The launch sequence depends only on what the host holds (op_cap, block_cap,
// restart_interval for the first carry's grid, file_cap == 0 to leave out the
// trailer launches), never on the device-side counts.  No workgroup
// waits on another inside a launch; every search loop is bounded.  All sizes
// and positions are u64.
//
// The tile scan, the carries' wave scan, the shared copy and the op loads are
// lvk/stage.h's (tile_scan, carry_scan, group_copy, load_op), instantiated
// with this file's tile, thread count and copy knobs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/table.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/knobs.h"
#include "lvk/sst_build.h"
#include "lvk/sst_read.h"
#include "lvk/stage.h"

namespace lvk {

// (The call's arguments, the size algebra, the separator, the index entry and
// the body of the entry emit are lvk/sst_build.h's: compact_output.hip shares
// them.)
constexpr uint32_t kSbBloomLds = 2048;  // bytes of filter bits a wave holds in LDS (1,638 keys at 10 bits per key)
static_assert(kSbBloomLds % 4 == 0, "whole LDS words");

// Byte i of the internal key (user key at k, ulen bytes, then the tag LE).
__device__ __forceinline__ uint32_t sb_ikey_at(const uint8_t *k, uint64_t ulen, uint64_t tag, uint64_t i) {
    return i < ulen ? k[i] : static_cast<uint32_t>(tag >> (8 * (i - ulen))) & 0xffu;
}

// Common-prefix length of a[0, m) and b[0, m): whole 8-byte words, then bytes.
__device__ __forceinline__ uint64_t sb_common(const uint8_t *a, const uint8_t *b, uint64_t m) {
    uint64_t i = 0;
    for (; i + 8 <= m; i += 8) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + i, 8);
        __builtin_memcpy(&y, b + i, 8);
        if (x != y) return i + (static_cast<uint32_t>(__builtin_ctzll(x ^ y)) >> 3);  // little-endian: the lowest differing byte
    }
    for (; i < m && a[i] == b[i]; ++i) {
    }
    return i;
}

// Common-prefix length of two internal keys.
__device__ __forceinline__ uint64_t sb_shared(const SbArgs &A, const lv_wb_op &p, const lv_wb_op &c) {
    const uint8_t *kp = A.payload + p.key_off, *kc = A.payload + c.key_off;
    const uint64_t m = p.key_len < c.key_len ? p.key_len : c.key_len;
    uint64_t s = sb_common(kp, kc, m);
    if (s < m) return s;
    for (uint32_t k = 0; k < 8; ++k, ++s)  // the shorter key's tag bytes: at most 8 more
        if (sb_ikey_at(kp, p.key_len, p.tag, s) != sb_ikey_at(kc, c.key_len, c.tag, s)) break;
    return s;
}

// Kernel 0 (one thread): the head.  A kernel, not a memset: the call is a
// chain of kernel launches only, which is what a captured graph replays.
__global__ void sb_init(const SbArgs A) {
    SbHead h{};
    *A.head = h;
    if (A.bpk) *A.bh = SbBloomHead{};
    if (A.mf) *A.ch = CoHead{};
}

// Kernel 1: sizes and the tile-local scans of P and S.
__global__ __launch_bounds__(kSbThreads) void sb_sizes(const SbArgs A) {
    __shared__ uint64_t s_p[kSbTile], s_s[kSbTile];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = sb_entries(A);
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSbTile;
    if (base >= n) return;
    const uint32_t cnt = static_cast<uint32_t>(n - base < kSbTile ? n - base : kSbTile);
    int bad = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        uint64_t nr = 0, d = 0;
        if (j < cnt) {
            const uint64_t i = base + j;
            const uint32_t oi = A.order[i], pi = i ? A.order[i - 1] : oi;
            uint64_t sh = 0;
            if (oi >= A.op_cap || pi >= A.op_cap) {
                bad = 1;
            } else {
                const lv_wb_op o = load_op(A.ops + oi), p = load_op(A.ops + pi);
                if (!extent_ok(o.key_off, o.key_len, A.payload_bytes) ||
                    !extent_ok(o.val_off, o.val_len, A.payload_bytes) ||
                    !extent_ok(p.key_off, p.key_len, A.payload_bytes)) {
                    bad = 1;
                } else {
                    if (i) sh = sb_shared(A, p, o);
                    const uint64_t klen = static_cast<uint64_t>(o.key_len) + 8, vlen = o.val_len;
                    nr = varint_len(sh) + varint_len(klen - sh) + varint_len(vlen) + (klen - sh) + vlen;
                    d = 1 + varint_len(klen) + varint_len(vlen) + klen + vlen - nr;
                }
            }
            A.shared[i] = sh;
        }
        s_p[j] = nr;
        s_s[j] = d;
    }
    if (__syncthreads_or(bad)) {  // not the memtable build's arguments: no table
        if (tid == 0) atomicOr(&A.head->bad, 1u);
        return;
    }
    tile_scan<kSbTile, kSbThreads>(s_p, 1, tid);
    tile_scan<kSbTile, kSbThreads>(s_s, A.R, tid);
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        if (j < cnt) {
            A.Pl[base + j] = s_p[j];
            A.Sl[base + j] = s_s[j];
        }
    }
    if (tid == 0) A.cP[blockIdx.x] = s_p[cnt - 1];
    for (uint32_t c = tid; c < A.R; c += kSbThreads) {  // the tile's sum of residue c: its last member's scan
        const uint32_t r0 = static_cast<uint32_t>((c + A.R - base % A.R) % A.R);
        A.cS[static_cast<uint64_t>(blockIdx.x) * A.R + c] = r0 < cnt ? s_s[r0 + (cnt - 1 - r0) / A.R * A.R] : 0;
    }
}

// Kernel 2: the exclusive scan over the tiles of column c, in place; one wave
// per column.  Column c is col[c + t * stride], t < tiles; its sum goes to
// total[c] when total is not null.  which: 0 = {P, S residues} (cP is column
// R), 1 = {block count, file bytes}, 2 = {index bytes}, 3 = {filter bytes};
// for several files (compact_output.hip) 4 = {file count}, 5 = {index bytes,
// filter bytes}, both by block id, and 6 = {file bytes, bound bytes, windows}
// by file.
__global__ __launch_bounds__(kSbThreads) void sb_carry(const SbArgs A, uint32_t which) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = blockIdx.x * (kSbThreads / 64) + (threadIdx.x >> 6);
    const uint64_t n = sb_entries(A);
    if (!n || A.head->bad) return;
    // (the filters' column is by block id, as 4 and 5 are; 6 is by file)
    const uint64_t units = which == 6 ? static_cast<uint64_t>(A.ch->nfiles)
                           : which >= 3 ? static_cast<uint64_t>(A.head->nblocks)
                                        : n;
    const uint64_t tiles = (units + kSbTile - 1) / kSbTile;
    uint64_t *col;
    uint64_t stride = 1;
    unsigned long long *total = nullptr;
    if (which == 4) {  // several files: the file count over the blocks
        if (c > 0) return;
        col = A.cK;
        total = &A.ch->nfiles;
    } else if (which == 5) {  // ... the index bytes and the filters' bytes over the blocks
        if (c > (A.bpk ? 1u : 0u)) return;
        col = c ? A.cF : A.cI;
        total = c ? &A.bh->filt_bytes : nullptr;  // (a file's index bytes are differences of the scan)
    } else if (which == 6) {  // ... the files' bytes, bound bytes and windows
        if (c > 2) return;
        col = c == 0 ? A.cA : c == 1 ? A.cU : A.cW;
        total = c == 0 ? &A.ch->arena_al : c == 1 ? &A.ch->bound_bytes : &A.ch->windows;
    } else if (which == 0) {
        if (c > A.R) return;
        col = c == A.R ? A.cP : A.cS + c;
        stride = c == A.R ? 1 : A.R;
    } else if (which == 1) {
        if (c > 1) return;
        col = c ? A.cB : A.cC;
        total = c ? &A.head->data_bytes : &A.head->nblocks;
    } else if (which == 2) {
        if (c > 0) return;
        col = A.cI;
        total = &A.head->idx_bytes;
    } else {
        if (c > 0) return;
        col = A.cF;
        total = &A.bh->filt_bytes;
    }
    const uint64_t run = carry_scan(col, stride, tiles, lane);
    if (total && lane == 0) *total = run;
}

// Kernel 3: next(s), and the start flags' initial state.
__global__ __launch_bounds__(kSbThreads) void sb_next(const SbArgs A) {
    const uint64_t n = sb_entries(A);
    const uint64_t s = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x;
    if (s >= n || A.head->bad) return;
    // an entry is at least 3 bytes: bs / 3 + 1 entries reach block_size
    uint64_t lo = s, hi = s + A.bs / 3 + 1;
    if (hi > n - 1) hi = n - 1;
    for (uint32_t it = 0; it < 40 && lo < hi; ++it) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (sb_estimate(A, s, mid) >= A.bs)
            hi = mid;
        else
            lo = mid + 1;
    }
    A.nxt[s] = static_cast<uint32_t>(lo + 1);
    A.F[s] = s == 0;
}

// Kernel 4: doubling pass p.  F holds the first 2^p block starts (and maybe
// more of them: a flag set during this pass is a true start too), src is
// next^(2^p).  A pass with 2^p >= n has nothing left to mark.
__global__ __launch_bounds__(kSbThreads) void sb_reach(const SbArgs A, uint32_t pass) {
    const uint64_t n = sb_entries(A);
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x;
    if (A.head->bad) return;
    sb_reach_pass(n, i, pass, A.nxt, A.J, A.F);
}

// Kernel 5: per block start its raw size; tile scans of the count and the bytes.
__global__ __launch_bounds__(kSbThreads) void sb_layout(const SbArgs A) {
    __shared__ uint64_t s_c[kSbTile], s_b[kSbTile];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = sb_entries(A);
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSbTile;
    if (base >= n || A.head->bad) return;
    const uint32_t cnt = static_cast<uint32_t>(n - base < kSbTile ? n - base : kSbTile);
    uint32_t large = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        uint64_t c = 0, b = 0;
        if (j < cnt && A.F[base + j]) {
            const uint64_t raw = sb_estimate(A, base + j, static_cast<uint64_t>(A.nxt[base + j]) - 1);
            large |= raw >= kSbLarge;
            c = 1;
            b = raw + LV_SST_TRAILER_SIZE;
        }
        s_c[j] = c;
        s_b[j] = b;
    }
    if (large) atomicOr(&A.head->large, 1u);
    __syncthreads();
    tile_scan<kSbTile, kSbThreads>(s_c, 1, tid);
    tile_scan<kSbTile, kSbThreads>(s_b, 1, tid);
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        if (j < cnt) {
            A.Cl[base + j] = s_c[j];
            A.Bl[base + j] = s_b[j];
        }
    }
    if (tid == 0) {
        A.cC[blockIdx.x] = s_c[cnt - 1];
        A.cB[blockIdx.x] = s_b[cnt - 1];
    }
}


// Kernel 6: per block start its id, offset and handle; the index entry's size
// and its tile scan.
__global__ __launch_bounds__(kSbThreads) void sb_index(const SbArgs A) {
    __shared__ uint64_t s_i[kSbTile];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = sb_entries(A);
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSbTile;
    if (base >= n || A.head->bad) return;
    const uint32_t cnt = static_cast<uint32_t>(n - base < kSbTile ? n - base : kSbTile);
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        uint64_t v = 0;
        if (j < cnt && A.F[base + j]) {
            const uint64_t s = base + j, e = static_cast<uint64_t>(A.nxt[s]) - 1, t = s / kSbTile;
            const uint64_t raw = sb_estimate(A, s, e);
            const uint64_t b = A.Cl[s] + A.cC[t] - 1, off = A.Bl[s] + A.cB[t] - (raw + LV_SST_TRAILER_SIZE);
            if (b < A.block_cap) {
                A.blk_start[b] = static_cast<uint32_t>(s);
                A.wsh[2 * b] = off;
                A.wsh[2 * b + 1] = raw;
            }
            if (A.bpk) {
                A.boff[b] = off;
                A.bstart[b] = static_cast<uint32_t>(s);
            }
            v = sb_index_entry(A, e, e + 1 >= n, load_op(A.ops + A.order[e]), off, raw).size;
        }
        s_i[j] = v;
    }
    __syncthreads();
    tile_scan<kSbTile, kSbThreads>(s_i, 1, tid);
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        if (j < cnt) A.Il[base + j] = s_i[j];
    }
    if (tid == 0) A.cI[blockIdx.x] = s_i[cnt - 1];
}

// Kernel 7 (one thread): the totals and the status, once, before any byte of
// d_file or d_handles is written.
__global__ void sb_plan(const SbArgs A) {
    SbHead *h = A.head;
    lv_sst_build_totals t{};
    lv_sst_bloom_totals bt{};
    uint64_t n = A.mt->entries;
    if (A.mt->status || n > A.op_cap || h->bad) {
        t.status = LV_SST_BUILD_NO_TABLE;
        n = 0;
    }
    t.entries = n;
    if (n) {
        const uint64_t nb = h->nblocks;
        t.data_blocks = nb;
        t.metaindex_offset = h->data_bytes;
        t.metaindex_size = 8;
        if (A.bpk) {  // the filter block goes first; the metaindex block holds its entry
            const uint64_t last = A.boff[nb - 1] >> LV_SST_FILTER_BASE_LG, ends = h->data_bytes >> LV_SST_FILTER_BASE_LG;
            bt.filters = last + 1 > ends ? last + 1 : ends;
            bt.filter_offset = h->data_bytes;
            bt.filter_size = A.bh->filt_bytes + 4 * bt.filters + 5;
            bt.filter_keys = n;
            if (bt.filter_size >= kSbLarge) t.status |= LV_SST_BUILD_BLOCK_LARGE;
            t.metaindex_offset = bt.filter_offset + bt.filter_size + LV_SST_TRAILER_SIZE;
            t.metaindex_size = 3 + kSbBloomName + varint_len(bt.filter_offset) + varint_len(bt.filter_size) + 8;
        }
        t.index_offset = t.metaindex_offset + t.metaindex_size + LV_SST_TRAILER_SIZE;
        t.index_size = h->idx_bytes + 4 * nb + 4;
        t.file_bytes = t.index_offset + t.index_size + LV_SST_TRAILER_SIZE + LV_SST_FOOTER_SIZE;
        if (h->large || t.index_size >= kSbLarge) t.status |= LV_SST_BUILD_BLOCK_LARGE;
        if (nb > A.block_cap) t.status |= LV_SST_BUILD_HANDLE_OVER;
        if (t.file_bytes > A.file_cap) t.status |= LV_SST_BUILD_FILE_OVER;
        if (!t.status) {
            h->go = 1;
            h->meta_off = t.metaindex_offset;
            h->index_off = t.index_offset;
            h->index_size = t.index_size;
            uint64_t *w = A.wsh + 2 * nb;
            if (A.bpk) {
                A.bh->filter_off = *w++ = bt.filter_offset;
                A.bh->filter_size = *w++ = bt.filter_size;
                A.bh->filters = bt.filters;
                A.bh->meta_size = t.metaindex_size;
            }
            *w++ = t.metaindex_offset;
            *w++ = t.metaindex_size;
            *w++ = t.index_offset;
            *w++ = t.index_size;
        }
    }
    *A.totals = t;
    if (A.bpk) *A.btotals = t.status || !n ? lv_sst_bloom_totals{} : bt;
}

// One file at A.file: a block's place is its handle in the workspace, and the
// index entries are scanned by entry position.
struct SbOneFile {
    const SbArgs &A;
    __device__ __forceinline__ SbBlockAt block(uint64_t i) const {
        const uint64_t b = A.Cl[i] + A.cC[i / kSbTile] - 1;  // < block_cap: the plan checked
        return SbBlockAt{A.blk_start[b], A.wsh[2 * b], A.wsh[2 * b], A.wsh[2 * b + 1]};
    }
    __device__ __forceinline__ SbIndexAt index(uint64_t i, const SbBlockAt &B) const {
        const uint64_t n = sb_entries(A);
        return SbIndexAt{A.file + A.head->index_off, A.head->idx_bytes, A.Cl[i] + A.cC[i / kSbTile] - 1,
                         A.Il[i] + A.cI[i / kSbTile], static_cast<uint64_t>(A.nxt[B.s]) >= n};
    }
};

// Kernel 8: the entries, the restart arrays, the index entries.  Every lane of
// a wave stays to the end: the long copies are the wave's.
__global__ __launch_bounds__(kSbThreads) void sb_emit(const SbArgs A) {
    if (!A.head->go) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n = sb_entries(A);
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x;
    if (static_cast<uint64_t>(blockIdx.x) * kSbThreads >= n) return;
    sb_emit_entry(A, i, i < n, lane, SbOneFile{A});
}

// Kernel 9: d_handles and the workspace copy's padding; one thread writes the
// metaindex block, the index block's restart count and type byte, and the
// footer.  The index block is not the seal's: that kernel gives a block to a
// group of 16 lanes, right for blocks of about block_size, while an index
// block grows with the table (one entry per data block).  It goes to the offsets API as a one-buffer batch, whose
// long-buffer split spreads it over the device.
__global__ __launch_bounds__(kSbThreads) void sb_tail(const SbArgs A) {
    const SbHead *h = A.head;
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x;
    const bool go = h->go;
    const uint64_t extra = A.bpk ? 3 : 2;  // the pairs behind the data blocks'
    const uint64_t nh = go ? h->nblocks + extra : 0;
    if (j < A.block_cap + extra) {
        if (j < nh) {
            A.handles[2 * j] = A.wsh[2 * j];
            A.handles[2 * j + 1] = A.wsh[2 * j + 1];
        }
        // the seal's are the data blocks and the metaindex block (the last pair
        // but one); it skips a handle out of range without touching the file
        if (!(go && (j < h->nblocks || j + 2 == nh))) {
            A.wsh[2 * j] = ~0ull;
            A.wsh[2 * j + 1] = 0;
        }
    }
    if (j == 0) {
        A.idx_off[0] = go ? h->index_off : 0;
        A.idx_len[0] = go ? static_cast<uint32_t>(h->index_size + 1) : 0;  // (< 2^32 - 1: the plan checked)
        if (A.bpk) {
            A.idx_off[1] = go ? A.bh->filter_off : 0;
            A.idx_len[1] = go ? static_cast<uint32_t>(A.bh->filter_size + 1) : 0;
        }
    }
    if (j == 0 && go) {
        A.file[h->index_off + h->index_size] = LV_SST_NO_COMPRESSION;
        uint8_t *m = A.file + h->meta_off;
        uint64_t meta_size = 8;
        if (A.bpk) {
            const SbBloomHead *bh = A.bh;
            // the filter block's end: array_offset, the base, the type byte
            uint8_t *e = A.file + bh->filter_off + bh->filter_size;
            sb_put_fixed32(e - 5, static_cast<uint32_t>(bh->filt_bytes));
            e[-1] = LV_SST_FILTER_BASE_LG;
            e[0] = LV_SST_NO_COMPRESSION;
            // the metaindex block's one entry: shared 0, the name, the filter block's handle
            constexpr char name[] = LV_SST_BLOOM_NAME;
            meta_size = bh->meta_size;
            m = put_varint(m, 0);
            m = put_varint(m, kSbBloomName);
            m = put_varint(m, meta_size - 3 - kSbBloomName - 8);
            for (uint32_t t = 0; t < kSbBloomName; ++t) *m++ = static_cast<uint8_t>(name[t]);
            m = put_varint(m, bh->filter_off);
            m = put_varint(m, bh->filter_size);
        }
        sb_put_fixed32(m, 0);  // (an empty BlockBuilder: 00 00 00 00 01 00 00 00)
        sb_put_fixed32(m + 4, 1);
        sb_put_fixed32(A.file + h->index_off + h->idx_bytes + 4 * h->nblocks, static_cast<uint32_t>(h->nblocks));
        uint8_t *f = A.file + h->index_off + h->index_size + LV_SST_TRAILER_SIZE, *q = f;
        q = put_varint(q, h->meta_off);
        q = put_varint(q, meta_size);
        q = put_varint(q, h->index_off);
        q = put_varint(q, h->index_size);
        while (q < f + 40) *q++ = 0;
        for (uint32_t t = 0; t < 8; ++t) *q++ = static_cast<uint8_t>(LV_SST_MAGIC >> (8 * t));
    }
}

// Kernel 10 (one thread): the index block's trailer from the batch's masked crc.
__global__ void sb_index_trailer(const SbArgs A) {
    const SbHead *h = A.head;
    if (!h->go) return;
    sb_put_fixed32(A.file + h->index_off + h->index_size + 1, A.idx_crc[0]);
    if (A.bpk) sb_put_fixed32(A.file + A.bh->filter_off + A.bh->filter_size + 1, A.idx_crc[1]);
}

// ---- the filter block (lv_sst_build_bloom_device) ----


// Kernel B1, a lane per data block (by id, after sb_index and the layout's
// carry): whether it is the first block of its window, then the keys of the
// window (the entries up to the first block of a later window, found by a
// bounded binary search over the block offsets) and its filter's size; the
// tile scan of the sizes.
__global__ __launch_bounds__(kSbThreads) void sb_bloom_sizes(const SbArgs A) {
    __shared__ uint64_t s_f[kSbTile];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = sb_entries(A);
    if (!n || A.head->bad) return;
    const uint64_t nb = A.head->nblocks;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSbTile;
    if (base >= nb) return;
    const uint32_t cnt = static_cast<uint32_t>(nb - base < kSbTile ? nb - base : kSbTile);
    uint64_t own[kSbPer];
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        uint64_t v = 0;
        if (j < cnt) {
            const uint64_t b = base + j, w = A.boff[b] >> LV_SST_FILTER_BASE_LG;
            uint32_t keys = 0;
            if (b == 0 || (A.boff[b - 1] >> LV_SST_FILTER_BASE_LG) != w) {
                const uint64_t lim = (w + 1) << LV_SST_FILTER_BASE_LG;
                uint64_t lo = b + 1, hi = nb;
                for (uint32_t it = 0; it < 40 && lo < hi; ++it) {
                    const uint64_t mid = lo + (hi - lo) / 2;
                    if (A.boff[mid] >= lim)
                        hi = mid;
                    else
                        lo = mid + 1;
                }
                keys = static_cast<uint32_t>((lo < nb ? A.bstart[lo] : n) - A.bstart[b]);
                v = sb_bloom_bytes(keys, A.bpk) + 1;
                if (v - 1 > kSbBloomLds) atomicOr(&A.bh->big, 1ull);
            }
            A.Fn[b] = keys;
        }
        own[k] = v;
        s_f[j] = v;
    }
    __syncthreads();
    tile_scan<kSbTile, kSbThreads>(s_f, 1, tid);
#pragma unroll
    for (uint32_t k = 0; k < kSbPer; ++k) {
        const uint32_t j = tid + k * kSbThreads;
        if (j < cnt) A.Fl[base + j] = s_f[j] - own[k];
    }
    if (tid == 0) A.cF[blockIdx.x] = s_f[cnt - 1];
}

// total bytes at dst from the LDS bytes at src: dst's ragged head and tail
// byte by byte, between them dwords of dst's alignment.  One wave.
__device__ __forceinline__ void sb_bloom_store(uint8_t *dst, const uint8_t *src, uint32_t total, uint32_t lane) {
    uint32_t head = static_cast<uint32_t>((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u);
    if (head > total) head = total;
    const uint32_t words = (total - head) / 4, tail = (total - head) % 4;
    if (lane < head) dst[lane] = src[lane];
    for (uint32_t g = lane; g < words; g += 64) {
        const uint8_t *p = src + head + 4 * g;
        *reinterpret_cast<uint32_t *>(dst + head + 4 * g) = lvr::le32(p);
    }
    if (lane < tail) dst[head + 4 * words + lane] = src[head + 4 * words + lane];
}

// Kernel B2, the filter emit: a wave per first-of-its-window block in a
// grid-stride loop over the data blocks.  The filter's bits are zeroed in the
// wave's LDS, each lane hashes user keys of the window and ORs their k bits in
// with LDS atomics (order-free: the bytes do not depend on the schedule), and
// the wave stores the bytes and the k byte.  A filter beyond kSbBloomLds bytes
// is stored as zeros here; sb_bloom_big sets its bits.
__global__ __launch_bounds__(kSbThreads) void sb_bloom_emit(const SbArgs A) {
    __shared__ uint32_t s_bits[kSbThreads / 64][kSbBloomLds / 4 + 1];
    if (!A.head->go) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t nb = A.head->nblocks, step = static_cast<uint64_t>(gridDim.x) * (kSbThreads / 64);
    const uint32_t k = sb_bloom_k(A.bpk);
    uint32_t *bits = s_bits[wave];
    for (uint64_t b = static_cast<uint64_t>(blockIdx.x) * (kSbThreads / 64) + wave; b < nb; b += step) {  // wave-uniform
        const uint32_t keys = A.Fn[b];
        if (!keys) continue;
        const uint64_t bytes = sb_bloom_bytes(keys, A.bpk);
        uint8_t *dst = sb_filter_at(A, b);
        if (bytes > kSbBloomLds) {
            const uint64_t head = (4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u;  // < 8 <= bytes
            const uint64_t words = (bytes - head) / 4, tail = (bytes - head) % 4;
            if (lane < head) dst[lane] = 0;
            for (uint64_t g = lane; g < words; g += 64) *reinterpret_cast<uint32_t *>(dst + head + 4 * g) = 0;
            if (lane < tail) dst[head + 4 * words + lane] = 0;
            if (lane == 0) dst[bytes] = static_cast<uint8_t>(k);
            if (A.mf && lane == 0) atomicOr(&A.bh->big, 1ull);  // (one file: sb_bloom_sizes said so before the plan)
            continue;
        }
        const uint32_t nbytes = static_cast<uint32_t>(bytes), nbits = nbytes * 8;
        for (uint32_t w = lane; w <= nbytes / 4; w += 64) bits[w] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0) atomicOr(&bits[nbytes / 4], k << (8 * (nbytes % 4)));  // the k byte
        const uint64_t s = A.bstart[b];
        for (uint32_t i = lane; i < keys; i += 64) {
            const lv_wb_op o = load_op(A.ops + A.order[s + i]);
            uint32_t h = lvr::hash(A.payload + o.key_off, o.key_len, lvr::kBloomSeed);
            const uint32_t delta = (h >> 17) | (h << 15);
            for (uint32_t j = 0; j < k; ++j) {
                const uint32_t pos = h % nbits;
                atomicOr(&bits[pos >> 5], 1u << (pos & 31u));  // little-endian: byte pos / 8, bit pos % 8
                h += delta;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        sb_bloom_store(dst, reinterpret_cast<const uint8_t *>(bits), nbytes + 1, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the stores' LDS reads precede the next filter's zeroing
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// Kernel B3: the bits of the filters sb_bloom_emit zero-filled, set with
// atomic ORs on aligned dwords of d_file.  This launch stores nothing else, so
// a dword such a filter shares with its neighbours keeps their bytes.
__global__ __launch_bounds__(kSbThreads) void sb_bloom_big(const SbArgs A) {
    if (!A.head->go || !A.bh->big) return;  // (sb_bloom_sizes found none: the usual case)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t nb = A.head->nblocks, step = static_cast<uint64_t>(gridDim.x) * (kSbThreads / 64);
    const uint32_t k = sb_bloom_k(A.bpk);
    for (uint64_t b = static_cast<uint64_t>(blockIdx.x) * (kSbThreads / 64) + wave; b < nb; b += step) {
        const uint32_t keys = A.Fn[b];
        if (!keys) continue;
        const uint64_t bytes = sb_bloom_bytes(keys, A.bpk), nbits = bytes * 8;
        if (bytes <= kSbBloomLds) continue;
        const uintptr_t dst = reinterpret_cast<uintptr_t>(sb_filter_at(A, b));
        const uint64_t s = A.bstart[b];
        for (uint32_t i = lane; i < keys; i += 64) {
            const lv_wb_op o = load_op(A.ops + A.order[s + i]);
            uint32_t h = lvr::hash(A.payload + o.key_off, o.key_len, lvr::kBloomSeed);
            const uint32_t delta = (h >> 17) | (h << 15);
            for (uint32_t j = 0; j < k; ++j) {
                const uint64_t pos = h % nbits;
                const uintptr_t at = dst + pos / 8;
                atomicOr(reinterpret_cast<uint32_t *>(at & ~static_cast<uintptr_t>(3)),
                         1u << (8 * static_cast<uint32_t>(at & 3u) + static_cast<uint32_t>(pos % 8)));
                h += delta;
            }
        }
    }
}

// Kernel B4, a lane per window in a grid-stride loop: the filter's start
// offset.  The first block at or beyond the window's first byte is the first
// of its own window, whose filter starts where this window's does (an empty
// window's filter is zero bytes); with no such block every filter lies before.
__global__ __launch_bounds__(kSbThreads) void sb_bloom_offsets(const SbArgs A) {
    if (!A.head->go) return;
    const uint64_t step = static_cast<uint64_t>(gridDim.x) * kSbThreads;
    if (A.mf) {  // several files: the windows are numbered file after file
        const uint64_t W = A.ch->windows;
        for (uint64_t f = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x; f < W; f += step) {
            uint8_t *slot;
            uint32_t value;
            co_window(A, f, &slot, &value);
            sb_put_fixed32(slot, value);
        }
        return;
    }
    const uint64_t nb = A.head->nblocks, F = A.bh->filters, total = A.bh->filt_bytes;
    uint8_t *arr = A.file + A.bh->filter_off + total;
    for (uint64_t f = static_cast<uint64_t>(blockIdx.x) * kSbThreads + threadIdx.x; f < F; f += step) {
        const uint64_t lim = f << LV_SST_FILTER_BASE_LG;
        uint64_t lo = 0, hi = nb;
        for (uint32_t it = 0; it < 40 && lo < hi; ++it) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (A.boff[mid] >= lim)
                hi = mid;
            else
                lo = mid + 1;
        }
        sb_put_fixed32(arr + 4 * f, static_cast<uint32_t>(lo < nb ? A.Fl[lo] + A.cF[lo / kSbTile] : total));
    }
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxOpCap = 0xfffffffeull;
constexpr uint64_t kMaxBlockCap = 0xfffffffcull;

constexpr uint64_t sb_tiles(uint64_t cap) { return (cap + lvk::kSbTile - 1) / lvk::kSbTile; }

// The workspace for op_cap = cap and block_cap = bc, region by region: fills
// A's workspace pointers and returns the CRC batch's sub-workspace
// (lv_crc32c_workspace_bytes(1) bytes).  bloom: lv_sst_build_bloom_device's,
// with a third handle, a second buffer in the batch and its own regions last.
uint8_t *sb_carve(Carve &C, uint64_t cap, uint64_t bc, lvk::SbArgs &A, bool bloom = false) {
    const uint64_t tiles = sb_tiles(cap);
    A.head = C.take<lvk::SbHead>(1);
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
    A.blk_start = C.take<uint32_t>(bc);
    const uint32_t nbuf = bloom ? 2 : 1;
    A.wsh = C.take<uint64_t>(2 * (bc + 1 + nbuf));
    if (uint32_t *idx = C.take<uint32_t>(4 * nbuf)) {  // the batch: {offsets (u64), lengths, crcs}
        A.idx_off = reinterpret_cast<uint64_t *>(idx);
        A.idx_len = idx + 2 * nbuf;
        A.idx_crc = idx + 3 * nbuf;
    }
    uint8_t *crc_ws = C.take<uint8_t>(lv_crc32c_workspace_bytes(nbuf));
    if (bloom) {
        A.bh = C.take<lvk::SbBloomHead>(1);
        A.boff = C.take<uint64_t>(cap);
        A.bstart = C.take<uint32_t>(cap);
        A.Fn = C.take<uint32_t>(cap);
        A.Fl = C.take<uint64_t>(cap);
        A.cF = C.take<uint64_t>(tiles);
    }
    return crc_ws;
}

// lv_sst_build_device (bloom == NULL) and lv_sst_build_bloom_device.
int sb_build(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops, const uint32_t *d_order,
             const lv_mt_totals *d_mt_totals, size_t op_cap, const lv_sst_build_options *opt,
             const lv_sst_bloom_options *bloom, uint8_t *d_file, uint64_t file_cap, uint64_t *d_handles,
             size_t block_cap, lv_sst_build_totals *d_totals, lv_sst_bloom_totals *d_bloom_totals, uint32_t flags,
             void *d_workspace, size_t workspace_bytes, void *stream);

}  // namespace

// sb_bloom_emit / sb_bloom_big: a wave per data block, so a workgroup takes
// kSbThreads / 64 blocks a trip; the table has at most op_cap blocks.
uint64_t lvgpu_internal::sb_bloom_grid(uint64_t op_cap, uint64_t *per_trip) {
    constexpr uint64_t kWaves = lvk::kSbThreads / 64;
    if (per_trip) *per_trip = kWaves;
    return std::min<uint64_t>((op_cap + kWaves - 1) / kWaves, 1024);
}
// sb_carry scans 64 tile sums a round (lvk::carry_scan).
uint64_t lvgpu_internal::sb_carry_round() { return 64ull * lvk::kSbTile; }
// sb_bloom_offsets: a lane per filter window, kSbThreads windows a workgroup trip.
uint64_t lvgpu_internal::sb_bloom_offsets_grid(uint64_t windows, uint64_t *per_trip) {
    if (per_trip) *per_trip = lvk::kSbThreads;
    return std::min<uint64_t>(windows / lvk::kSbThreads + 1, 1024);
}

extern "C" {

size_t lv_sst_build_workspace_bytes(size_t op_cap, size_t block_cap) {
    if (op_cap > kMaxOpCap || block_cap > kMaxBlockCap) return 0;
    lvk::SbArgs A{};
    Carve C{nullptr};
    sb_carve(C, op_cap, block_cap, A);
    return C.at;
}

size_t lv_sst_build_bloom_workspace_bytes(size_t op_cap, size_t block_cap) {
    if (op_cap > kMaxOpCap || block_cap > kMaxBlockCap) return 0;
    lvk::SbArgs A{};
    Carve C{nullptr};
    sb_carve(C, op_cap, block_cap, A, true);
    return C.at;
}

int lv_sst_build_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops, const uint32_t *d_order,
                        const lv_mt_totals *d_mt_totals, size_t op_cap, const lv_sst_build_options *opt,
                        uint8_t *d_file, uint64_t file_cap, uint64_t *d_handles, size_t block_cap,
                        lv_sst_build_totals *d_totals, uint32_t flags, void *d_workspace, size_t workspace_bytes,
                        void *stream) {
    return sb_build(d_payload, payload_bytes, d_ops, d_order, d_mt_totals, op_cap, opt, nullptr, d_file, file_cap,
                    d_handles, block_cap, d_totals, nullptr, flags, d_workspace, workspace_bytes, stream);
}

int lv_sst_build_bloom_device(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops,
                              const uint32_t *d_order, const lv_mt_totals *d_mt_totals, size_t op_cap,
                              const lv_sst_build_options *opt, const lv_sst_bloom_options *bloom, uint8_t *d_file,
                              uint64_t file_cap, uint64_t *d_handles, size_t block_cap, lv_sst_build_totals *d_totals,
                              lv_sst_bloom_totals *d_bloom_totals, uint32_t flags, void *d_workspace,
                              size_t workspace_bytes, void *stream) {
    g_err.clear();
    if (!bloom) return set_err(LV_ERR_INVALID, "null bloom options");
    if (bloom->bits_per_key < 1 || bloom->bits_per_key > 64) return set_err(LV_ERR_INVALID, "bits_per_key must be in [1, 64]");
    if (bloom->reserved) return set_err(LV_ERR_INVALID, "bloom options: reserved must be 0");
    if (!d_bloom_totals) return set_err(LV_ERR_INVALID, "null d_bloom_totals");
    if (misaligned(d_bloom_totals, 8)) return set_err(LV_ERR_INVALID, "d_bloom_totals must be 8-byte aligned");
    return sb_build(d_payload, payload_bytes, d_ops, d_order, d_mt_totals, op_cap, opt, bloom, d_file, file_cap,
                    d_handles, block_cap, d_totals, d_bloom_totals, flags, d_workspace, workspace_bytes, stream);
}

}  // extern "C"

namespace {

int sb_build(const uint8_t *d_payload, size_t payload_bytes, const lv_wb_op *d_ops, const uint32_t *d_order,
             const lv_mt_totals *d_mt_totals, size_t op_cap, const lv_sst_build_options *opt,
             const lv_sst_bloom_options *bloom, uint8_t *d_file, uint64_t file_cap, uint64_t *d_handles,
             size_t block_cap, lv_sst_build_totals *d_totals, lv_sst_bloom_totals *d_bloom_totals, uint32_t flags,
             void *d_workspace, size_t workspace_bytes, void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    const uint32_t bs = opt ? opt->block_size : LV_SST_DEFAULT_BLOCK_SIZE;
    const uint32_t ri = opt ? opt->restart_interval : LV_SST_DEFAULT_RESTART_INTERVAL;
    if (bs < 1 || bs > LV_SST_MAX_BLOCK_SIZE) return set_err(LV_ERR_INVALID, "block_size must be in [1, 2^30]");
    if (ri < 1 || ri > LV_SST_MAX_RESTART_INTERVAL)
        return set_err(LV_ERR_INVALID, "restart_interval must be in [1, 1024]");
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
    if (file_cap && !d_file) return set_err(LV_ERR_INVALID, "null d_file");
    if (misaligned(d_file, 16)) return set_err(LV_ERR_INVALID, "d_file must be 16-byte aligned");
    if (!d_handles) return set_err(LV_ERR_INVALID, "null d_handles");
    if (misaligned(d_handles, 8)) return set_err(LV_ERR_INVALID, "d_handles must be 8-byte aligned");
    if (!d_workspace) return set_err(LV_ERR_INVALID, "null workspace");
    if (misaligned(d_workspace, 16)) return set_err(LV_ERR_INVALID, "workspace must be 16-byte aligned");
    lvk::SbArgs A{};
    Carve C{static_cast<uint8_t *>(d_workspace)};
    uint8_t *crc_ws = sb_carve(C, op_cap, block_cap, A, bloom != nullptr);
    if (workspace_bytes < C.at) return set_err(LV_ERR_INVALID, "workspace too small");
    const uint32_t nbuf = bloom ? 2 : 1;  // the CRC batch's buffers; block_cap + 1 + nbuf handle pairs
    const uint64_t handle_bytes = (static_cast<uint64_t>(block_cap) + 1 + nbuf) * 16;
    const struct {
        const void *p;
        uint64_t bytes;
        const char *name;
    } ins[3] = {{d_payload, payload_bytes, "d_payload"},
                {d_ops, static_cast<uint64_t>(op_cap) * sizeof(lv_wb_op), "d_ops"},
                {d_order, static_cast<uint64_t>(op_cap) * sizeof(uint32_t), "d_order"}};
    for (const auto &in : ins) {
        if (overlaps(d_file, file_cap, in.p, in.bytes)) return set_err(LV_ERR_INVALID, std::string("d_file overlaps ") + in.name);
        if (overlaps(d_handles, handle_bytes, in.p, in.bytes))
            return set_err(LV_ERR_INVALID, std::string("d_handles overlaps ") + in.name);
    }
    if (overlaps(d_file, file_cap, d_handles, handle_bytes)) return set_err(LV_ERR_INVALID, "d_file overlaps d_handles");
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
    A.file = d_file;
    A.file_cap = file_cap;
    A.handles = d_handles;
    A.block_cap = block_cap;
    A.totals = d_totals;
    A.bpk = bloom ? bloom->bits_per_key : 0;
    A.btotals = d_bloom_totals;

    const dim3 b(lvk::kSbThreads);
    const uint32_t tiles = static_cast<uint32_t>(sb_tiles(op_cap));
    const uint32_t eg = static_cast<uint32_t>((static_cast<uint64_t>(op_cap) + lvk::kSbThreads - 1) / lvk::kSbThreads);
    constexpr uint32_t kWaves = lvk::kSbThreads / 64;
    hipLaunchKernelGGL(lvk::sb_init, dim3(1), dim3(1), 0, s, A);
    if (tiles) {
        hipLaunchKernelGGL(lvk::sb_sizes, dim3(tiles), b, 0, s, A);
        hipLaunchKernelGGL(lvk::sb_carry, dim3((ri + 1 + kWaves - 1) / kWaves), b, 0, s, A, 0u);
        hipLaunchKernelGGL(lvk::sb_next, dim3(eg), b, 0, s, A);
        for (uint32_t p = 0; (1ull << p) < op_cap; ++p) hipLaunchKernelGGL(lvk::sb_reach, dim3(eg), b, 0, s, A, p);
        hipLaunchKernelGGL(lvk::sb_layout, dim3(tiles), b, 0, s, A);
        hipLaunchKernelGGL(lvk::sb_carry, dim3(1), b, 0, s, A, 1u);
        hipLaunchKernelGGL(lvk::sb_index, dim3(tiles), b, 0, s, A);
        hipLaunchKernelGGL(lvk::sb_carry, dim3(1), b, 0, s, A, 2u);
        if (bloom) {
            hipLaunchKernelGGL(lvk::sb_bloom_sizes, dim3(tiles), b, 0, s, A);
            hipLaunchKernelGGL(lvk::sb_carry, dim3(1), b, 0, s, A, 3u);
        }
    }
    hipLaunchKernelGGL(lvk::sb_plan, dim3(1), dim3(1), 0, s, A);
    if (tiles) hipLaunchKernelGGL(lvk::sb_emit, dim3(eg), b, 0, s, A);
    if (tiles && bloom) {
        // a wave per data block, a lane per window: grid-stride loops over capped grids
        const uint32_t wg = static_cast<uint32_t>(lvgpu_internal::sb_bloom_grid(op_cap));
        const uint32_t og = static_cast<uint32_t>(lvgpu_internal::sb_bloom_offsets_grid(file_cap >> LV_SST_FILTER_BASE_LG));
        hipLaunchKernelGGL(lvk::sb_bloom_emit, dim3(wg), b, 0, s, A);
        hipLaunchKernelGGL(lvk::sb_bloom_big, dim3(wg), b, 0, s, A);
        hipLaunchKernelGGL(lvk::sb_bloom_offsets, dim3(og), b, 0, s, A);
    }
    const uint32_t hg = static_cast<uint32_t>((static_cast<uint64_t>(block_cap) + 1 + nbuf + lvk::kSbThreads - 1) / lvk::kSbThreads);
    hipLaunchKernelGGL(lvk::sb_tail, dim3(hg), b, 0, s, A);
    if (int rc = check_launch()) return rc;
    if (tiles && file_cap) {
        // the trailers: the seal's own kernel over the padded handles (data blocks and metaindex) ...
        if (int rc = lvgpu_internal::launch_sst_blocks(true, d_file, file_cap, A.wsh, nullptr,
                                                       static_cast<size_t>(block_cap) + 1 + nbuf, nullptr, nullptr, stream))
            return rc;
        // ... and the index block (with a filter policy, the filter block too) as a batch of the
        // offsets API (an empty one when nothing was written)
        if (int rc = lv_crc32c_batch_device_ws(d_file, A.idx_off, A.idx_len, nullptr, A.idx_crc, nbuf, LV_CRC_MASK,
                                               crc_ws, lv_crc32c_workspace_bytes(nbuf), stream))
            return rc;
        hipLaunchKernelGGL(lvk::sb_index_trailer, dim3(1), dim3(1), 0, s, A);
        if (int rc = check_launch()) return rc;
    }
    g_kernel = bloom ? "sb_init+sb_sizes+sb_carry+sb_next+sb_reach+sb_layout+sb_index+sb_bloom_sizes+sb_plan+sb_emit+"
                       "sb_bloom_emit+sb_bloom_big+sb_bloom_offsets+sb_tail+sst_blocks_kernel<seal>+"
                       "crc32c_fused_small_kernel+sb_index_trailer"
                     : "sb_init+sb_sizes+sb_carry+sb_next+sb_reach+sb_layout+sb_index+sb_plan+sb_emit+sb_tail+"
                       "sst_blocks_kernel<seal>+crc32c_fused_small_kernel+sb_index_trailer";
    return LV_OK;
}

}  // namespace
