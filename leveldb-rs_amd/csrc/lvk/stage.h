// Device primitives shared by the pipeline stages (lvk/stage.h): WriteBatch
// decode (write_batch.hip) and encode (write_batch_encode.hip), memtable build
// and get (memtable.hip) and range reads (memtable_range.hip), SSTable
// build (sst_build.hip), get (sst_get.hip) and scan (sst_scan.hip), the
// compaction filter (compact.hip), VersionEdit decode and encode
// (version_edit.hip), the version builder (version_set.hip).
//
// The stages hand each other an op table (32-byte lv_wb_op entries over a
// payload or an arena) and are built from the same few parts: an extent check
// on what an op points at, the op as two 16-B accesses, user keys compared as
// bytes, a u64 shuffle and the wave's sum, least and greatest, a varint's
// length and store, the record of a row by its bounds, a two-level scan
// (tile-local in LDS, then one wave over the tiles' sums) and a copy of long
// byte strings that the lanes of a wave share.  Each part is here once; the
// tile sizes, thread counts and copy knobs stay with the stage that owns them
// and come in as template arguments.  What only the two record decoders share
// (byte sources, varint reads, the wave's dispatch) is lvk/records.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../../include/lvgpu/write_batch.h"
#include "core.h"

namespace lvk {

// [off, off + len) lies inside [0, bytes).  All u64: nothing wraps.
__device__ __forceinline__ bool extent_ok(uint64_t off, uint64_t len, uint64_t bytes) {
    return off <= bytes && len <= bytes - off;
}

// An op as two 16-B loads / stores.  p must be 16-B aligned: an op table is
// (every entry point checks d_ops), and an op is 32 bytes, so each entry is.
__device__ __forceinline__ lv_wb_op load_op(const lv_wb_op *p) {
    const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
    const u32x4 a = q[0], b = q[1];
    lv_wb_op o;
    o.tag = (static_cast<uint64_t>(a.y) << 32) | a.x;
    o.key_off = (static_cast<uint64_t>(a.w) << 32) | a.z;
    o.val_off = (static_cast<uint64_t>(b.y) << 32) | b.x;
    o.key_len = b.z;
    o.val_len = b.w;
    return o;
}

__device__ __forceinline__ void store_op(lv_wb_op *p, const lv_wb_op &o) {
    u32x4 *q = reinterpret_cast<u32x4 *>(p);
    q[0] = u32x4{static_cast<uint32_t>(o.tag), static_cast<uint32_t>(o.tag >> 32), static_cast<uint32_t>(o.key_off),
                 static_cast<uint32_t>(o.key_off >> 32)};
    q[1] = u32x4{static_cast<uint32_t>(o.val_off), static_cast<uint32_t>(o.val_off >> 32), o.key_len, o.val_len};
}

// 8 bytes at any alignment as a big-endian word: all of them are key bytes.
__device__ __forceinline__ uint64_t load_be64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return __builtin_bswap64(v);
}

// BytewiseComparator over a[0, alen) and b[0, blen): -1 / 0 / +1.  Whole
// 8-byte words while both have them, then bytes: nothing outside is read.
__device__ __forceinline__ int cmp_bytes(const uint8_t *a, uint64_t alen, const uint8_t *b, uint64_t blen) {
    const uint64_t m = alen < blen ? alen : blen;
    uint64_t i = 0;
    for (; i + 8 <= m; i += 8) {
        const uint64_t x = load_be64(a + i), y = load_be64(b + i);
        if (x != y) return x < y ? -1 : 1;
    }
    for (; i < m; ++i) {
        const uint32_t x = a[i], y = b[i];
        if (x != y) return x < y ? -1 : 1;
    }
    return alen < blen ? -1 : alen > blen ? 1 : 0;
}

// a[0, alen) and b[0, blen) are the same bytes: the lengths first, then whole
// 8-byte words at any alignment, then the rest.  Nothing outside is read.
__device__ __forceinline__ bool same_bytes(const uint8_t *a, uint64_t alen, const uint8_t *b, uint64_t blen) {
    if (alen != blen) return false;
    uint64_t i = 0;
    for (; i + 8 <= alen; i += 8) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + i, 8);
        __builtin_memcpy(&y, b + i, 8);
        if (x != y) return false;
    }
    for (; i < alen; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

// Inclusive scan of v over the 64 lanes of a wave.  Every lane of the wave
// calls it (the shuffles read inactive lanes' registers otherwise).
__device__ __forceinline__ uint64_t wave_incl(uint64_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint64_t u = __shfl_up(static_cast<unsigned long long>(v), o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// Lane src's v, and v summed / its least / its greatest over the 64 lanes of a
// wave, in every lane.  Every lane of the wave calls them, as above.
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src) {
    return __shfl(static_cast<unsigned long long>(v), static_cast<int>(src), 64);
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(static_cast<unsigned long long>(v), static_cast<int>(d), 64);
    return v;
}
__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        const uint64_t o = __shfl_xor(static_cast<unsigned long long>(v), static_cast<int>(d), 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        const uint64_t o = __shfl_xor(static_cast<unsigned long long>(v), static_cast<int>(d), 64);
        v = o > v ? o : v;
    }
    return v;
}

// A varint's length, and its bytes stored at p: returns the byte behind them.
__device__ __forceinline__ uint32_t varint_len(uint64_t v) {
    uint32_t n = 1;
    while (v >= 128) {
        v >>= 7;
        ++n;
    }
    return n;
}
__device__ __forceinline__ uint8_t *put_varint(uint8_t *p, uint64_t v) {
    while (v >= 128) {
        *p++ = static_cast<uint8_t>(v | 0x80);
        v >>= 7;
    }
    *p++ = static_cast<uint8_t>(v);
    return p;
}

// The record of row i of an ascending bounds array: the r with
// bounds[r] <= i < bounds[r + 1], searched in [lo, hi] (it lies there).
// Empty records make equal bounds: the last of them whose bound is <= i is
// the one.  Bounded by the 32 bits of a record index.
__device__ __forceinline__ uint64_t record_of(const uint64_t *bounds, uint64_t i, uint64_t lo, uint64_t hi) {
    for (uint32_t it = 0; it < 33 && lo < hi; ++it) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;  // in (lo, hi]
        if (bounds[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// In-place inclusive scan of the LDS array s[0, kTile) with stride st: the
// chains s[j] += s[j - st] (st = 1: the plain scan; st = R: one scan per
// residue of R).  A workgroup of kThreads threads, thread tid; it contains
// __syncthreads(), so every thread of the workgroup calls it, with s complete
// (a barrier after the last store to s, or a __syncthreads_or that served as
// one).  1 <= st; kTile is a multiple of kThreads.
template <uint32_t kTile, uint32_t kThreads>
__device__ __forceinline__ void tile_scan(uint64_t *s, uint32_t st, uint32_t tid) {
    static_assert(kTile % kThreads == 0, "a tile is whole rounds of a workgroup");
    constexpr uint32_t kPer = kTile / kThreads;
    for (uint32_t off = st; off < kTile; off <<= 1) {
        uint64_t v[kPer];
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t j = tid + k * kThreads;
            v[k] = j >= off ? s[j - off] : 0;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) s[tid + k * kThreads] += v[k];
        __syncthreads();
    }
}

// The second level of a scan: the tiles' sums col[t * stride], t < tiles,
// become their exclusive scan, in place; returns their sum.  One wave, all 64
// lanes, owns the column (tiles and stride are wave-uniform); nobody else
// touches it during the launch.
__device__ __forceinline__ uint64_t carry_scan(uint64_t *col, uint64_t stride, uint64_t tiles, uint32_t lane) {
    uint64_t run = 0;
    for (uint64_t t0 = 0; t0 < tiles; t0 += 64) {  // wave-uniform
        const uint64_t t = t0 + lane;
        const uint64_t v = t < tiles ? col[t * stride] : 0;
        const uint64_t inc = wave_incl(v, lane);
        if (t < tiles) col[t * stride] = run + inc - v;
        run += __shfl(static_cast<unsigned long long>(inc), 63, 64);
    }
    return run;
}

// len bytes from src to dst by kLanes lanes (lane < kLanes; kLanes divides
// 64): dst's ragged head and tail byte by byte, between them 16-byte granules
// of dst's alignment (an unaligned load, an aligned store).  len >= 16.
template <uint32_t kLanes>
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, uint64_t len, uint32_t lane) {
    static_assert(kLanes >= 1 && 64 % kLanes == 0, "a wave is whole groups of copy lanes");
    const uint32_t head = static_cast<uint32_t>((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
    const uint64_t gran = (len - head) / 16;
    const uint32_t tail = static_cast<uint32_t>((len - head) % 16);
    for (uint32_t i = lane; i < head; i += kLanes) dst[i] = src[i];
    for (uint64_t g = lane; g < gran; g += kLanes) {
        u32x4 v;
        __builtin_memcpy(&v, src + head + g * 16, 16);
        *reinterpret_cast<u32x4 *>(dst + head + g * 16) = v;
    }
    for (uint32_t i = lane; i < tail; i += kLanes) dst[head + gran * 16 + i] = src[head + gran * 16 + i];
}

// A lane's copy job (len may be 0; dst and src are then not read): one
// shorter than kWaveCopy the lane does itself, the others its wave does, a
// group of kLanes lanes per job and 64 / kLanes jobs at a time.  Every lane
// of the wave calls it, lane = its index in the wave.  kWaveCopy >= 16.
template <uint32_t kLanes, uint32_t kWaveCopy>
__device__ __forceinline__ void group_copy(uint8_t *dst, const uint8_t *src, uint64_t len, uint32_t lane) {
    static_assert(kWaveCopy >= 16, "a wave copy has at least one granule");
    constexpr uint32_t kGroups = 64 / kLanes;
    if (len < kWaveCopy)
        for (uint64_t i = 0; i < len; ++i) dst[i] = src[i];
    uint64_t todo = __ballot(len >= kWaveCopy);
    const uint32_t grp = lane / kLanes;
    while (todo) {  // wave-uniform
        int l = -1;  // this group's job: the grp-th lane of todo, if there is one
        uint64_t t = todo;
#pragma unroll
        for (uint32_t k = 0; k < kGroups; ++k) {
            if (k <= grp) l = t ? __ffsll(static_cast<unsigned long long>(t)) - 1 : -1;
            t &= t - 1;  // (0 stays 0)
        }
        todo = t;
        const int from = l < 0 ? 0 : l;
        uint8_t *d = reinterpret_cast<uint8_t *>(__shfl(reinterpret_cast<unsigned long long>(dst), from, 64));
        const uint8_t *sp = reinterpret_cast<const uint8_t *>(__shfl(reinterpret_cast<unsigned long long>(src), from, 64));
        const uint64_t m = __shfl(static_cast<unsigned long long>(len), from, 64);
        if (l >= 0) wave_copy<kLanes>(d, sp, m, lane % kLanes);
    }
}

}  // namespace lvk
