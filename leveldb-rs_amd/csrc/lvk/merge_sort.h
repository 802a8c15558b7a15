// The comparison sort shared by the memtable build (memtable.hip) and the
// version builder (version_set.hip): a bitonic network over one tile in LDS,
// and merge passes in which a workgroup owns one output tile and finds its
// share of the two input runs by merge path.  The entry type and the strict
// total order come in as template arguments: an entry is a whole number of
// 16-byte quads, `less(a, b)` orders two of them (padding entries last), and
// the tile size and thread count stay with the stage that owns them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "core.h"

namespace lvk {

// s[0, m) sorted in place, m a power of two >= 2 (the caller filled the slots
// behind its entries with padding).  Contains barriers: every thread of the
// workgroup calls it, behind a barrier after the last store to s.
template <uint32_t kThreads, class Ent, class Less>
__device__ __forceinline__ void lds_bitonic_sort(Ent *s, uint32_t m, uint32_t tid, const Less &less) {
    for (uint32_t k = 2; k <= m; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < m / 2; t += kThreads) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const bool up = (i & k) == 0;
                const Ent a = s[i], b = s[l];
                if (less(b, a) == up) {
                    s[i] = b;
                    s[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

// The merge path of diagonal d over the sorted runs a[0, la) and b[0, lb):
// how many of the first d outputs come from a.  At most 33 steps (la < 2^32).
template <class Ent, class Less>
__device__ __forceinline__ uint64_t merge_path(const Less &less, const Ent *a, uint64_t la, const Ent *b, uint64_t lb,
                                               uint64_t d) {
    uint64_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    for (uint32_t it = 0; it < 64 && lo < hi; ++it) {
        const uint64_t mid = lo + (hi - lo) / 2;  // lo <= mid < hi: mid < la and d - 1 - mid < lb
        if (less(b[d - 1 - mid], a[mid]))
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// One output tile of one merge pass: the runs of w entries of in[0, n) merged
// in pairs into out, of which this workgroup writes [o0, o0 + kTile) (o0 < n,
// w < n).  Two threads find the tile's merge-path diagonals by binary search,
// the inputs are staged in s (kTile entries of LDS), every thread merges
// kTile / kThreads outputs and the tile leaves in coalesced stores.
template <uint32_t kTile, uint32_t kThreads, class Ent, class Less>
__device__ __forceinline__ void merge_tile(const Less &less, const Ent *in, Ent *out, uint64_t n, uint64_t w,
                                           uint64_t o0, Ent *s, uint64_t *s_split, uint32_t tid) {
    static_assert(kTile % kThreads == 0 && sizeof(Ent) % 16 == 0, "a thread's share is whole, an entry whole quads");
    constexpr uint32_t kPer = kTile / kThreads;
    const uint64_t start = o0 / (2 * w) * (2 * w);
    const uint64_t mid = start + w < n ? start + w : n, end = start + 2 * w < n ? start + 2 * w : n;
    const uint64_t la = mid - start, lb = end - mid;
    const Ent *ra = in + start, *rb = in + mid;
    const uint64_t d0 = o0 - start, d1 = d0 + kTile < la + lb ? d0 + kTile : la + lb;
    if (tid < 2) s_split[tid] = merge_path(less, ra, la, rb, lb, tid ? d1 : d0);
    __syncthreads();
    const uint64_t a0 = s_split[0], a1 = s_split[1], b0 = d0 - a0;
    const uint32_t na = static_cast<uint32_t>(a1 - a0), total = static_cast<uint32_t>(d1 - d0), nb = total - na;
    for (uint32_t j = tid; j < total; j += kThreads) s[j] = j < na ? ra[a0 + j] : rb[b0 + (j - na)];
    __syncthreads();
    // this thread's outputs [q0, q1) of the tile: its own diagonal, then a serial merge
    const uint32_t q0 = tid * kPer < total ? tid * kPer : total;
    const uint32_t q1 = q0 + kPer < total ? q0 + kPer : total;
    uint32_t x = static_cast<uint32_t>(merge_path(less, s, na, s + na, nb, q0)), y = q0 - x;
    constexpr uint32_t kQ = sizeof(Ent) / 16;  // an entry as 16-B register quads
    u32x4 r[kPer][kQ];
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        uint32_t from = 0;
        if (q0 + k < q1) {
            const bool take_a = y >= nb || (x < na && !less(s[na + y], s[x]));
            from = take_a ? x : na + y;
            x += take_a;
            y += !take_a;
        }
#pragma unroll
        for (uint32_t v = 0; v < kQ; ++v) r[k][v] = reinterpret_cast<const u32x4 *>(s + from)[v];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k)
        if (q0 + k < q1) {
#pragma unroll
            for (uint32_t v = 0; v < kQ; ++v) reinterpret_cast<u32x4 *>(s + q0 + k)[v] = r[k][v];
        }
    __syncthreads();
    for (uint32_t j = tid; j < total; j += kThreads) out[o0 + j] = s[j];
}

}  // namespace lvk
