// The log format on the device and the parts wal_frame_kernel
// (wal_encode.hip) and wal_unframe_kernel (wal_decode.hip) share (lvk/wal.h).
// The two kernels mirror each other: a workgroup takes one 32 KiB block, puts
// its fragments' positions in LDS as 16-bit offsets, and follows the output in
// 16-byte granules of the output's alignment; a lane finds the fragment under
// its granule with a search in LDS.  A granule wholly inside one fragment is
// one unaligned 16-B load and one aligned 16-B store, in the kernel itself;
// any other granule is composed byte by byte into two halves and stored here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../../include/lvgpu/wal.h"
#include "core.h"

namespace lvk {

constexpr uint32_t kWalBlock = LV_WAL_BLOCK_SIZE;             // log_format.rs:63
constexpr uint32_t kWalHeader = LV_WAL_HEADER_SIZE;           // log_format.rs:66
constexpr uint32_t kWalMaxFrags = kWalBlock / kWalHeader + 1;  // headers that fit one block
static_assert(kWalBlock == 32768 && kWalHeader == 7, "the log format (in-block positions are 16-bit)");

// How many of the ascending s[0, n) (LDS) are <= x: the last fragment at or
// before x is the one before that index.
__device__ __forceinline__ uint32_t count_le(const uint16_t *s, uint32_t n, uint32_t x) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t m = (a + b) >> 1;
        if (s[m] <= x)
            a = m + 1;
        else
            b = m;
    }
    return a;
}

// A granule composed byte by byte is held as two halves, byte k < 8 in lo and
// the others in hi (the kernels pack them themselves: through a helper
// frame_compose's 16 steps were no longer unrolled).  Its bytes k with bit k
// of `valid` set go to q[k]: one 16-B store when all 16 are (q is then 16-B
// aligned), else byte by byte, so that bytes another workgroup owns, or that
// lie outside the output, are never stored.
__device__ __forceinline__ void granule_store(uint8_t *q, uint64_t lo, uint64_t hi, uint32_t valid) {
    if (valid == 0xffffu) {
        u32x4 v;
        v.x = static_cast<uint32_t>(lo);
        v.y = static_cast<uint32_t>(lo >> 32);
        v.z = static_cast<uint32_t>(hi);
        v.w = static_cast<uint32_t>(hi >> 32);
        *reinterpret_cast<u32x4 *>(q) = v;
    } else {
        for (uint32_t k = 0; k < 16; ++k)
            if (valid & (1u << k)) q[k] = static_cast<uint8_t>((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xffu);
    }
}

// The checksum a header at h stores (LE32, log_writer.rs:117-125), unmasked
// (crc32c.rs:59-63).
__device__ __forceinline__ uint32_t stored_crc(const uint8_t *h) {
    const uint32_t stored = h[0] | (static_cast<uint32_t>(h[1]) << 8) | (static_cast<uint32_t>(h[2]) << 16) |
                            (static_cast<uint32_t>(h[3]) << 24);
    const uint32_t rot = stored - 0xa282ead8u;
    return (rot >> 17) | (rot << 15);
}

}  // namespace lvk
