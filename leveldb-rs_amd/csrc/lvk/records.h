// Device parts shared by the record decoders (lvk/records.h): WriteBatch
// decode (write_batch.hip) and VersionEdit decode (version_edit.hip).
//
// Both formats are sequential inside a record and independent across records,
// and both stages walk a record through a byte source: a record of up to
// kSmall bytes by one lane over the aligned 16-byte granule under the byte it
// needs (LaneSrc), a longer one by its wave through an LDS window, wave-
// uniformly (WaveSrc).  A wave takes 64 consecutive records at a time
// (dispatch): each lane walks its own if it is small, then the wave walks the
// large ones among them one after another.  The sizes (kSmall, the window and
// its round) stay with the stage that owns them and come in as template
// arguments; what a walk does with what it parses, and its status codes, stay
// with the stage too.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "stage.h"

namespace lvk {

// Records to walk: none when upstream wrote no arrays or the arrays are too
// short for what it counted.
__device__ __forceinline__ uint64_t records_to_walk(const uint64_t *records, const uint64_t *upstream, uint64_t rec_cap) {
    if (upstream && *upstream) return 0;
    const uint64_t n = *records;
    return n > rec_cap ? 0ull : n;
}

// ---- byte sources ---------------------------------------------------------
// One lane: the aligned granule under the last byte asked for, in registers.
struct LaneSrc {
    const uint8_t *p;
    uint64_t gi;
    u32x4 g;
    __device__ __forceinline__ explicit LaneSrc(const uint8_t *payload) : p(payload), gi(~0ull), g{0, 0, 0, 0} {}
    __device__ __forceinline__ uint32_t byte(uint64_t a) {
        const uint64_t addr = reinterpret_cast<uint64_t>(p) + a;
        const uint64_t q = addr >> 4;
        if (q != gi) {
            g = *reinterpret_cast<const u32x4 *>(q << 4);
            gi = q;
        }
        const uint32_t i = static_cast<uint32_t>(addr) & 15u;
        const uint32_t w = i < 8 ? (i < 4 ? g.x : g.y) : (i < 12 ? g.z : g.w);
        return (w >> (8 * (i & 3u))) & 0xffu;
    }
};

// LDS behind a window: the register refill reads three aligned words from the
// word under a window byte, so the last 12 bytes read may begin at the
// window's last word and run into the pad.  Nothing else is read past the
// window, and of those words only the rn bytes inside the loaded part of the
// window are ever used.  A wave's window is `uint8_t[kWindow + kWinPad]`,
// 16-byte aligned.
constexpr uint32_t kWinPad = 16;

// One wave: a window of kWindow bytes in LDS, from an aligned address.  A
// window opens where the parser lands after a skip, with its first round
// (kRound bytes: an entry's header after a long value is all that is wanted
// of it); when the walk runs on past that round, the rest of the window is
// loaded at once.  A window is reused while the byte asked for lies inside
// it, backwards too; otherwise the next one starts at that byte's granule, so
// what lies between is skipped, not read.  Only granules that begin before
// the record's end are loaded (the rest read as 0 and are never asked for),
// so nothing is read past the granule that holds the record's last byte.
// Every call is wave-uniform.
template <uint32_t kWindow, uint32_t kRound>
struct WaveSrc {
    static_assert(kRound % 16 == 0, "a round is whole granules");
    static_assert(kWindow % kRound == 0 && kWindow > kRound, "a window is whole rounds, more than one");
    const uint8_t *p;
    uint8_t *lds;
    uint64_t lo, end;  // window start address (16-B aligned; ~0: none), record end address
    uint32_t have;     // bytes of the window that are loaded
    uint32_t lane;
    // the rn (<= 8) bytes from address ra on, in a register pair: an entry's
    // header is parsed from it, so the LDS round trip is paid once per header,
    // not once per byte
    uint64_t ra, rw;
    uint32_t rn;
    __device__ __forceinline__ WaveSrc(const uint8_t *payload, uint8_t *window, uint64_t rec_end, uint32_t l)
        : p(payload), lds(window), lo(~0ull), end(reinterpret_cast<uint64_t>(payload) + rec_end), have(0), lane(l),
          ra(0), rw(0), rn(0) {}
    __device__ __forceinline__ void load(uint32_t from, uint32_t to) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the reads of the old window are done
        for (uint32_t slot = from / 16 + lane; slot < to / 16; slot += 64) {
            const uint64_t ga = lo + static_cast<uint64_t>(slot) * 16;
            u32x4 v{0, 0, 0, 0};
            if (ga < end) v = *reinterpret_cast<const u32x4 *>(ga);
            reinterpret_cast<u32x4 *>(lds)[slot] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the stores of the new one are
    }
    __device__ __forceinline__ void refill(uint64_t addr) {
        if (lo == ~0ull || addr < lo || addr - lo >= kWindow) {
            lo = addr & ~15ull;
            have = 0;
        }
        const uint32_t at = static_cast<uint32_t>(addr - lo);
        if (at >= have) {  // a new window: its first round; running on: the rest
            const uint32_t to = have ? kWindow : kRound;
            load(have, to);
            have = to;
        }
        // 8 bytes from `at`: three aligned words and a byte shift (kWinPad)
        const uint32_t *w = reinterpret_cast<const uint32_t *>(lds + (at & ~3u));
        const uint32_t d0 = w[0], d1 = w[1], d2 = w[2], s = at & 3u;
        const uint32_t l32 = __builtin_amdgcn_alignbyte(d1, d0, s), h32 = __builtin_amdgcn_alignbyte(d2, d1, s);
        rw = (static_cast<uint64_t>(h32) << 32) | l32;
        ra = addr;
        rn = have - at < 8u ? have - at : 8u;
    }
    __device__ __forceinline__ uint32_t byte(uint64_t a) {
        const uint64_t addr = reinterpret_cast<uint64_t>(p) + a;
        uint64_t d = addr - ra;
        if (d >= rn) {
            refill(addr);
            d = 0;
        }
        return static_cast<uint32_t>(rw >> (8u * static_cast<uint32_t>(d))) & 0xffu;
    }
};

// ---- varints through a source ----------------------------------------------
// coding.rs:186-204 over the record's remaining input [*pos, n) of the record
// at payload offset off: true with *v and *pos past the varint; false (a
// fifth byte with its top bit set, or the input ends) with neither written.
template <class Src>
__device__ __forceinline__ bool varint32(Src &src, uint64_t off, uint64_t n, uint64_t *pos, uint32_t *v) {
    uint32_t result = 0;
    uint64_t p = *pos;
    for (uint32_t shift = 0; shift <= 28 && p < n; shift += 7) {
        const uint32_t b = src.byte(off + p);
        ++p;
        result |= (b & 0x7fu) << shift;  // bits above 31 of the fifth byte fall off
        if (!(b & 0x80u)) {
            *pos = p;
            *v = result;
            return true;
        }
    }
    return false;
}

// coding.rs:223-241, the same over ten bytes.
template <class Src>
__device__ __forceinline__ bool varint64(Src &src, uint64_t off, uint64_t n, uint64_t *pos, uint64_t *v) {
    uint64_t result = 0;
    uint64_t p = *pos;
    for (uint32_t shift = 0; shift <= 63 && p < n; shift += 7) {
        const uint64_t b = src.byte(off + p);
        ++p;
        result |= (b & 0x7fu) << shift;  // bits above 63 of the tenth byte fall off
        if (!(b & 0x80u)) {
            *pos = p;
            *v = result;
            return true;
        }
    }
    return false;
}

// ---- a wave's 64 records -----------------------------------------------------
// What record_class says of a record.  A stage reports kRecOutOfRange with its
// own status code; there is as little to walk as for kRecNone.
enum : uint32_t { kRecNone = 0, kRecLane = 1, kRecWave = 2, kRecOutOfRange = 3 };

// Record r's extent and class: kRecNone beyond the n records, kRecOutOfRange
// when the extent leaves the payload (*off = *len = 0 in both), else the
// extent and kRecLane (up to kSmall bytes) or kRecWave.
template <uint32_t kSmall>
__device__ __forceinline__ uint32_t record_class(const uint64_t *rec_off, const uint64_t *rec_len, uint64_t payload_bytes,
                                                 uint64_t r, uint64_t n, uint64_t *off, uint64_t *len) {
    *off = 0;
    *len = 0;
    if (r >= n) return kRecNone;
    const uint64_t o = rec_off[r], l = rec_len[r];
    // !extent_ok(o, l, payload_bytes), spelled out: through the helper the compares come out inverted
    // and the walks behind them move by 24 bytes, which measured 1-2 % slower on long records
    if (o > payload_bytes || l > payload_bytes - o) return kRecOutOfRange;  // u64, no wrap
    *off = o;
    *len = l;
    return l <= kSmall ? kRecLane : kRecWave;
}

// The walks of a wave's 64 records, lane i holding the class and the extent
// of record i: own() in every lane whose record is kRecLane, then
// wave(b, off, len), once for each lane b whose record is kRecWave, in lane
// order, with lane b's extent in every lane.  Every lane of the wave enters,
// whatever its class (the ballot and the shuffles are the whole wave's), and
// the loop is wave-uniform, so wave() may build a WaveSrc and walk wave-
// uniformly.  What else of lane b the walk needs (its output bases) wave()
// takes with shfl64(.., b); the walk's result is the same in every lane, and
// lane b is the one to keep it.
template <class Own, class Wave>
__device__ __forceinline__ void dispatch(uint32_t cls, uint64_t off, uint64_t len, Own &&own, Wave &&wave) {
    if (cls == kRecLane) own();
    uint64_t m = __ballot(cls == kRecWave);
    while (m) {  // wave-uniform
        const uint32_t b = static_cast<uint32_t>(__builtin_ctzll(m));
        m &= m - 1;
        wave(b, shfl64(off, b), shfl64(len, b));
    }
}

}  // namespace lvk
