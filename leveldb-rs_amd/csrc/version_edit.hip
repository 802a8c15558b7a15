// lv_version_edit_decode_device / lv_version_edit_encode_device /
// lv_version_edit_files_device (include/lvgpu/version_edit.h;
// csrc/version_edit.cc holds the serial twins): VersionEdit::decode_from and
// encode_to (version_edit.rs:192-319) for a batch of MANIFEST records in HBM.
//
// Decode is write_batch.hip's shape, the format being sequential inside a
// record and independent across records:
//
//   vd_init    (one thread) zeroes the call's head in the workspace.
//   vd_count   a workgroup per tile of kVdTile records: every record is walked
//              once -- its edit (to the workspace), its three row counts and
//              its status; the tile's three sums, its first bad record and the
//              last record before that carrying each has bit.
//   vd_tiles   (one wave) lvk::carry_scan over the tiles' three columns, the
//              first bad record and last_has over the tiles, the totals and
//              the status.
//   vd_emit    lvk::tile_scan of the tile's counts (three columns, stride 3)
//              gives each record's three bases; the edit is copied out and the
//              records with rows are walked again.
//
// Count and emit share one walk (vd_walk), templated on the byte source and
// the row sink.  The byte sources, the varint reads, a record's class and the
// wave's dispatch are the ones write_batch.hip uses, lvk/records.h's: a
// record of up to kVdSmall bytes is walked by one lane over the aligned
// 16-byte granule under the byte it needs (LaneSrc); a longer one by its wave
// through an LDS window (WaveSrc), wave-uniformly, and lane k % 64 stores
// row k.
//
// Encode is write_batch_encode.hip's shape, all or nothing: validate the
// bounds; size every item (a record's scalar group or one row) with a tile
// scan; carry; emit.  The item order is the four tables one after another
// (edits, pointers, deleted, files), each with cap + 1 slots rounded up to
// whole tiles, so a tile holds one kind and slot `cap` exists: the bytes of
// kind k before row i are one lookup (ve_before) whatever i <= cap is, and a
// record's place is its scalar groups' prefix plus three differences of those.
//
// Every grid is sized by the capacities, one workgroup per tile, no
// grid-stride loop; the only loops whose trip count grows with the input are
// the carries' rounds of 64 tiles.  All positions are u64.  The wave
// reductions, the varint's length and store and the record of a row
// (record_of) are lvk/stage.h's.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/version_edit.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/records.h"

namespace lvk {

// ============================ decode ========================================
constexpr uint32_t kVdThreads = 256;
constexpr uint32_t kVdTile = kVdThreads;              // records per tile: one per thread, 64 per wave
constexpr uint32_t kVdWaves = kVdThreads / 64;
constexpr uint32_t kVdSmall = 16384;                  // records up to this many bytes: one lane each
constexpr uint32_t kVdWindow = 4096;                  // LDS window of a wave-class record, bytes
constexpr uint32_t kVdRound = 64 * 16;                // one load of the wave: 64 lanes x 16 B

struct VdHead {  // workspace, zeroed by vd_init
    unsigned long long bad;
    uint64_t n, status, pad;
};

struct VdArgs {
    const uint8_t *payload;
    uint64_t payload_bytes;
    const uint64_t *rec_off, *rec_len, *records, *upstream;
    uint64_t rec_cap;
    lv_ve_decode_out out;
    // workspace
    VdHead *head;
    lv_ve_edit *edits;  // [rec_cap] the count walk's edits
    uint64_t *cnt;      // [3 rec_cap] file, deleted and pointer rows of each record
    uint64_t *tsum;     // [3 tiles] the tiles' rows, then (vd_tiles) the rows before the tile
    uint64_t *tinfo;    // [6 tiles] the tile's first bad record (~0: none), 1 + the last record before it with each has bit
};

// ---- row sinks -----------------------------------------------------------------
struct VdNoSink {
    __device__ __forceinline__ void file(uint64_t, const lv_ve_file &) {}
    __device__ __forceinline__ void deleted(uint64_t, const lv_ve_deleted &) {}
    __device__ __forceinline__ void pointer(uint64_t, const lv_ve_pointer &) {}
};

// Row k of the record goes to its table at base + k.  A lane on its own stores
// every row (mask 0, lane 0); in a wave's uniform walk lane k % 64 does
// (mask 63).  The capacity checks never fail: the status said the rows fit.
struct VdSink {
    lv_ve_decode_out o;
    uint64_t bf, bd, bp;
    uint32_t lane, mask;
    __device__ __forceinline__ bool mine(uint64_t k) const { return (static_cast<uint32_t>(k) & mask) == lane; }
    __device__ __forceinline__ void file(uint64_t k, const lv_ve_file &f) {
        if (mine(k) && bf + k < o.file_cap) o.d_files[bf + k] = f;
    }
    __device__ __forceinline__ void deleted(uint64_t k, const lv_ve_deleted &d) {
        if (mine(k) && bd + k < o.deleted_cap) o.d_deleted[bd + k] = d;
    }
    __device__ __forceinline__ void pointer(uint64_t k, const lv_ve_pointer &q) {
        if (mine(k) && bp + k < o.pointer_cap) o.d_pointers[bp + k] = q;
    }
};

// ---- the walk ------------------------------------------------------------------
struct VdRes {
    lv_ve_edit e;
    uint64_t nf, nd, np;
};

// coding.rs:294-305; the body is skipped, not read.  *at = its offset in the payload.
template <class Src>
__device__ __forceinline__ uint32_t vd_varstring(Src &src, uint64_t off, uint64_t n, uint64_t *pos, uint64_t *at,
                                                 uint32_t *len) {
    uint32_t l;
    if (!varint32(src, off, n, pos, &l)) return LV_VE_BAD_VARINT32;
    if (n - *pos < l) return LV_VE_BAD_LENGTH;
    *at = off + *pos;
    *len = l;
    *pos += l;
    return LV_VE_OK;
}

// get_level (version_edit.rs:361-369): the comparison is the i32's.
template <class Src>
__device__ __forceinline__ uint32_t vd_level(Src &src, uint64_t off, uint64_t n, uint64_t *pos, uint32_t *level,
                                             uint32_t *flags) {
    if (!varint32(src, off, n, pos, level)) return LV_VE_BAD_VARINT32;
    if (*level & 0x80000000u)
        *flags |= LV_VE_FLAG_NEG_LEVEL;
    else if (*level >= LV_VE_NUM_LEVELS)
        return LV_VE_BAD_LEVEL;
    return LV_VE_OK;
}

// VersionEdit::decode_from over d_payload[off, off + n), the extent already
// known to lie inside the payload.  Reads only bytes of the record (through src).
template <class Src, class Sink>
__device__ __forceinline__ VdRes vd_walk(Src &src, Sink &sink, uint64_t off, uint64_t n) {
    VdRes r{};
    lv_ve_edit &e = r.e;
    uint64_t pos = 0;
    uint32_t st = LV_VE_OK;
    while (st == LV_VE_OK) {
        uint32_t tag;
        if (!varint32(src, off, n, &pos, &tag)) {
            if (pos < n) st = LV_VE_INVALID_TAG;
            break;
        }
        tag &= 0xffu;
        if (tag == 1) {
            if ((st = vd_varstring(src, off, n, &pos, &e.comparator_off, &e.comparator_len)) == LV_VE_OK)
                e.has |= LV_VE_HAS_COMPARATOR;
        } else if (tag == 2 || tag == 3 || tag == 4 || tag == 9) {
            uint64_t v;
            if (!varint64(src, off, n, &pos, &v)) {
                st = LV_VE_BAD_VARINT64;
            } else if (tag == 2) {
                e.log_number = v;
                e.has |= LV_VE_HAS_LOG_NUMBER;
            } else if (tag == 9) {
                e.prev_log_number = v;
                e.has |= LV_VE_HAS_PREV_LOG_NUMBER;
            } else if (tag == 3) {
                e.next_file_number = v;
                e.has |= LV_VE_HAS_NEXT_FILE;
            } else {
                e.last_sequence = v;
                e.has |= LV_VE_HAS_LAST_SEQUENCE;
            }
        } else if (tag == 5) {
            lv_ve_pointer q{};
            if ((st = vd_level(src, off, n, &pos, &q.level, &e.flags)) != LV_VE_OK) break;
            if ((st = vd_varstring(src, off, n, &pos, &q.key_off, &q.key_len)) != LV_VE_OK) break;
            if (q.key_len < 8) e.flags |= LV_VE_FLAG_SHORT_KEY;
            sink.pointer(r.np, q);
            ++r.np;
        } else if (tag == 6) {
            lv_ve_deleted d{};
            if ((st = vd_level(src, off, n, &pos, &d.level, &e.flags)) != LV_VE_OK) break;
            if (!varint64(src, off, n, &pos, &d.number)) {
                st = LV_VE_BAD_VARINT64;
                break;
            }
            sink.deleted(r.nd, d);
            ++r.nd;
        } else if (tag == 7) {
            lv_ve_file f{};
            if ((st = vd_level(src, off, n, &pos, &f.level, &e.flags)) != LV_VE_OK) break;
            if (!varint64(src, off, n, &pos, &f.number) || !varint64(src, off, n, &pos, &f.file_size)) {
                st = LV_VE_BAD_VARINT64;
                break;
            }
            if ((st = vd_varstring(src, off, n, &pos, &f.smallest_off, &f.smallest_len)) != LV_VE_OK) break;
            if ((st = vd_varstring(src, off, n, &pos, &f.largest_off, &f.largest_len)) != LV_VE_OK) break;
            if (f.smallest_len < 8 || f.largest_len < 8) e.flags |= LV_VE_FLAG_SHORT_KEY;
            sink.file(r.nf, f);
            ++r.nf;
        } else {
            st = LV_VE_UNKNOWN_TAG;
        }
    }
    if (st != LV_VE_OK) r = VdRes{};  // the reference returns Err: nothing of the object is a result
    r.e.status = st;
    return r;
}

// Kernel 0 (one thread): the head.  A kernel, not a memset: a memset node inside a longer captured
// graph does not replay reliably (DESIGN, mt_init), and a chain of kernels does.
__global__ void vd_init(VdHead *h) { *h = VdHead{}; }

// Kernel 1: the count walk.  A workgroup takes tile blockIdx.x, each wave 64
// consecutive records of it: every lane walks its own if it is small, then the
// wave walks the large ones among them one after another.
__global__ __launch_bounds__(kVdThreads) void vd_count(const VdArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[kVdWaves][kVdWindow + kWinPad];
    __shared__ unsigned long long s_sum[3], s_fb, s_lh[5];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t n = records_to_walk(A.records, A.upstream, A.rec_cap);
    const uint64_t tile = blockIdx.x;
    if (tile * kVdTile >= n) return;  // the whole workgroup
    if (tid < 3) s_sum[tid] = 0;
    if (tid < 5) s_lh[tid] = 0;
    if (tid == 0) s_fb = ~0ull;
    __syncthreads();
    const uint64_t r = tile * kVdTile + tid;
    uint64_t off, len;
    const uint32_t cls = record_class<kVdSmall>(A.rec_off, A.rec_len, A.payload_bytes, r, n, &off, &len);
    VdRes res{};
    res.e.status = cls == kRecOutOfRange ? LV_VE_OUT_OF_RANGE : LV_VE_OK;
    dispatch(
        cls, off, len,
        [&] {
            LaneSrc src(A.payload);
            VdNoSink sink;
            res = vd_walk(src, sink, off, len);
        },
        [&](uint32_t b, uint64_t woff, uint64_t wlen) {
            WaveSrc<kVdWindow, kVdRound> src(A.payload, s_win[wave], woff + wlen, lane);
            VdNoSink sink;
            const VdRes wr = vd_walk(src, sink, woff, wlen);
            if (lane == b) res = wr;
        });
    const bool live = r < n, bad = live && res.e.status != LV_VE_OK;
    if (live) {
        A.edits[r] = res.e;
        A.cnt[3 * r + 0] = res.nf;
        A.cnt[3 * r + 1] = res.nd;
        A.cnt[3 * r + 2] = res.np;
    }
    const uint64_t sf = wave_sum(live ? res.nf : 0), sd = wave_sum(live ? res.nd : 0),
                   sp = wave_sum(live ? res.np : 0), sb = wave_sum(bad ? 1 : 0);
    const uint64_t fb = wave_min(bad ? r : ~0ull);
    if (lane == 0) {
        if (sf) atomicAdd(&s_sum[0], static_cast<unsigned long long>(sf));
        if (sd) atomicAdd(&s_sum[1], static_cast<unsigned long long>(sd));
        if (sp) atomicAdd(&s_sum[2], static_cast<unsigned long long>(sp));
        if (sb) atomicAdd(&A.head->bad, static_cast<unsigned long long>(sb));
        if (fb != ~0ull) atomicMin(&s_fb, static_cast<unsigned long long>(fb));
    }
    __syncthreads();
    const bool before = live && r < s_fb;
#pragma unroll
    for (uint32_t b = 0; b < 5; ++b) {
        const uint64_t v = wave_max(before && ((res.e.has >> b) & 1u) ? r + 1 : 0);
        if (lane == 0 && v) atomicMax(&s_lh[b], static_cast<unsigned long long>(v));
    }
    __syncthreads();
    if (tid < 3) A.tsum[3 * tile + tid] = s_sum[tid];
    if (tid == 0) A.tinfo[6 * tile] = s_fb;
    if (tid < 5) A.tinfo[6 * tile + 1 + tid] = s_lh[tid];
}

// Kernel 2 (one wave): the tiles' three columns become their exclusive scans;
// the first bad record and last_has over the tiles; the totals and the status.
__global__ __launch_bounds__(64) void vd_tiles(const VdArgs A) {
    const uint32_t lane = threadIdx.x;
    const uint64_t n = records_to_walk(A.records, A.upstream, A.rec_cap);
    const uint64_t tiles = (n + kVdTile - 1) / kVdTile;
    uint64_t sum[3];
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) sum[c] = carry_scan(A.tsum + c, 3, tiles, lane);
    uint64_t fb = ~0ull;
    for (uint64_t t = lane; t < tiles; t += 64) {
        const uint64_t v = A.tinfo[6 * t];
        fb = v < fb ? v : fb;
    }
    fb = wave_min(fb);
    // tiles before the first bad record's hold no bad record: their last-with-bit is the whole tile's
    const uint64_t upto = fb == ~0ull ? tiles : fb / kVdTile + 1;
    uint64_t lh[5] = {0, 0, 0, 0, 0};
    for (uint64_t t = lane; t < upto; t += 64)
#pragma unroll
        for (uint32_t b = 0; b < 5; ++b) {
            const uint64_t v = A.tinfo[6 * t + 1 + b];
            lh[b] = v > lh[b] ? v : lh[b];
        }
#pragma unroll
    for (uint32_t b = 0; b < 5; ++b) lh[b] = wave_max(lh[b]);
    if (lane == 0) {
        uint64_t status = 0;
        const bool up = A.upstream && *A.upstream;
        if (up) status |= LV_VE_DECODE_UPSTREAM;
        if (!up && *A.records > A.rec_cap) status |= LV_VE_DECODE_REC_OVER;
        if (sum[0] > A.out.file_cap) status |= LV_VE_DECODE_FILE_OVER;
        if (sum[1] > A.out.deleted_cap) status |= LV_VE_DECODE_DELETED_OVER;
        if (sum[2] > A.out.pointer_cap) status |= LV_VE_DECODE_POINTER_OVER;
        lv_ve_totals tot{};
        tot.records = up ? 0ull : *A.records;
        tot.files = sum[0];
        tot.deleted = sum[1];
        tot.pointers = sum[2];
        tot.bad_records = A.head->bad;
        tot.first_bad = n ? (fb == ~0ull ? n : fb) : 0;
#pragma unroll
        for (uint32_t b = 0; b < 5; ++b) tot.last_has[b] = lh[b];
        tot.status = status;
        *A.out.d_totals = tot;
        A.head->n = n;
        A.head->status = status;
        if (!status) {
            A.out.d_rec_file[n] = sum[0];
            A.out.d_rec_deleted[n] = sum[1];
            A.out.d_rec_pointer[n] = sum[2];
        }
    }
}

// Kernel 3: the emit walk.  The scan of the tile's counts gives each record's
// three bases; the records with rows are walked again, as in vd_count.
__global__ __launch_bounds__(kVdThreads) void vd_emit(const VdArgs A) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[kVdWaves][kVdWindow + kWinPad];
    __shared__ uint64_t s_scan[3 * kVdTile];
    if (A.head->status) return;  // only the totals are written
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t n = A.head->n;
    const uint64_t tile = blockIdx.x;
    if (tile * kVdTile >= n) return;  // the whole workgroup
    const uint64_t r = tile * kVdTile + tid;
    uint64_t c[3];
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
        c[k] = r < n ? A.cnt[3 * r + k] : 0ull;
        s_scan[3 * tid + k] = c[k];
    }
    __syncthreads();
    tile_scan<3 * kVdTile, kVdThreads>(s_scan, 3, tid);
    uint64_t base[3];
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) base[k] = A.tsum[3 * tile + k] + s_scan[3 * tid + k] - c[k];
    uint64_t off, len;
    uint32_t cls = record_class<kVdSmall>(A.rec_off, A.rec_len, A.payload_bytes, r, n, &off, &len);
    if (r < n) {
        A.out.d_rec_file[r] = base[0];
        A.out.d_rec_deleted[r] = base[1];
        A.out.d_rec_pointer[r] = base[2];
        A.out.d_edits[r] = A.edits[r];
    }
    if (!(c[0] | c[1] | c[2])) cls = kRecNone;  // nothing to write
    dispatch(
        cls, off, len,
        [&] {
            LaneSrc src(A.payload);
            VdSink sink{A.out, base[0], base[1], base[2], 0, 0};
            vd_walk(src, sink, off, len);
        },
        [&](uint32_t b, uint64_t woff, uint64_t wlen) {
            WaveSrc<kVdWindow, kVdRound> src(A.payload, s_win[wave], woff + wlen, lane);
            VdSink sink{A.out, shfl64(base[0], b), shfl64(base[1], b), shfl64(base[2], b), lane, 63u};
            vd_walk(src, sink, woff, wlen);
        });
}

// ============================ encode ========================================
constexpr uint32_t kVeThreads = 256;
constexpr uint32_t kVeTile = 1024;      // items per scan tile
constexpr uint32_t kVePer = kVeTile / kVeThreads;
constexpr uint32_t kVeWaveCopy = 64;    // bytes from which a copy is a lane group's
constexpr uint32_t kVeCopyLanes = 16;   // lanes of a wave that share one such copy
static_assert(kVeTile % kVeThreads == 0, "a tile is whole rounds of a workgroup");

struct VeHead {  // workspace, zeroed by ve_init
    uint64_t st0;  // ve_validate: UPSTREAM or REC_OVER
    uint64_t n;    // the records to encode (0 with st0)
    uint64_t go;   // ve_carry: status 0 and something to write
    // the lowest failing (record, kind) / (kind, row) as the maximum of its complement (0: none)
    unsigned long long bad_rec, bad_item;
    uint64_t pad[3];
};

struct VeArgs {
    const uint8_t *src;
    uint64_t src_bytes;
    lv_ve_encode_in in;
    const uint64_t *records, *upstream;
    uint64_t rec_cap;
    lv_ve_encode_out out;
    uint64_t seg[5];  // the first item of each kind (EDIT, POINTER, DELETED, FILE), then the item count
    // workspace
    VeHead *head;
    uint64_t *pre;   // [items] the bytes of the items before item j in its tile
    uint64_t *tsum;  // [tiles] the tiles' bytes, then (ve_carry) the bytes before the tile
    uint64_t *tkey;  // [tiles] the tiles' comparator and key bytes
};

__device__ __forceinline__ uint32_t ve_kind(const VeArgs &A, uint64_t item) {
    return (item >= A.seg[1]) + (item >= A.seg[2]) + (item >= A.seg[3]);
}
__device__ __forceinline__ const uint64_t *ve_bounds(const VeArgs &A, uint32_t kind) {
    return kind == LV_VE_KIND_POINTER ? A.in.d_rec_pointer : kind == LV_VE_KIND_DELETED ? A.in.d_rec_deleted : A.in.d_rec_file;
}
// The bytes of all items before slot i of `kind` (i <= its cap; behind ve_carry).
__device__ __forceinline__ uint64_t ve_before(const VeArgs &A, uint32_t kind, uint64_t i) {
    const uint64_t j = A.seg[kind] + i;
    return A.pre[j] + A.tsum[j / kVeTile];
}
// The bytes of record r's rows of `kind`.
__device__ __forceinline__ uint64_t ve_rows(const VeArgs &A, uint32_t kind, uint64_t r) {
    const uint64_t *b = ve_bounds(A, kind);
    return ve_before(A, kind, b[r + 1]) - ve_before(A, kind, b[r]);
}
// Where record r begins in d_out.
__device__ __forceinline__ uint64_t ve_rec_off(const VeArgs &A, uint64_t r) {
    uint64_t at = ve_before(A, LV_VE_KIND_EDIT, r);
#pragma unroll
    for (uint32_t k = LV_VE_KIND_POINTER; k <= LV_VE_KIND_FILE; ++k) {
        const uint64_t *b = ve_bounds(A, k);
        at += ve_before(A, k, b[r]) - ve_before(A, k, b[0]);
    }
    return at;
}

// Kernel 0 (one thread): the head (a kernel, not a memset: see vd_init).
__global__ void ve_init(VeHead *h) { *h = VeHead{}; }

// Kernel 1: UPSTREAM and REC_OVER, then the three bounds arrays, a lane per record.
__global__ __launch_bounds__(kVeThreads) void ve_validate(const VeArgs A) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kVeThreads + threadIdx.x;
    uint64_t st0 = 0, n = 0;
    if (A.upstream && *A.upstream) {
        st0 = LV_VE_ENCODE_UPSTREAM;
    } else {
        n = *A.records;
        if (n > A.rec_cap) {
            st0 = LV_VE_ENCODE_REC_OVER;
            n = 0;
        }
    }
    if (r == 0) {  // (nobody reads these during this launch)
        A.head->st0 = st0;
        A.head->n = n;
    }
    if (r < n) {
        const uint64_t cap[4] = {0, A.in.pointer_cap, A.in.deleted_cap, A.in.file_cap};
#pragma unroll
        for (uint32_t k = LV_VE_KIND_FILE; k >= LV_VE_KIND_POINTER; --k) {  // (the maximum keeps the lowest kind)
            const uint64_t *b = ve_bounds(A, k);
            const uint64_t lo = b[r], hi = b[r + 1];
            if (!(lo <= hi && hi <= cap[k])) atomicMax(&A.head->bad_rec, static_cast<unsigned long long>(~((r << 2) | k)));
        }
    }
}

// Kernel 2: the items' checks and sizes, the tile-local scan.  No byte of d_src is read.
__global__ __launch_bounds__(kVeThreads) void ve_size(const VeArgs A) {
    __shared__ uint64_t s[kVeTile];
    __shared__ uint64_t s_key[kVeThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const VeHead *h = A.head;
    const uint64_t n = h->n;
    if (!n || h->bad_rec) return;  // no row is read
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kVeTile;
    const uint32_t kind = ve_kind(A, base);  // a tile holds one kind
    const uint64_t *b = kind ? ve_bounds(A, kind) : nullptr;
    const uint64_t lo = kind ? b[0] : 0, hi = kind ? b[n] : n;
    uint64_t own[kVePer], kb = 0;
#pragma unroll
    for (uint32_t k = 0; k < kVePer; ++k) {
        const uint32_t j = tid + k * kVeThreads;
        const uint64_t i = base + j - A.seg[kind];
        uint64_t v = 0;
        if (lo <= i && i < hi) {
            bool ok;
            if (kind == LV_VE_KIND_EDIT) {
                const lv_ve_edit e = A.in.d_edits[i];
                const bool cmp = e.has & LV_VE_HAS_COMPARATOR;
                ok = !(e.has & ~LV_VE_HAS_ALL) && (!cmp || extent_ok(e.comparator_off, e.comparator_len, A.src_bytes));
                if (cmp) {
                    v += 1 + varint_len(e.comparator_len) + static_cast<uint64_t>(e.comparator_len);
                    kb += e.comparator_len;
                }
                if (e.has & LV_VE_HAS_LOG_NUMBER) v += 1 + varint_len(e.log_number);
                if (e.has & LV_VE_HAS_PREV_LOG_NUMBER) v += 1 + varint_len(e.prev_log_number);
                if (e.has & LV_VE_HAS_NEXT_FILE) v += 1 + varint_len(e.next_file_number);
                if (e.has & LV_VE_HAS_LAST_SEQUENCE) v += 1 + varint_len(e.last_sequence);
            } else if (kind == LV_VE_KIND_POINTER) {
                const lv_ve_pointer q = A.in.d_pointers[i];
                ok = q.level < LV_VE_NUM_LEVELS && extent_ok(q.key_off, q.key_len, A.src_bytes);
                v = 2 + varint_len(q.key_len) + static_cast<uint64_t>(q.key_len);
                kb += q.key_len;
            } else if (kind == LV_VE_KIND_DELETED) {
                const lv_ve_deleted d = A.in.d_deleted[i];
                ok = d.level < LV_VE_NUM_LEVELS;
                if (ok && i > lo && b[record_of(b, i, 0, n - 1)] != i) {  // not its record's first row
                    const lv_ve_deleted q = A.in.d_deleted[i - 1];
                    ok = q.level < d.level || (q.level == d.level && q.number < d.number);
                }
                v = 2 + varint_len(d.number);
            } else {
                const lv_ve_file f = A.in.d_files[i];
                ok = f.level < LV_VE_NUM_LEVELS && extent_ok(f.smallest_off, f.smallest_len, A.src_bytes) &&
                     extent_ok(f.largest_off, f.largest_len, A.src_bytes);
                v = 2 + varint_len(f.number) + varint_len(f.file_size) + varint_len(f.smallest_len) +
                    varint_len(f.largest_len) + static_cast<uint64_t>(f.smallest_len) + f.largest_len;
                kb += static_cast<uint64_t>(f.smallest_len) + f.largest_len;
            }
            if (!ok) atomicMax(&A.head->bad_item, ~((static_cast<unsigned long long>(kind) << 60) | i));
        }
        own[k] = v;
        s[j] = v;
    }
    __syncthreads();
    tile_scan<kVeTile, kVeThreads>(s, 1, tid);
#pragma unroll
    for (uint32_t k = 0; k < kVePer; ++k) {
        const uint32_t j = tid + k * kVeThreads;
        A.pre[base + j] = s[j] - own[k];
    }
    kb = wave_sum(kb);  // (every lane is here)
    if (lane == 0) s_key[tid >> 6] = kb;
    __syncthreads();
    if (tid == 0) {
        uint64_t k = 0;
#pragma unroll
        for (uint32_t w = 0; w < kVeThreads / 64; ++w) k += s_key[w];
        A.tsum[blockIdx.x] = s[kVeTile - 1];
        A.tkey[blockIdx.x] = k;
    }
}

// Kernel 3 (one wave): the tiles' sums become their exclusive scan; the totals
// and the status, once, before any byte of the outputs is written.
__global__ __launch_bounds__(64) void ve_carry(const VeArgs A) {
    VeHead *h = A.head;
    const uint32_t lane = threadIdx.x;
    lv_ve_encode_totals t{};
    t.bad_record = t.bad_kind = t.bad_row = ~0ull;
    const uint64_t n = h->n;  // (wave-uniform, like every branch below)
    if (h->st0) {
        t.status = h->st0;
        if (h->st0 == LV_VE_ENCODE_REC_OVER) t.records = *A.records;
    } else if (h->bad_rec) {
        const uint64_t v = ~static_cast<uint64_t>(h->bad_rec);
        t.status = LV_VE_ENCODE_BAD_BOUNDS;
        t.records = n;
        t.bad_record = v >> 2;
        t.bad_kind = v & 3u;
    } else if (h->bad_item) {
        const uint64_t v = ~static_cast<uint64_t>(h->bad_item);
        t.status = LV_VE_ENCODE_BAD_ROW;
        t.records = n;
        t.bad_kind = v >> 60;
        t.bad_row = v & ((1ull << 60) - 1);
        t.bad_record = t.bad_kind ? record_of(ve_bounds(A, static_cast<uint32_t>(t.bad_kind)), t.bad_row, 0, n - 1) : t.bad_row;
    } else if (n) {
        const uint64_t tiles = A.seg[4] / kVeTile;
        t.out_bytes = carry_scan(A.tsum, 1, tiles, lane);
        uint64_t kb = 0;
        for (uint64_t i = lane; i < tiles; i += 64) kb += A.tkey[i];
        t.key_bytes = wave_sum(kb);
        t.records = n;
        t.files = A.in.d_rec_file[n] - A.in.d_rec_file[0];
        t.deleted = A.in.d_rec_deleted[n] - A.in.d_rec_deleted[0];
        t.pointers = A.in.d_rec_pointer[n] - A.in.d_rec_pointer[0];
        if (t.out_bytes > A.out.out_cap) t.status = LV_VE_ENCODE_OUT_OVER;
        if (lane == 0) h->go = !t.status;
    }
    if (lane == 0) *A.out.d_totals = t;
}

// Kernel 4: a lane per item.  An edit's lane writes its record's extent and
// scalar group, a row's lane its row; the comparator and the keys are
// lvk::group_copy's, so every lane of a wave stays to the end.
__global__ __launch_bounds__(kVeThreads) void ve_emit(const VeArgs A) {
    const VeHead *h = A.head;
    if (!h->go) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n = h->n;
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kVeThreads + threadIdx.x;
    const uint32_t kind = ve_kind(A, j);  // (a workgroup holds one kind: kVeTile is a multiple of its size)
    const uint64_t i = j - A.seg[kind];
    const uint64_t *b = kind ? ve_bounds(A, kind) : nullptr;
    const uint64_t lo = kind ? b[0] : 0, hi = kind ? b[n] : n;
    uint8_t *d0 = nullptr, *d1 = nullptr;
    const uint8_t *s0 = nullptr, *s1 = nullptr;
    uint64_t n0 = 0, n1 = 0;
    if (lo <= i && i < hi) {
        if (kind == LV_VE_KIND_EDIT) {
            const lv_ve_edit e = A.in.d_edits[i];
            const uint64_t off = ve_rec_off(A, i);
            A.out.d_rec_off[i] = off;
            A.out.d_rec_len[i] = ve_before(A, LV_VE_KIND_EDIT, i + 1) - ve_before(A, LV_VE_KIND_EDIT, i) +
                                 ve_rows(A, LV_VE_KIND_POINTER, i) + ve_rows(A, LV_VE_KIND_DELETED, i) +
                                 ve_rows(A, LV_VE_KIND_FILE, i);
            uint8_t *p = A.out.d_out + off;
            if (e.has & LV_VE_HAS_COMPARATOR) {
                *p++ = 1;
                p = put_varint(p, e.comparator_len);
                d0 = p;
                s0 = A.src + e.comparator_off;
                n0 = e.comparator_len;
                p += n0;
            }
            if (e.has & LV_VE_HAS_LOG_NUMBER) {
                *p++ = 2;
                p = put_varint(p, e.log_number);
            }
            if (e.has & LV_VE_HAS_PREV_LOG_NUMBER) {
                *p++ = 9;
                p = put_varint(p, e.prev_log_number);
            }
            if (e.has & LV_VE_HAS_NEXT_FILE) {
                *p++ = 3;
                p = put_varint(p, e.next_file_number);
            }
            if (e.has & LV_VE_HAS_LAST_SEQUENCE) {
                *p++ = 4;
                p = put_varint(p, e.last_sequence);
            }
        } else {
            const uint64_t r = record_of(b, i, 0, n - 1);
            // the record, its scalar group, the kinds before this one, the rows of this kind before this one
            uint64_t at = ve_rec_off(A, r) + ve_before(A, LV_VE_KIND_EDIT, r + 1) - ve_before(A, LV_VE_KIND_EDIT, r);
            if (kind > LV_VE_KIND_POINTER) at += ve_rows(A, LV_VE_KIND_POINTER, r);
            if (kind > LV_VE_KIND_DELETED) at += ve_rows(A, LV_VE_KIND_DELETED, r);
            at += ve_before(A, kind, i) - ve_before(A, kind, b[r]);
            uint8_t *p = A.out.d_out + at;
            if (kind == LV_VE_KIND_POINTER) {
                const lv_ve_pointer q = A.in.d_pointers[i];
                *p++ = 5;
                *p++ = static_cast<uint8_t>(q.level);
                p = put_varint(p, q.key_len);
                d0 = p;
                s0 = A.src + q.key_off;
                n0 = q.key_len;
            } else if (kind == LV_VE_KIND_DELETED) {
                const lv_ve_deleted d = A.in.d_deleted[i];
                *p++ = 6;
                *p++ = static_cast<uint8_t>(d.level);
                p = put_varint(p, d.number);
            } else {
                const lv_ve_file f = A.in.d_files[i];
                *p++ = 7;
                *p++ = static_cast<uint8_t>(f.level);
                p = put_varint(p, f.number);
                p = put_varint(p, f.file_size);
                p = put_varint(p, f.smallest_len);
                d0 = p;
                s0 = A.src + f.smallest_off;
                n0 = f.smallest_len;
                p += n0;
                p = put_varint(p, f.largest_len);
                d1 = p;
                s1 = A.src + f.largest_off;
                n1 = f.largest_len;
            }
        }
    }
    group_copy<kVeCopyLanes, kVeWaveCopy>(d0, s0, n0, lane);
    group_copy<kVeCopyLanes, kVeWaveCopy>(d1, s1, n1, lane);
}

// ============================ files =========================================
__global__ void ve_files_init(unsigned long long *status) { *status = 0; }

__global__ __launch_bounds__(256) void ve_files(const lv_version_file *vf, const lv_sst_table *tables,
                                                 const uint64_t *count, uint64_t cap, lv_ve_file *rows,
                                                 uint64_t *rec_file, unsigned long long *status) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint64_t total = *count, n = total < cap ? total : cap;
    if (i == 0) {
        if (rec_file) {
            rec_file[0] = 0;
            rec_file[1] = n;
        }
        if (total > cap) atomicAdd(status, static_cast<unsigned long long>(total - cap));
    }
    if (i >= n) return;
    const lv_version_file f = vf[i];
    const lv_sst_table t = tables[i];
    lv_ve_file row{};
    row.number = f.number;
    row.file_size = t.file_bytes;
    row.smallest_off = f.smallest_off;
    row.largest_off = f.largest_off;
    row.smallest_len = f.smallest_len;
    row.largest_len = f.largest_len;
    row.level = f.level;
    rows[i] = row;
    if (f.status || t.status) atomicAdd(status, 1ull);
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxRecCap = 0xfffffffeull;
constexpr uint64_t kMaxDecodeRows = 1ull << 56;  // cap * 48 stays far from 2^64
constexpr uint64_t kMaxEncodeRows = 1ull << 30;  // no sum of sizes leaves u64 (version_edit.h)

constexpr uint64_t vd_tiles_of(uint64_t cap) { return (cap + lvk::kVdTile - 1) / lvk::kVdTile; }

void vd_carve(Carve &C, uint64_t cap, lvk::VdArgs &A) {
    A.head = C.take<lvk::VdHead>(1);
    A.edits = C.take<lv_ve_edit>(cap);
    A.cnt = C.take<uint64_t>(3 * cap);
    A.tsum = C.take<uint64_t>(3 * vd_tiles_of(cap));
    A.tinfo = C.take<uint64_t>(6 * vd_tiles_of(cap));
}

// cap + 1 slots in whole tiles
constexpr uint64_t ve_slots(uint64_t cap) { return (cap + 1 + lvk::kVeTile - 1) / lvk::kVeTile * lvk::kVeTile; }

void ve_carve(Carve &C, uint64_t rec_cap, uint64_t file_cap, uint64_t deleted_cap, uint64_t pointer_cap, lvk::VeArgs &A) {
    A.seg[0] = 0;
    A.seg[1] = A.seg[0] + ve_slots(rec_cap);
    A.seg[2] = A.seg[1] + ve_slots(pointer_cap);
    A.seg[3] = A.seg[2] + ve_slots(deleted_cap);
    A.seg[4] = A.seg[3] + ve_slots(file_cap);
    A.head = C.take<lvk::VeHead>(1);
    A.pre = C.take<uint64_t>(A.seg[4]);
    A.tsum = C.take<uint64_t>(A.seg[4] / lvk::kVeTile);
    A.tkey = C.take<uint64_t>(A.seg[4] / lvk::kVeTile);
}

}  // namespace

extern "C" {

size_t lv_version_edit_decode_workspace_bytes(size_t rec_cap) {
    lvk::VdArgs A{};
    Carve C{nullptr};
    vd_carve(C, rec_cap, A);
    return C.at;
}

int lv_version_edit_decode_device(const uint8_t *d_payload, size_t payload_bytes, const uint64_t *d_rec_off,
                                  const uint64_t *d_rec_len, const uint64_t *d_records,
                                  const uint64_t *d_upstream_status, size_t rec_cap, const lv_ve_decode_out *out,
                                  uint32_t flags, void *d_workspace, size_t workspace_bytes, void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (!out) return set_err(LV_ERR_INVALID, "null output descriptor");
    if (!out->d_totals) return set_err(LV_ERR_INVALID, "null d_totals");
    if (misaligned(out->d_totals, 8)) return set_err(LV_ERR_INVALID, "d_totals must be 8-byte aligned");
    if (!d_records) return set_err(LV_ERR_INVALID, "null d_records");
    if (!d_payload && payload_bytes) return set_err(LV_ERR_INVALID, "null d_payload");
    if (rec_cap > kMaxRecCap) return set_err(LV_ERR_INVALID, "rec_cap too large for one decode (at most 2^32 - 2)");
    if (out->file_cap > kMaxDecodeRows || out->deleted_cap > kMaxDecodeRows || out->pointer_cap > kMaxDecodeRows)
        return set_err(LV_ERR_INVALID, "row capacity too large (at most 2^56)");
    if (rec_cap && (!d_rec_off || !d_rec_len)) return set_err(LV_ERR_INVALID, "null record array (d_rec_off / d_rec_len)");
    if (rec_cap && !out->d_edits) return set_err(LV_ERR_INVALID, "null d_edits");
    if (!out->d_rec_file || !out->d_rec_deleted || !out->d_rec_pointer)
        return set_err(LV_ERR_INVALID, "null bounds array (d_rec_file / d_rec_deleted / d_rec_pointer)");
    if (misaligned(out->d_rec_file, 8) || misaligned(out->d_rec_deleted, 8) || misaligned(out->d_rec_pointer, 8))
        return set_err(LV_ERR_INVALID, "the bounds arrays must be 8-byte aligned");
    if ((out->file_cap && !out->d_files) || (out->deleted_cap && !out->d_deleted) || (out->pointer_cap && !out->d_pointers))
        return set_err(LV_ERR_INVALID, "null row table (d_files / d_deleted / d_pointers)");
    if (misaligned(out->d_edits, 16) || misaligned(out->d_files, 16) || misaligned(out->d_deleted, 16) ||
        misaligned(out->d_pointers, 16))
        return set_err(LV_ERR_INVALID, "d_edits and the row tables must be 16-byte aligned");
    if (!d_workspace) return set_err(LV_ERR_INVALID, "null workspace");
    if (misaligned(d_workspace, 16)) return set_err(LV_ERR_INVALID, "workspace must be 16-byte aligned");
    lvk::VdArgs A{};
    Carve C{static_cast<uint8_t *>(d_workspace)};
    vd_carve(C, rec_cap, A);
    if (workspace_bytes < C.at) return set_err(LV_ERR_INVALID, "workspace too small");
    if (overlaps(out->d_files, static_cast<uint64_t>(out->file_cap) * sizeof(lv_ve_file), d_payload, payload_bytes) ||
        overlaps(out->d_deleted, static_cast<uint64_t>(out->deleted_cap) * sizeof(lv_ve_deleted), d_payload, payload_bytes) ||
        overlaps(out->d_pointers, static_cast<uint64_t>(out->pointer_cap) * sizeof(lv_ve_pointer), d_payload, payload_bytes))
        return set_err(LV_ERR_INVALID, "a row table overlaps d_payload");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    A.payload = d_payload;
    A.payload_bytes = payload_bytes;
    A.rec_off = d_rec_off;
    A.rec_len = d_rec_len;
    A.records = d_records;
    A.upstream = d_upstream_status;
    A.rec_cap = rec_cap;
    A.out = *out;

    const dim3 b(lvk::kVdThreads);
    const uint32_t grid = static_cast<uint32_t>(vd_tiles_of(rec_cap));
    hipLaunchKernelGGL(lvk::vd_init, dim3(1), dim3(1), 0, s, A.head);
    if (grid) hipLaunchKernelGGL(lvk::vd_count, dim3(grid), b, 0, s, A);
    hipLaunchKernelGGL(lvk::vd_tiles, dim3(1), dim3(64), 0, s, A);
    if (grid) hipLaunchKernelGGL(lvk::vd_emit, dim3(grid), b, 0, s, A);
    g_kernel = "vd_init+vd_count+vd_tiles+vd_emit";
    return check_launch();
}

size_t lv_version_edit_encode_workspace_bytes(size_t rec_cap, size_t file_cap, size_t deleted_cap, size_t pointer_cap) {
    if (rec_cap > kMaxRecCap || file_cap > kMaxEncodeRows || deleted_cap > kMaxEncodeRows || pointer_cap > kMaxEncodeRows)
        return 0;
    lvk::VeArgs A{};
    Carve C{nullptr};
    ve_carve(C, rec_cap, file_cap, deleted_cap, pointer_cap, A);
    return C.at;
}

int lv_version_edit_encode_device(const uint8_t *d_src, size_t src_bytes, const lv_ve_encode_in *in,
                                  const uint64_t *d_records, const uint64_t *d_upstream_status, size_t rec_cap,
                                  const lv_ve_encode_out *out, uint32_t flags, void *d_workspace,
                                  size_t workspace_bytes, void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (!in || !out) return set_err(LV_ERR_INVALID, "null input or output descriptor");
    if (!out->d_totals) return set_err(LV_ERR_INVALID, "null d_totals");
    if (misaligned(out->d_totals, 8)) return set_err(LV_ERR_INVALID, "d_totals must be 8-byte aligned");
    if (!d_records) return set_err(LV_ERR_INVALID, "null d_records");
    if (!d_src && src_bytes) return set_err(LV_ERR_INVALID, "null d_src");
    if (rec_cap > kMaxRecCap) return set_err(LV_ERR_INVALID, "rec_cap too large for one encode (at most 2^32 - 2)");
    if (in->file_cap > kMaxEncodeRows || in->deleted_cap > kMaxEncodeRows || in->pointer_cap > kMaxEncodeRows)
        return set_err(LV_ERR_INVALID, "row capacity too large for one encode (at most 2^30)");
    if (!in->d_rec_file || !in->d_rec_deleted || !in->d_rec_pointer)
        return set_err(LV_ERR_INVALID, "null bounds array (d_rec_file / d_rec_deleted / d_rec_pointer)");
    if (misaligned(in->d_rec_file, 8) || misaligned(in->d_rec_deleted, 8) || misaligned(in->d_rec_pointer, 8))
        return set_err(LV_ERR_INVALID, "the bounds arrays must be 8-byte aligned");
    if (rec_cap && (!in->d_edits || !out->d_rec_off || !out->d_rec_len))
        return set_err(LV_ERR_INVALID, "null record array (d_edits / d_rec_off / d_rec_len)");
    if (misaligned(out->d_rec_off, 8) || misaligned(out->d_rec_len, 8))
        return set_err(LV_ERR_INVALID, "d_rec_off and d_rec_len must be 8-byte aligned");
    if ((in->file_cap && !in->d_files) || (in->deleted_cap && !in->d_deleted) || (in->pointer_cap && !in->d_pointers))
        return set_err(LV_ERR_INVALID, "null row table (d_files / d_deleted / d_pointers)");
    if (misaligned(in->d_edits, 16) || misaligned(in->d_files, 16) || misaligned(in->d_deleted, 16) ||
        misaligned(in->d_pointers, 16))
        return set_err(LV_ERR_INVALID, "d_edits and the row tables must be 16-byte aligned");
    if (out->out_cap && !out->d_out) return set_err(LV_ERR_INVALID, "null d_out");
    if (!d_workspace) return set_err(LV_ERR_INVALID, "null workspace");
    if (misaligned(d_workspace, 16)) return set_err(LV_ERR_INVALID, "workspace must be 16-byte aligned");
    lvk::VeArgs A{};
    Carve C{static_cast<uint8_t *>(d_workspace)};
    ve_carve(C, rec_cap, in->file_cap, in->deleted_cap, in->pointer_cap, A);
    if (workspace_bytes < C.at) return set_err(LV_ERR_INVALID, "workspace too small");
    if (overlaps(out->d_out, out->out_cap, d_src, src_bytes)) return set_err(LV_ERR_INVALID, "d_out overlaps d_src");
    if (overlaps(out->d_out, out->out_cap, in->d_edits, static_cast<uint64_t>(rec_cap) * sizeof(lv_ve_edit)) ||
        overlaps(out->d_out, out->out_cap, in->d_files, static_cast<uint64_t>(in->file_cap) * sizeof(lv_ve_file)) ||
        overlaps(out->d_out, out->out_cap, in->d_deleted, static_cast<uint64_t>(in->deleted_cap) * sizeof(lv_ve_deleted)) ||
        overlaps(out->d_out, out->out_cap, in->d_pointers, static_cast<uint64_t>(in->pointer_cap) * sizeof(lv_ve_pointer)))
        return set_err(LV_ERR_INVALID, "d_out overlaps a table");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    A.src = d_src;
    A.src_bytes = src_bytes;
    A.in = *in;
    A.records = d_records;
    A.upstream = d_upstream_status;
    A.rec_cap = rec_cap;
    A.out = *out;

    const dim3 b(lvk::kVeThreads);
    // a lane per record, at least one workgroup: its first thread judges UPSTREAM and REC_OVER
    const uint32_t rec_grid =
        static_cast<uint32_t>(rec_cap ? (static_cast<uint64_t>(rec_cap) + lvk::kVeThreads - 1) / lvk::kVeThreads : 1);
    const uint32_t tiles = static_cast<uint32_t>(A.seg[4] / lvk::kVeTile);
    hipLaunchKernelGGL(lvk::ve_init, dim3(1), dim3(1), 0, s, A.head);
    hipLaunchKernelGGL(lvk::ve_validate, dim3(rec_grid), b, 0, s, A);
    hipLaunchKernelGGL(lvk::ve_size, dim3(tiles), b, 0, s, A);
    hipLaunchKernelGGL(lvk::ve_carry, dim3(1), dim3(64), 0, s, A);
    hipLaunchKernelGGL(lvk::ve_emit, dim3(tiles * lvk::kVePer), b, 0, s, A);
    g_kernel = "ve_init+ve_validate+ve_size+ve_carry+ve_emit";
    return check_launch();
}

int lv_version_edit_files_device(const lv_version_file *d_version_files, const lv_sst_table *d_tables,
                                 const uint64_t *d_file_count, size_t files_cap, lv_ve_file *d_files,
                                 uint64_t *d_rec_file, uint64_t *d_status, void *stream) {
    g_err.clear();
    if (!d_file_count || !d_status) return set_err(LV_ERR_INVALID, "null d_file_count or d_status");
    if (files_cap && (!d_version_files || !d_tables || !d_files))
        return set_err(LV_ERR_INVALID, "null file array (d_version_files / d_tables / d_files)");
    if (files_cap > kMaxEncodeRows) return set_err(LV_ERR_INVALID, "files_cap too large (at most 2^30)");
    if (misaligned(d_files, 16)) return set_err(LV_ERR_INVALID, "d_files must be 16-byte aligned");
    if (misaligned(d_version_files, 8) || misaligned(d_tables, 8) || misaligned(d_file_count, 8) ||
        misaligned(d_rec_file, 8) || misaligned(d_status, 8))
        return set_err(LV_ERR_INVALID, "the record arrays, d_file_count, d_rec_file and d_status must be 8-byte aligned");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t grid = static_cast<uint32_t>(files_cap ? (static_cast<uint64_t>(files_cap) + 255) / 256 : 1);
    hipLaunchKernelGGL(lvk::ve_files_init, dim3(1), dim3(1), 0, s, reinterpret_cast<unsigned long long *>(d_status));
    hipLaunchKernelGGL(lvk::ve_files, dim3(grid), dim3(256), 0, s, d_version_files, d_tables, d_file_count,
                       static_cast<uint64_t>(files_cap), d_files, d_rec_file, reinterpret_cast<unsigned long long *>(d_status));
    g_kernel = "ve_files_init+ve_files";
    return check_launch();
}

}  // extern "C"
