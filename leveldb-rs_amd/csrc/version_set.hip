// lv_version_apply_device (include/lvgpu/version_set.h; csrc/version_set.cc
// holds the serial twin, upstream's Builder written out): the edits of a
// MANIFEST in HBM applied to a version that lv_version_open_device reads.
//
// The Builder keeps a set per level and walks the records one after another;
// here a row is judged on its own.  A pair (level, number) is live iff it has a
// NewFile row in record r and no deleted row in a later record, so two facts
// per pair decide everything: the largest record that deletes it and the
// lowest row that adds it.  Both are order-free reductions (a max and a min)
// into an open-addressing table keyed by (level << 56 | number).
//
//   vs_clear     empties the pair table, a slot per lane; its first thread
//                zeroes the call's head.
//   vs_bounds    a lane per record: UPSTREAM and REC_OVER, the three bounds
//                arrays, and per has bit the last record that carries it.
//   vs_rows      a lane per item (pointers, deleted rows, NewFile rows and
//                directory entries one after another, each kind in whole
//                workgroups): the row's checks; a pointer takes its level's
//                maximum; a deleted row enters max(record + 1), a NewFile row
//                min(row) into its pair's slot; a directory entry is compared
//                with its predecessor.
//   vs_live      a tile of kVsTile NewFile rows: the pair's slot again.  A row
//                that is not its pair's lowest is a duplicate; the lowest is
//                live iff no later record deletes the pair.  A live row is
//                looked up in the directory and counted into its level; the
//                tile's live flags are scanned in LDS.
//   vs_carry     (one wave) the tiles' sums become their exclusive scan; the
//                status, once, and the totals.
//   vs_gather    a lane per NewFile row: a live row becomes a sort entry at its
//                scanned position.
//   vs_tile_sort / vs_merge   lvk/merge_sort.h under the version's order.
//   vs_emit      a lane per live file, in the sorted order.
//
// Every grid is sized by a capacity, one item per lane, no grid-stride loop;
// launches beyond the device-side counts return at once.  The loops that can
// grow with the input are bounded: a probe by the table's slots, a search by
// the 32 bits of an index, the carry by its rounds of 64 tiles.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/version_set.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/merge_sort.h"
#include "lvk/stage.h"

namespace lvk {

constexpr uint32_t kVsThreads = 256;
constexpr uint32_t kVsTile = 1024;  // NewFile rows per scan tile; live files per sort tile
constexpr uint32_t kVsPer = kVsTile / kVsThreads;
constexpr uint32_t kVsPrefix = 16;  // user-key bytes held in a sort entry
constexpr uint32_t kVsNone = 0xffffffffu;
constexpr unsigned long long kVsEmpty = ~0ull;  // no key is: a key is below 7 << 56
static_assert(kVsTile % kVsThreads == 0, "a tile is whole rounds of a workgroup");

struct alignas(16) VsSlot {  // one pair
    unsigned long long key;  // (level << 56) | number
    uint32_t del;            // 1 + the largest record with a deleted row of the pair, 0: none
    uint32_t add;            // the lowest NewFile row of the pair, kVsNone: none
};
static_assert(sizeof(VsSlot) == 16, "slot size");

struct alignas(16) VsEnt {  // a live file in the sort
    uint64_t p[2];          // levels >= 1: the smallest user key's bytes [0, 16) as big-endian words, zero-padded;
                            // level 0: the number, 0
    uint32_t klen, level;   // the user key's length (level 0: 0); kVsNone: a padding entry
    uint32_t row, pad;      // the NewFile row
};
static_assert(sizeof(VsEnt) == 32, "entry size");

struct VsHead {  // workspace, zeroed by vs_clear
    uint64_t st0, n;   // vs_bounds: UPSTREAM or REC_OVER; the records to apply (0 with st0)
    // the lowest failing (record, kind) / (kind, row) / row / entry as the maximum of its complement (0: none)
    unsigned long long bad_rec, bad_item, dup, bad_dir;
    unsigned long long last_has[5], cp[LV_NUM_LEVELS];
    unsigned long long lfiles[LV_NUM_LEVELS], lbytes[LV_NUM_LEVELS], max_number, unplaced;
    uint64_t sorted;  // vs_carry: the files to order and emit (0 with a status)
    uint64_t pad;
};

struct VsArgs {
    const uint8_t *src;
    uint64_t src_bytes;
    lv_ve_encode_in in;
    const uint64_t *records, *upstream;
    uint64_t rec_cap;
    const lv_vs_placement *dir;
    uint64_t dir_n;
    lv_vs_out out;
    uint64_t seg[5];  // the first item of each kind (POINTER, DELETED, FILE, DIRECTORY), then the item count
    uint64_t slots;   // of the pair table: a power of two
    uint64_t ftiles;  // scan tiles over file_cap
    // workspace
    VsHead *head;
    VsSlot *table;
    uint32_t *pre;    // [ftiles kVsTile] (live rows before row i in its tile) << 1 | live
    uint32_t *place;  // [file_cap] a live row's directory index, kVsNone: unplaced
    uint64_t *tsum;   // [ftiles] the tiles' live rows, then (vs_carry) the live rows before the tile
    VsEnt *buf[2];    // [files_cap] each
};

__device__ __forceinline__ uint64_t vs_key(uint32_t level, uint64_t number) {
    return (static_cast<uint64_t>(level) << 56) | number;
}
__device__ __forceinline__ uint64_t vs_hash(uint64_t key) {
    key *= 0x9e3779b97f4a7c15ull;
    return key ^ (key >> 29);
}
// The slot of `key`, claimed if absent (insert) or slots if absent.  The table
// is at most half full, so a probe ends; the bound makes that unconditional.
__device__ __forceinline__ uint64_t vs_slot(const VsArgs &A, uint64_t key, bool insert) {
    const uint64_t mask = A.slots - 1;
    uint64_t h = vs_hash(key) & mask;
    for (uint64_t it = 0; it < A.slots; ++it) {
        unsigned long long cur = __atomic_load_n(&A.table[h].key, __ATOMIC_RELAXED);
        if (cur == kVsEmpty) {
            if (!insert) return A.slots;
            cur = atomicCAS(&A.table[h].key, kVsEmpty, static_cast<unsigned long long>(key));
            if (cur == kVsEmpty) return h;
        }
        if (cur == key) return h;
        h = (h + 1) & mask;
    }
    return A.slots;
}

// The index of `number` in the directory, kVsNone if absent.  Bounded.
__device__ __forceinline__ uint32_t vs_dir_find(const VsArgs &A, uint64_t number) {
    uint64_t lo = 0, hi = A.dir_n;
    for (uint32_t it = 0; it < 33 && lo < hi; ++it) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (A.dir[mid].number < number)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < A.dir_n && A.dir[lo].number == number ? static_cast<uint32_t>(lo) : kVsNone;
}

// Kernel 0: the pair table and the head (a kernel, not a memset: see vd_init).
__global__ __launch_bounds__(kVsThreads) void vs_clear(const VsArgs A) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kVsThreads + threadIdx.x;
    if (i == 0) *A.head = VsHead{};
    if (i < A.slots) A.table[i] = VsSlot{kVsEmpty, 0u, kVsNone};
}

// Kernel 1: UPSTREAM and REC_OVER, the bounds arrays and the scalars' last records, a lane per record.
__global__ __launch_bounds__(kVsThreads) void vs_bounds(const VsArgs A) {
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kVsThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t st0 = 0, n = 0;
    if (A.upstream && *A.upstream) {
        st0 = LV_VS_UPSTREAM;
    } else {
        n = *A.records;
        if (n > A.rec_cap) {
            st0 = LV_VS_REC_OVER;
            n = 0;
        }
    }
    if (r == 0) {  // (nobody reads these during this launch)
        A.head->st0 = st0;
        A.head->n = n;
    }
    uint32_t has = 0;
    if (r < n) {
        const uint64_t cap[4] = {0, A.in.pointer_cap, A.in.deleted_cap, A.in.file_cap};
        const uint64_t *bounds[4] = {nullptr, A.in.d_rec_pointer, A.in.d_rec_deleted, A.in.d_rec_file};
#pragma unroll
        for (uint32_t k = LV_VE_KIND_FILE; k >= LV_VE_KIND_POINTER; --k) {  // (the maximum keeps the lowest kind)
            const uint64_t lo = bounds[k][r], hi = bounds[k][r + 1];
            if (!(lo <= hi && hi <= cap[k])) atomicMax(&A.head->bad_rec, static_cast<unsigned long long>(~((r << 2) | k)));
        }
        has = A.in.d_edits[r].has;
    }
#pragma unroll
    for (uint32_t b = 0; b < 5; ++b) {  // (every lane is here)
        const uint64_t v = wave_max((has >> b) & 1u ? r + 1 : 0);
        if (lane == 0 && v) atomicMax(&A.head->last_has[b], static_cast<unsigned long long>(v));
    }
}

// Kernel 2: a lane per item.  No byte of d_src is read.
__global__ __launch_bounds__(kVsThreads) void vs_rows(const VsArgs A) {
    VsHead *h = A.head;
    const uint64_t n = h->n;
    if (!n || h->bad_rec) return;  // no row is read
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kVsThreads + threadIdx.x;
    const uint32_t kind = 1u + (j >= A.seg[1]) + (j >= A.seg[2]) + (j >= A.seg[3]);  // (a workgroup holds one kind)
    const uint64_t i = j - A.seg[kind - 1];
    if (kind == LV_VS_KIND_DIRECTORY) {
        if (i >= 1 && i < A.dir_n && A.dir[i - 1].number >= A.dir[i].number) atomicMax(&h->bad_dir, ~static_cast<unsigned long long>(i));
        return;
    }
    const uint64_t *b = kind == LV_VE_KIND_POINTER ? A.in.d_rec_pointer : kind == LV_VE_KIND_DELETED ? A.in.d_rec_deleted : A.in.d_rec_file;
    if (!(b[0] <= i && i < b[n])) return;
    bool ok;
    if (kind == LV_VE_KIND_POINTER) {
        const lv_ve_pointer q = A.in.d_pointers[i];
        ok = q.level < LV_NUM_LEVELS && q.key_len >= 8 && extent_ok(q.key_off, q.key_len, A.src_bytes);
        if (ok) atomicMax(&h->cp[q.level], static_cast<unsigned long long>(i + 1));
    } else if (kind == LV_VE_KIND_DELETED) {
        const lv_ve_deleted d = A.in.d_deleted[i];
        ok = d.level < LV_NUM_LEVELS && d.number < LV_VS_MAX_NUMBER;
        if (ok) {
            const uint64_t s = vs_slot(A, vs_key(d.level, d.number), true);
            if (s < A.slots) atomicMax(&A.table[s].del, static_cast<uint32_t>(record_of(b, i, 0, n - 1) + 1));
        }
    } else {
        const lv_ve_file f = A.in.d_files[i];
        ok = f.level < LV_NUM_LEVELS && f.number < LV_VS_MAX_NUMBER && f.smallest_len >= 8 && f.largest_len >= 8 &&
             extent_ok(f.smallest_off, f.smallest_len, A.src_bytes) && extent_ok(f.largest_off, f.largest_len, A.src_bytes);
        if (ok) {
            const uint64_t s = vs_slot(A, vs_key(f.level, f.number), true);
            if (s < A.slots) atomicMin(&A.table[s].add, static_cast<uint32_t>(i));
        }
    }
    if (!ok) atomicMax(&h->bad_item, ~((static_cast<unsigned long long>(kind) << 60) | i));
}

// Kernel 3: liveness, placement and the tile-local scan of a tile of NewFile rows.
__global__ __launch_bounds__(kVsThreads) void vs_live(const VsArgs A) {
    __shared__ uint64_t s[kVsTile];
    __shared__ unsigned long long s_files[LV_NUM_LEVELS], s_bytes[LV_NUM_LEVELS], s_max, s_unplaced;
    const uint32_t tid = threadIdx.x;
    VsHead *h = A.head;
    const uint64_t n = h->n;
    if (!n || h->bad_rec || h->bad_item) return;  // every row was accepted and has its slot
    if (tid < LV_NUM_LEVELS) s_files[tid] = s_bytes[tid] = 0;
    if (tid == 0) s_max = s_unplaced = 0;
    __syncthreads();
    const uint64_t *b = A.in.d_rec_file;
    const uint64_t lo = b[0], hi = b[n];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kVsTile;
    uint32_t own[kVsPer];
#pragma unroll
    for (uint32_t k = 0; k < kVsPer; ++k) {
        const uint32_t j = tid + k * kVsThreads;
        const uint64_t i = base + j;
        uint32_t live = 0;
        if (lo <= i && i < hi) {
            const lv_ve_file f = A.in.d_files[i];
            const uint64_t sl = vs_slot(A, vs_key(f.level, f.number), false);
            if (sl < A.slots) {
                const VsSlot p = A.table[sl];
                if (p.add != static_cast<uint32_t>(i))
                    atomicMax(&h->dup, ~static_cast<unsigned long long>(i));  // an earlier row adds the pair
                else
                    live = p.del <= record_of(b, i, 0, n - 1) + 1;  // no deleted row in a later record
            }
            if (live) {
                uint32_t at = kVsNone;
                if (A.dir_n) {
                    at = vs_dir_find(A, f.number);
                    if (at != kVsNone && A.dir[at].file_cap < f.file_size) at = kVsNone;
                    if (at == kVsNone) atomicAdd(&s_unplaced, 1ull);
                }
                A.place[i] = at;
                atomicAdd(&s_files[f.level], 1ull);
                atomicAdd(&s_bytes[f.level], static_cast<unsigned long long>(f.file_size));
                atomicMax(&s_max, static_cast<unsigned long long>(f.number));
            }
        }
        own[k] = live;
        s[j] = live;
    }
    __syncthreads();
    tile_scan<kVsTile, kVsThreads>(s, 1, tid);
#pragma unroll
    for (uint32_t k = 0; k < kVsPer; ++k) {
        const uint32_t j = tid + k * kVsThreads;
        A.pre[base + j] = (static_cast<uint32_t>(s[j] - own[k]) << 1) | own[k];
    }
    if (tid == 0) {
        A.tsum[blockIdx.x] = s[kVsTile - 1];
        if (s_max) atomicMax(&h->max_number, s_max);
        if (s_unplaced) atomicAdd(&h->unplaced, s_unplaced);
    }
    if (tid < LV_NUM_LEVELS && s_files[tid]) {
        atomicAdd(&h->lfiles[tid], s_files[tid]);
        atomicAdd(&h->lbytes[tid], s_bytes[tid]);
    }
}

// Kernel 4 (one wave): the tiles' sums become their exclusive scan; the status
// and the totals, once, before any row of the outputs is written.
__global__ __launch_bounds__(64) void vs_carry(const VsArgs A) {
    VsHead *h = A.head;
    const uint32_t lane = threadIdx.x;
    lv_vs_totals t{};
    t.bad_kind = t.bad_row = ~0ull;
    const uint64_t n = h->n;  // (wave-uniform, like every branch below)
    t.records = n;
    if (h->st0) {
        t.status = h->st0;
        if (h->st0 == LV_VS_REC_OVER) t.records = *A.records;
    } else if (h->bad_rec) {
        const uint64_t v = ~static_cast<uint64_t>(h->bad_rec);
        t.status = LV_VS_BAD_BOUNDS;
        t.bad_row = v >> 2;
        t.bad_kind = v & 3u;
    } else if (h->bad_item) {
        const uint64_t v = ~static_cast<uint64_t>(h->bad_item);
        t.status = LV_VS_BAD_ROW;
        t.bad_kind = v >> 60;
        t.bad_row = v & ((1ull << 60) - 1);
    } else if (h->dup) {
        t.status = LV_VS_DUPLICATE;
        t.bad_kind = LV_VE_KIND_FILE;
        t.bad_row = ~static_cast<uint64_t>(h->dup);
    } else if (h->bad_dir) {
        t.status = LV_VS_BAD_DIRECTORY;
        t.bad_kind = LV_VS_KIND_DIRECTORY;
        t.bad_row = ~static_cast<uint64_t>(h->bad_dir);
    } else if (n) {
        t.live = carry_scan(A.tsum, 1, A.ftiles, lane);
        if (t.live > A.out.files_cap) t.status = LV_VS_FILE_OVER;
        t.new_files = A.in.d_rec_file[n] - A.in.d_rec_file[0];
        t.deleted = A.in.d_rec_deleted[n] - A.in.d_rec_deleted[0];
        t.pointers = A.in.d_rec_pointer[n] - A.in.d_rec_pointer[0];
        t.unplaced = h->unplaced;
        t.max_file_number = h->max_number;
#pragma unroll
        for (uint32_t l = 0; l < LV_NUM_LEVELS; ++l) {
            t.level_files[l] = h->lfiles[l];
            t.level_bytes[l] = h->lbytes[l];
            t.compact_pointer[l] = h->cp[l];
        }
        const unsigned long long *lh = h->last_has;
        if (lh[0]) {
            t.comparator_off = A.in.d_edits[lh[0] - 1].comparator_off;
            t.comparator_len = A.in.d_edits[lh[0] - 1].comparator_len;
        }
        if (lh[1]) t.log_number = A.in.d_edits[lh[1] - 1].log_number;
        if (lh[2]) t.prev_log_number = A.in.d_edits[lh[2] - 1].prev_log_number;
        if (lh[3]) t.next_file_number = A.in.d_edits[lh[3] - 1].next_file_number;
        if (lh[4]) t.last_sequence = A.in.d_edits[lh[4] - 1].last_sequence;
#pragma unroll
        for (uint32_t b = 0; b < 5; ++b)
            if (lh[b]) t.has |= 1u << b;
        // MarkFileNumberUsed(log_number), then (prev_log_number)
        if (lh[1] && t.next_file_number <= t.log_number) t.next_file_number = t.log_number + 1;
        if (lh[2] && t.next_file_number <= t.prev_log_number) t.next_file_number = t.prev_log_number + 1;
    }
    if (lane == 0) {
        h->sorted = t.status ? 0 : t.live;
        *A.out.d_totals = t;
    }
}

// Kernel 5: a live row becomes a sort entry at its position among the live rows.
__global__ __launch_bounds__(kVsThreads) void vs_gather(const VsArgs A) {
    const VsHead *h = A.head;
    if (!h->sorted) return;
    const uint64_t n = h->n;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kVsThreads + threadIdx.x;
    if (!(A.in.d_rec_file[0] <= i && i < A.in.d_rec_file[n])) return;
    const uint32_t pv = A.pre[i];
    if (!(pv & 1u)) return;
    const uint64_t at = A.tsum[i / kVsTile] + (pv >> 1);
    if (at >= A.out.files_cap) return;  // (never: the status said the live rows fit)
    const lv_ve_file f = A.in.d_files[i];
    VsEnt e{};
    e.level = f.level;
    e.row = static_cast<uint32_t>(i);
    if (f.level == 0) {
        e.p[0] = f.number;
    } else {
        const uint8_t *k = A.src + f.smallest_off;
        const uint32_t ulen = f.smallest_len - 8, have = ulen < kVsPrefix ? ulen : kVsPrefix;
#pragma unroll
        for (uint32_t w = 0; w < kVsPrefix / 8; ++w) {
            uint64_t v = 0;
            if (have >= 8 * w + 8) {
                v = load_be64(k + 8 * w);
            } else {
                for (uint32_t q = 8 * w; q < have; ++q) v |= static_cast<uint64_t>(k[q]) << (56 - 8 * (q & 7u));
            }
            e.p[w] = v;
        }
        e.klen = ulen;
    }
    A.buf[1][at] = e;
}

// The version's order (version.h), a strict total order over the live files
// (a pair is live once): level ascending; level 0 by number descending; levels
// >= 1 by smallest internal key (user key ascending, tag descending), then
// number ascending.  Padding entries come after every file.
struct VsLess {
    const uint8_t *src;
    const lv_ve_file *files;
    __device__ __forceinline__ bool operator()(const VsEnt &a, const VsEnt &b) const {
        if (a.level != b.level) return a.level < b.level;
        if (a.level == kVsNone) return false;
        if (a.level == 0) return a.p[0] > b.p[0];
#pragma unroll
        for (uint32_t w = 0; w < kVsPrefix / 8; ++w)
            if (a.p[w] != b.p[w]) return a.p[w] < b.p[w];
        const lv_ve_file &fa = files[a.row], &fb = files[b.row];
        // equal prefixes.  A key no longer than the prefix is then a prefix of the other: the length decides.
        if (a.klen <= kVsPrefix || b.klen <= kVsPrefix) {
            if (a.klen != b.klen) return a.klen < b.klen;
        } else {
            const int c = cmp_bytes(src + fa.smallest_off + kVsPrefix, a.klen - kVsPrefix, src + fb.smallest_off + kVsPrefix,
                                    b.klen - kVsPrefix);
            if (c) return c < 0;
        }
        uint64_t ta, tb;  // the tags: 8 little-endian bytes behind the user key
        __builtin_memcpy(&ta, src + fa.smallest_off + a.klen, 8);
        __builtin_memcpy(&tb, src + fb.smallest_off + b.klen, 8);
        if (ta != tb) return ta > tb;
        return fa.number < fb.number;
    }
};

// Kernel 6: the sort of one tile of entries, from buffer 1 to buffer 0.
__global__ __launch_bounds__(kVsThreads) void vs_tile_sort(const VsArgs A) {
    __shared__ VsEnt s[kVsTile];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = A.head->sorted;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kVsTile;
    if (base >= n) return;
    const uint32_t cnt = static_cast<uint32_t>(n - base < kVsTile ? n - base : kVsTile);
    uint32_t m = 2;  // the network's size: the power of two that holds the tile's entries
    while (m < cnt) m <<= 1;
    for (uint32_t j = tid; j < m; j += kVsThreads) {
        VsEnt e;
        e.p[0] = e.p[1] = ~0ull;
        e.klen = e.level = e.row = e.pad = kVsNone;
        if (j < cnt) e = A.buf[1][base + j];
        s[j] = e;
    }
    __syncthreads();
    lds_bitonic_sort<kVsThreads>(s, m, tid, VsLess{A.src, A.in.d_files});
    for (uint32_t j = tid; j < cnt; j += kVsThreads) A.buf[0][base + j] = s[j];
}

// Kernel 7: one merge pass.  Runs of w = kVsTile << pass entries, in pairs.
__global__ __launch_bounds__(kVsThreads) void vs_merge(const VsArgs A, uint32_t pass) {
    __shared__ VsEnt s[kVsTile];
    __shared__ uint64_t s_split[2];
    const uint64_t n = A.head->sorted;
    const uint64_t w = static_cast<uint64_t>(kVsTile) << pass;
    const uint64_t o0 = static_cast<uint64_t>(blockIdx.x) * kVsTile;
    if (w >= n || o0 >= n) return;  // one run already, or beyond the entries
    const VsEnt *in = pass & 1u ? A.buf[1] : A.buf[0];
    VsEnt *out = pass & 1u ? A.buf[0] : A.buf[1];
    merge_tile<kVsTile, kVsThreads>(VsLess{A.src, A.in.d_files}, in, out, n, w, o0, s, s_split, threadIdx.x);
}

// Kernel 8: the rows of the version, a lane per live file in the sorted order.
__global__ __launch_bounds__(kVsThreads) void vs_emit(const VsArgs A) {
    const uint64_t n = A.head->sorted;
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kVsThreads + threadIdx.x;
    if (j >= n || j >= A.out.files_cap) return;
    uint32_t par = 0;  // the passes that ran: those whose run width is below n
    for (uint64_t w = kVsTile; w < n; w <<= 1) par ^= 1u;
    const VsEnt e = (par ? A.buf[1] : A.buf[0])[j];
    const lv_ve_file f = A.in.d_files[e.row];
    const uint32_t at = A.place[e.row];
    lv_version_file o{};
    o.number = f.number;
    if (at != kVsNone) {
        o.file_off = A.dir[at].file_off;
        o.file_cap = A.dir[at].file_cap;
    } else if (!A.dir_n) {
        o.file_cap = f.file_size;
    } else {
        o.status = LV_VERSION_FILE_UNPLACED;
    }
    o.smallest_off = f.smallest_off;
    o.largest_off = f.largest_off;
    o.smallest_len = f.smallest_len;
    o.largest_len = f.largest_len;
    o.level = f.level;
    o.reserved = e.row;
    A.out.d_files_out[j] = o;
    if (A.out.d_dir_index) A.out.d_dir_index[j] = at;
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxRecCap = 0xfffffffeull;
constexpr uint64_t kMaxRows = 1ull << 30;

constexpr uint64_t vs_blocks(uint64_t items) { return (items + lvk::kVsThreads - 1) / lvk::kVsThreads; }

void vs_carve(Carve &C, uint64_t file_cap, uint64_t deleted_cap, uint64_t files_cap, lvk::VsArgs &A) {
    A.slots = lvk::kVsTile;
    while (A.slots < 2 * (file_cap + deleted_cap)) A.slots <<= 1;
    A.ftiles = (file_cap + lvk::kVsTile - 1) / lvk::kVsTile;
    A.head = C.take<lvk::VsHead>(1);
    A.table = C.take<lvk::VsSlot>(A.slots);
    A.pre = C.take<uint32_t>(A.ftiles * lvk::kVsTile);
    A.place = C.take<uint32_t>(file_cap);
    A.tsum = C.take<uint64_t>(A.ftiles);
    A.buf[0] = C.take<lvk::VsEnt>(files_cap);
    A.buf[1] = C.take<lvk::VsEnt>(files_cap);
}

}  // namespace

extern "C" {

size_t lv_version_apply_workspace_bytes(size_t file_cap, size_t deleted_cap, size_t files_cap) {
    if (file_cap > kMaxRows || deleted_cap > kMaxRows || files_cap > LV_VERSION_MAX_FILES) return 0;
    lvk::VsArgs A{};
    Carve C{nullptr};
    vs_carve(C, file_cap, deleted_cap, files_cap, A);
    return C.at;
}

int lv_version_apply_device(const uint8_t *d_src, size_t src_bytes, const lv_ve_encode_in *in,
                            const uint64_t *d_records, const uint64_t *d_upstream_status, size_t rec_cap,
                            const lv_vs_placement *d_dir, size_t dir_n, const lv_vs_out *out, uint32_t flags,
                            void *d_workspace, size_t workspace_bytes, void *stream) {
    g_err.clear();
    if (flags) return set_err(LV_ERR_INVALID, "unknown flag bits (none are defined)");
    if (!in || !out) return set_err(LV_ERR_INVALID, "null input or output descriptor");
    if (!out->d_totals) return set_err(LV_ERR_INVALID, "null d_totals");
    if (misaligned(out->d_totals, 8)) return set_err(LV_ERR_INVALID, "d_totals must be 8-byte aligned");
    if (!d_records) return set_err(LV_ERR_INVALID, "null d_records");
    if (!d_src && src_bytes) return set_err(LV_ERR_INVALID, "null d_src");
    if (rec_cap > kMaxRecCap) return set_err(LV_ERR_INVALID, "rec_cap too large for one apply (at most 2^32 - 2)");
    if (in->file_cap > kMaxRows || in->deleted_cap > kMaxRows || in->pointer_cap > kMaxRows || dir_n > kMaxRows)
        return set_err(LV_ERR_INVALID, "row capacity or dir_n too large for one apply (at most 2^30)");
    if (out->files_cap > LV_VERSION_MAX_FILES) return set_err(LV_ERR_INVALID, "files_cap above LV_VERSION_MAX_FILES");
    if (!in->d_rec_file || !in->d_rec_deleted || !in->d_rec_pointer)
        return set_err(LV_ERR_INVALID, "null bounds array (d_rec_file / d_rec_deleted / d_rec_pointer)");
    if (misaligned(in->d_rec_file, 8) || misaligned(in->d_rec_deleted, 8) || misaligned(in->d_rec_pointer, 8))
        return set_err(LV_ERR_INVALID, "the bounds arrays must be 8-byte aligned");
    if (rec_cap && !in->d_edits) return set_err(LV_ERR_INVALID, "null d_edits");
    if ((in->file_cap && !in->d_files) || (in->deleted_cap && !in->d_deleted) || (in->pointer_cap && !in->d_pointers))
        return set_err(LV_ERR_INVALID, "null row table (d_files / d_deleted / d_pointers)");
    if (misaligned(in->d_edits, 16) || misaligned(in->d_files, 16) || misaligned(in->d_deleted, 16) ||
        misaligned(in->d_pointers, 16))
        return set_err(LV_ERR_INVALID, "d_edits and the row tables must be 16-byte aligned");
    if (dir_n && !d_dir) return set_err(LV_ERR_INVALID, "null d_dir");
    if (out->files_cap && !out->d_files_out) return set_err(LV_ERR_INVALID, "null d_files_out");
    if (misaligned(d_dir, 8) || misaligned(out->d_files_out, 8))
        return set_err(LV_ERR_INVALID, "d_dir and d_files_out must be 8-byte aligned");
    if (misaligned(out->d_dir_index, 4)) return set_err(LV_ERR_INVALID, "d_dir_index must be 4-byte aligned");
    if (!d_workspace) return set_err(LV_ERR_INVALID, "null workspace");
    if (misaligned(d_workspace, 16)) return set_err(LV_ERR_INVALID, "workspace must be 16-byte aligned");
    lvk::VsArgs A{};
    Carve C{static_cast<uint8_t *>(d_workspace)};
    vs_carve(C, in->file_cap, in->deleted_cap, out->files_cap, A);
    if (workspace_bytes < C.at) return set_err(LV_ERR_INVALID, "workspace too small");
    const struct { const void *p; uint64_t bytes; } inputs[] = {
        {d_src, src_bytes},
        {in->d_edits, static_cast<uint64_t>(rec_cap) * sizeof(lv_ve_edit)},
        {in->d_files, static_cast<uint64_t>(in->file_cap) * sizeof(lv_ve_file)},
        {in->d_deleted, static_cast<uint64_t>(in->deleted_cap) * sizeof(lv_ve_deleted)},
        {in->d_pointers, static_cast<uint64_t>(in->pointer_cap) * sizeof(lv_ve_pointer)},
        {in->d_rec_file, (static_cast<uint64_t>(rec_cap) + 1) * 8},
        {in->d_rec_deleted, (static_cast<uint64_t>(rec_cap) + 1) * 8},
        {in->d_rec_pointer, (static_cast<uint64_t>(rec_cap) + 1) * 8},
        {d_dir, static_cast<uint64_t>(dir_n) * sizeof(lv_vs_placement)},
    };
    for (const auto &i : inputs)
        if (overlaps(out->d_files_out, static_cast<uint64_t>(out->files_cap) * sizeof(lv_version_file), i.p, i.bytes) ||
            (out->d_dir_index && overlaps(out->d_dir_index, static_cast<uint64_t>(out->files_cap) * 4, i.p, i.bytes)))
            return set_err(LV_ERR_INVALID, "d_files_out or d_dir_index overlaps an input");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    A.src = d_src;
    A.src_bytes = src_bytes;
    A.in = *in;
    A.records = d_records;
    A.upstream = d_upstream_status;
    A.rec_cap = rec_cap;
    A.dir = d_dir;
    A.dir_n = dir_n;
    A.out = *out;
    // the items: each kind in whole workgroups
    A.seg[0] = 0;
    A.seg[1] = A.seg[0] + vs_blocks(in->pointer_cap) * lvk::kVsThreads;
    A.seg[2] = A.seg[1] + vs_blocks(in->deleted_cap) * lvk::kVsThreads;
    A.seg[3] = A.seg[2] + vs_blocks(in->file_cap) * lvk::kVsThreads;
    A.seg[4] = A.seg[3] + vs_blocks(dir_n) * lvk::kVsThreads;

    const dim3 b(lvk::kVsThreads);
    // a lane per record, at least one workgroup: its first thread judges UPSTREAM and REC_OVER
    const uint32_t rec_grid = static_cast<uint32_t>(rec_cap ? vs_blocks(rec_cap) : 1);
    const uint32_t item_grid = static_cast<uint32_t>(A.seg[4] / lvk::kVsThreads);
    const uint32_t file_grid = static_cast<uint32_t>(vs_blocks(in->file_cap));
    const uint32_t sort_tiles = static_cast<uint32_t>((static_cast<uint64_t>(out->files_cap) + lvk::kVsTile - 1) / lvk::kVsTile);
    hipLaunchKernelGGL(lvk::vs_clear, dim3(static_cast<uint32_t>(vs_blocks(A.slots))), b, 0, s, A);
    hipLaunchKernelGGL(lvk::vs_bounds, dim3(rec_grid), b, 0, s, A);
    if (item_grid) hipLaunchKernelGGL(lvk::vs_rows, dim3(item_grid), b, 0, s, A);
    if (A.ftiles) hipLaunchKernelGGL(lvk::vs_live, dim3(static_cast<uint32_t>(A.ftiles)), b, 0, s, A);
    hipLaunchKernelGGL(lvk::vs_carry, dim3(1), dim3(64), 0, s, A);
    if (sort_tiles) {
        if (file_grid) hipLaunchKernelGGL(lvk::vs_gather, dim3(file_grid), b, 0, s, A);
        hipLaunchKernelGGL(lvk::vs_tile_sort, dim3(sort_tiles), b, 0, s, A);
        for (uint32_t pass = 0; (static_cast<uint64_t>(lvk::kVsTile) << pass) < out->files_cap; ++pass)
            hipLaunchKernelGGL(lvk::vs_merge, dim3(sort_tiles), b, 0, s, A, pass);
        hipLaunchKernelGGL(lvk::vs_emit, dim3(static_cast<uint32_t>(vs_blocks(out->files_cap))), b, 0, s, A);
    }
    g_kernel = "vs_clear+vs_bounds+vs_rows+vs_live+vs_carry+vs_gather+vs_tile_sort+vs_merge+vs_emit";
    return check_launch();
}

}  // extern "C"
