// Device-resident WAL Reader (the read side of SURVEY 8f row 1 with the log
// and the records in HBM): lv_wal_decode_device.  It takes a log and the
// arrays lv_wal_scan_device made of it and replays Reader::read_record with
// initial_offset == 0 (log_reader.rs:120-364, as wal_host.cc restates it):
// the stored checksums are compared, FIRST/MIDDLE/LAST fragments are joined
// into logical records, the drop rules are applied and reported.  The Reader's
// sequential state machine is restated as scans (below), so nothing is
// sequential in the log's length and nothing comes back to the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/wal.h"
#include "lv_internal.h"
#include "lvh.h"
#include "lvk/sort.h"
#include "lvk/wal.h"

namespace lvk {

constexpr uint32_t kDecThreads = 256;
constexpr uint32_t kDecPer = 4;                            // entries per thread
constexpr uint32_t kDecTile = kDecThreads * kDecPer;       // entries per scan tile
constexpr uint64_t kDecNone = ~0ull;

// What a scan entry is to the Reader.  SKIP: never reached (after its block's
// first kill) or not an entry.  The BAD_* are the kills (BadRecord events);
// EOF is a bad length in a short final block (silent, log_reader.rs:318-323).
// The Reader hands a physical record's type byte on in the same integer that
// carries its own Eof (5) and BadRecord (6) codes, so read_record takes a
// well-formed record of type 5 for the end of the file -- STOP: it returns
// "no more records", silently, and nothing after it is read -- and one of
// type 6 for a bad record (BAD_ZERO's event without the kill: the rest of the
// block is still read).  lv_wal_reader and the oracle do the same.
enum : uint32_t {
    kEvSkip = 0,
    kEvFull = 1,
    kEvFirst = 2,
    kEvMiddle = 3,
    kEvLast = 4,
    kEvType0 = 5,
    kEvUnknown = 6,
    kEvBadZero = 7,
    kEvBadLen = 8,
    kEvBadCrc = 9,
    kEvEof = 10,
    kEvStop = 11,
};
// An event word: code | x << 8, x = the payload length, or for BAD_LEN /
// BAD_CRC the bytes the kill reports (header to block end, <= 32768).

// The Reader's state between two entries, and a composite of events acting
// on it.  Every event either sets the state whatever it was (kConst: FULL,
// FIRST, LAST, a kill, a bad type) or adds to the open record's size if there
// is one (MIDDLE; SKIP adds 0), so a run of events is "constant state" or
// "add k": closed under composition, associative.
// A STOP is constant too, and absorbing: no later event changes it.
constexpr uint32_t kOpConst = 1, kOpIn = 2, kOpStop = 4;
struct DecOp {
    uint32_t flags;  // kOpConst | kOpIn (in_fragmented_record; const only)
    uint32_t pad;
    uint64_t size;   // const: scratch.len(); add: k
    uint64_t start;  // const, in: prospective_record_offset
};

__device__ __forceinline__ DecOp dec_ident() { return DecOp{0u, 0u, 0ull, 0ull}; }
__device__ __forceinline__ DecOp dec_closed() { return DecOp{kOpConst, 0u, 0ull, 0ull}; }

// a, then b
__device__ __forceinline__ DecOp dec_compose(const DecOp &a, const DecOp &b) {
    if (a.flags & kOpStop) return a;
    if (b.flags & kOpConst) return b;
    DecOp r = a;
    if (!(a.flags & kOpConst) || (a.flags & kOpIn)) r.size += b.size;
    return r;
}

__device__ __forceinline__ DecOp dec_event_op(uint32_t code, uint32_t x, uint64_t hdr) {
    if (code == kEvSkip) return dec_ident();
    if (code == kEvMiddle) return DecOp{0u, 0u, x, 0ull};
    if (code == kEvFirst) return DecOp{kOpConst | kOpIn, 0u, x, hdr};
    if (code == kEvStop) return DecOp{kOpConst | kOpStop, 0u, 0ull, 0ull};
    return dec_closed();
}

struct DecSum {
    uint64_t recs, pay, reps, drop;
};
__device__ __forceinline__ DecSum dec_add(const DecSum &a, const DecSum &b) {
    return DecSum{a.recs + b.recs, a.pay + b.pay, a.reps + b.reps, a.drop + b.drop};
}

// What one reached entry does (wal_host.cc:259-308): the state after it, the
// record it emits, its reports in the Reader's order.
struct DecVal {
    uint32_t emit, nrep;
    uint64_t emit_len, rec_log;
    uint64_t rb[2];
    uint32_t rr[2];
};

__device__ __forceinline__ void dec_report(DecVal *v, uint64_t bytes, uint32_t reason) {
    v->rb[v->nrep] = bytes;
    v->rr[v->nrep] = reason;
    ++v->nrep;
}

__device__ __forceinline__ void dec_step(uint32_t code, uint32_t x, uint64_t hdr, DecOp *s, DecVal *v) {
    v->emit = 0;
    v->nrep = 0;
    v->emit_len = 0;
    v->rec_log = 0;
    v->rb[0] = v->rb[1] = 0;
    v->rr[0] = v->rr[1] = 0;
    if (s->flags & kOpStop) return;  // the Reader has returned its end of file
    const bool in = (s->flags & kOpIn) != 0;
    const uint64_t size = in ? s->size : 0ull;
    switch (code) {
        case kEvSkip:
            return;
        case kEvFull:
            if (in) dec_report(v, size, LV_WAL_DROP_NO_END_1);
            v->emit = 1;
            v->emit_len = x;
            v->rec_log = hdr;
            break;
        case kEvFirst:
            if (in) dec_report(v, size, LV_WAL_DROP_NO_END_2);
            *s = DecOp{kOpConst | kOpIn, 0u, x, hdr};
            return;
        case kEvMiddle:
            if (!in)
                dec_report(v, x, LV_WAL_DROP_NO_START_1);
            else
                s->size += x;
            return;
        case kEvLast:
            if (!in) {
                dec_report(v, x, LV_WAL_DROP_NO_START_2);
            } else {
                v->emit = 1;
                v->emit_len = size + x;
                v->rec_log = s->start;
            }
            break;
        case kEvType0:
            dec_report(v, x + size, LV_WAL_DROP_UNEXPECTED_TYPE);
            break;
        case kEvUnknown:
            dec_report(v, x + size, LV_WAL_DROP_UNKNOWN_TYPE);
            break;
        case kEvBadLen:
            dec_report(v, x, LV_WAL_DROP_BAD_LENGTH);
            if (in) dec_report(v, size, LV_WAL_DROP_MID_RECORD);
            break;
        case kEvBadCrc:
            dec_report(v, x, LV_WAL_DROP_CHECKSUM);
            if (in) dec_report(v, size, LV_WAL_DROP_MID_RECORD);
            break;
        case kEvBadZero:
            if (in) dec_report(v, size, LV_WAL_DROP_MID_RECORD);
            break;
        case kEvStop:
            *s = DecOp{kOpConst | kOpStop, 0u, 0ull, 0ull};
            return;
        default:  // kEvEof: the Reader stops, an open record is dropped silently
            break;
    }
    *s = dec_closed();
}

__device__ __forceinline__ void dec_accumulate(DecSum *a, const DecVal &v) {
    a->recs += v.emit;
    a->pay += v.emit_len;
    a->reps += v.nrep;
    a->drop += v.rb[0] + v.rb[1];
}

// The workgroup scan over LDS (Hillis-Steele, kDecThreads values of T in
// lds): each thread gets the composite of the values of the threads before
// it, the identity where there are none, and *total the composite of all;
// then(a, b) is "a, then b".  With kBack the threads are taken in reverse: a
// thread gets the composite of those after it, the last thread's value first.
// The identity of every scan here is the zero value T{} (dec_ident(), no sums,
// no event); handed in as an argument it cost wal_dec_tiles and wal_dec_apply
// some 30 instructions each.  It ends with a barrier, so lds can be reused at
// once.  The tiles are few against the copy's bytes, so the two barriers per
// step do not show.
template <bool kBack, class T, class F>
__device__ __forceinline__ T dec_scan(T v, T *lds, T *total, F then) {
    const uint32_t t = kBack ? kDecThreads - 1 - threadIdx.x : threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kDecThreads; d <<= 1) {
        T o{};
        if (t >= d) o = lds[t - d];
        __syncthreads();
        if (t >= d) {
            v = then(o, v);
            lds[t] = v;
        }
        __syncthreads();
    }
    const T ex = t ? lds[t - 1] : T{};
    *total = lds[kDecThreads - 1];
    __syncthreads();
    return ex;
}
// Under this, backward, a thread gets the first non-zero value of the threads
// after it (0: none) and *total the first of the whole workgroup: the nearer
// value is the later one.
__device__ __forceinline__ uint32_t dec_nearer(uint32_t farther, uint32_t nearer) { return nearer ? nearer : farther; }

// What a tile of kDecTile entries does, as far as it can be said without the
// state it starts in.  The incoming state matters only up to the tile's first
// constant event: the MIDDLEs before it (pre_n of them, pre_k bytes) and that
// event itself (first_*); `sums` holds everything after it.
struct DecTileSum {
    DecOp op;
    DecSum sums;
    uint64_t pre_n, pre_k;
    uint64_t first_hdr;
    uint32_t first_code, first_x;
};
// What the tile scan hands each tile: the state it starts in, the records,
// payload bytes and reports before it, the first constant event after it.
struct DecTileIn {
    DecOp state;
    uint64_t recs, pay, reps;
    uint32_t next_code, pad;
};
struct DecHead {
    uint64_t n, status;
};

struct DecArgs {
    const uint8_t *log;
    uint64_t bytes;
    const uint64_t *hdr_off;
    const uint32_t *crc;  // null: no checksum
    const uint32_t *info;
    const uint64_t *count;
    uint64_t cap;      // scan_cap
    uint64_t nb;       // entries of each block array (cap + 1)
    uint64_t nblocks;  // blocks of the log
    lv_wal_decode_out out;
    // workspace
    DecHead *head;
    uint32_t *ev;
    uint64_t *fpos;  // output position of each live fragment, kDecNone otherwise
    uint32_t *fkill, *bfirst, *bend;  // per block: first kill, first entry, end entry
    DecTileSum *tsum;
    DecTileIn *tin;
};

__device__ __forceinline__ uint64_t dec_count(const DecArgs &A) {
    const uint64_t n = *A.count;
    return n > A.cap ? 0ull : n;  // the scan overflowed: it wrote no entries
}

// Kernel 0: "none" (2^32 - 1) in every block's first kill, first entry and end
// entry.  A kernel, not a memset: a memset node inside a longer captured graph does not
// replay reliably (DESIGN, mt_init), and a chain of kernels does.
__global__ __launch_bounds__(kDecThreads) void wal_dec_init(uint32_t *p, uint64_t n) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kDecThreads;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kDecThreads + threadIdx.x; i < n; i += stride) p[i] = ~0u;
}

// Kernel 1: every entry's event, each block's first kill and entry range.
__global__ __launch_bounds__(kDecThreads) void wal_dec_classify(const DecArgs A) {
    const uint64_t n = dec_count(A);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kDecThreads;
    const uint64_t eof_blk = A.bytes % kWalBlock ? A.bytes / kWalBlock : kDecNone;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kDecThreads + threadIdx.x; i < n; i += stride) {
        const uint64_t hdr = A.hdr_off[i];
        const uint32_t info = A.info[i];
        const uint32_t type = info & 0xffu, status = (info >> 8) & 0xffu, len = info >> 16;
        const uint64_t blk = hdr / kWalBlock;
        uint32_t code = kEvSkip, x = 0;
        bool kill = false;
        if (blk < A.nb && hdr + kWalHeader <= A.bytes) {
            const uint64_t end = (blk + 1) * kWalBlock < A.bytes ? (blk + 1) * kWalBlock : A.bytes;
            const uint32_t left = static_cast<uint32_t>(end - hdr);
            if (status == LV_WAL_REC_BAD_LENGTH) {  // log_reader.rs:312-324
                code = blk == eof_blk ? kEvEof : kEvBadLen;
                x = left;
                kill = true;
            } else if (status == LV_WAL_REC_ZERO) {  // log_reader.rs:326-331
                code = kEvBadZero;
                kill = true;
            } else if (status == LV_WAL_REC_OK && kWalHeader + len <= left) {
                bool ok = true;
                if (A.crc)  // log_reader.rs:335-342
                    ok = stored_crc(A.log + hdr) == A.crc[i];
                if (!ok) {
                    code = kEvBadCrc;
                    x = left;
                    kill = true;
                } else {
                    code = type == 0 ? kEvType0 : (type <= 4 ? type : kEvUnknown);
                    if (type == 5) code = kEvStop;     // the Reader's Eof code
                    if (type == 6) code = kEvBadZero;  // its BadRecord code: no kill
                    x = len;
                }
            }
            if (code != kEvSkip) {
                if (kill) atomicMin(&A.fkill[blk], static_cast<uint32_t>(i));
                if (i == 0 || A.hdr_off[i - 1] / kWalBlock != blk) A.bfirst[blk] = static_cast<uint32_t>(i);
                if (i + 1 == n || A.hdr_off[i + 1] / kWalBlock != blk) A.bend[blk] = static_cast<uint32_t>(i + 1);
            }
        }
        A.ev[i] = code | (x << 8);
    }
}

// Entry i as the Reader meets it: skipped when past its block's first kill.
__device__ __forceinline__ void dec_load(const DecArgs &A, uint64_t i, uint64_t n, uint32_t *code, uint32_t *x,
                                         uint64_t *hdr) {
    *code = kEvSkip;
    *x = 0;
    *hdr = 0;
    if (i >= n) return;
    const uint32_t e = A.ev[i];
    if ((e & 0xffu) == kEvSkip) return;
    const uint64_t h = A.hdr_off[i];
    if (i > A.fkill[h / kWalBlock]) return;
    *code = e & 0xffu;
    *x = e >> 8;
    *hdr = h;
}

// Kernel 2: each tile's summary.
__global__ __launch_bounds__(kDecThreads) void wal_dec_reduce(const DecArgs A) {
    __shared__ DecOp s_op[kDecThreads];
    __shared__ unsigned long long s_acc[6];
    __shared__ uint64_t s_first_hdr;
    __shared__ uint32_t s_first_code, s_first_x;
    const uint32_t t = threadIdx.x;
    const uint64_t n = dec_count(A);
    const uint64_t ntiles = (n + kDecTile - 1) / kDecTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (t < 6) s_acc[t] = 0;
        if (t == 0) {
            s_first_code = 0;
            s_first_x = 0;
            s_first_hdr = 0;
        }
        uint32_t code[kDecPer], x[kDecPer];
        uint64_t hdr[kDecPer];
        DecOp loc = dec_ident();
#pragma unroll
        for (uint32_t j = 0; j < kDecPer; ++j) {
            dec_load(A, tile * kDecTile + t * kDecPer + j, n, &code[j], &x[j], &hdr[j]);
            loc = dec_compose(loc, dec_event_op(code[j], x[j], hdr[j]));
        }
        DecOp total;  // (the scan's first barrier orders the zeroing above)
        DecOp s = dec_scan<false>(loc, s_op, &total, dec_compose);
        bool known = (s.flags & kOpConst) != 0;
        DecSum sum{0, 0, 0, 0};
        uint64_t pre_n = 0, pre_k = 0;
#pragma unroll
        for (uint32_t j = 0; j < kDecPer; ++j) {
            if (code[j] == kEvSkip) continue;
            DecVal v;
            if (!known) {
                if (code[j] == kEvMiddle) {
                    ++pre_n;
                    pre_k += x[j];
                    continue;
                }
                // the tile's first constant event: its values wait for the
                // tile scan, the state after it does not
                s_first_code = code[j];
                s_first_x = x[j];
                s_first_hdr = hdr[j];
                s = dec_closed();
                dec_step(code[j], x[j], hdr[j], &s, &v);
                known = true;
                continue;
            }
            dec_step(code[j], x[j], hdr[j], &s, &v);
            dec_accumulate(&sum, v);
        }
        if (sum.recs) atomicAdd(&s_acc[0], static_cast<unsigned long long>(sum.recs));
        if (sum.pay) atomicAdd(&s_acc[1], static_cast<unsigned long long>(sum.pay));
        if (sum.reps) atomicAdd(&s_acc[2], static_cast<unsigned long long>(sum.reps));
        if (sum.drop) atomicAdd(&s_acc[3], static_cast<unsigned long long>(sum.drop));
        if (pre_n) atomicAdd(&s_acc[4], static_cast<unsigned long long>(pre_n));
        if (pre_k) atomicAdd(&s_acc[5], static_cast<unsigned long long>(pre_k));
        __syncthreads();
        if (t == 0) {
            DecTileSum ts;
            ts.op = total;
            ts.sums = DecSum{s_acc[0], s_acc[1], s_acc[2], s_acc[3]};
            ts.pre_n = s_acc[4];
            ts.pre_k = s_acc[5];
            ts.first_hdr = s_first_hdr;
            ts.first_code = s_first_code;
            ts.first_x = s_first_x;
            A.tsum[tile] = ts;
        }
        __syncthreads();
    }
}

// Kernel 3 (one workgroup): the scan of the tile summaries, the totals and
// the status.
__global__ __launch_bounds__(kDecThreads) void wal_dec_tiles(const DecArgs A) {
    __shared__ DecOp s_op[kDecThreads];
    __shared__ DecSum s_sum[kDecThreads];
    __shared__ uint32_t s_code[kDecThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t n = dec_count(A);
    const uint64_t ntiles = (n + kDecTile - 1) / kDecTile;
    DecOp carry = dec_closed();
    DecSum csum{0, 0, 0, 0};
    for (uint64_t base = 0; base < ntiles; base += kDecThreads) {
        const uint64_t tile = base + t;
        DecTileSum ts{};
        if (tile < ntiles) ts = A.tsum[tile];
        DecOp total;
        const DecOp ex = dec_scan<false>(ts.op, s_op, &total, dec_compose);
        DecOp st = dec_compose(carry, ex);  // the state the tile starts in
        const DecOp st_in = st;
        DecSum v = ts.sums;
        if (st.flags & kOpStop) {  // nothing of this tile is read
            v = DecSum{0, 0, 0, 0};
            ts.first_code = 0;
        } else if (st.flags & kOpIn) {
            st.size += ts.pre_k;
        } else {  // each MIDDLE with no start reports its own length
            v.reps += ts.pre_n;
            v.drop += ts.pre_k;
        }
        if (ts.first_code) {
            DecVal fv;
            dec_step(ts.first_code, ts.first_x, ts.first_hdr, &st, &fv);
            dec_accumulate(&v, fv);
        }
        DecSum vtotal;
        const DecSum vex = dec_scan<false>(v, s_sum, &vtotal, dec_add);
        if (tile < ntiles) {
            DecTileIn ti;
            ti.state = st_in;
            ti.recs = csum.recs + vex.recs;
            ti.pay = csum.pay + vex.pay;
            ti.reps = csum.reps + vex.reps;
            ti.next_code = 0;
            ti.pad = 0;
            A.tin[tile] = ti;
        }
        carry = dec_compose(carry, total);
        csum = dec_add(csum, vtotal);
    }
    // the first constant event after each tile (whether an open record closes)
    uint32_t next = 0;
    const uint64_t chunks = (ntiles + kDecThreads - 1) / kDecThreads;
    for (uint64_t c = chunks; c-- > 0;) {
        const uint64_t tile = c * kDecThreads + t;
        const uint32_t mine = tile < ntiles ? A.tsum[tile].first_code : 0u;
        uint32_t all;
        const uint32_t ex = dec_scan<true>(mine, s_code, &all, dec_nearer);
        if (tile < ntiles) A.tin[tile].next_code = ex ? ex : next;
        if (all) next = all;
    }
    if (t == 0) {
        uint64_t status = 0;
        if (*A.count > A.cap) status |= LV_WAL_DECODE_SCAN_OVER;
        if (csum.recs > A.out.rec_cap) status |= LV_WAL_DECODE_REC_OVER;
        if (csum.pay > A.out.payload_cap) status |= LV_WAL_DECODE_PAYLOAD_OVER;
        if (A.out.d_rep_bytes && csum.reps > A.out.rep_cap) status |= LV_WAL_DECODE_REPORT_OVER;
        lv_wal_decode_totals tot;
        tot.records = csum.recs;
        tot.payload_bytes = csum.pay;
        tot.reports = csum.reps;
        tot.dropped_bytes = csum.drop;
        tot.status = status;
        *A.out.d_totals = tot;
        A.head->n = n;
        A.head->status = status;
    }
}

// Kernel 4: the apply pass.  Each entry's incoming state, its records and
// reports at their prefix-sum positions, each live fragment's output position.
__global__ __launch_bounds__(kDecThreads) void wal_dec_apply(const DecArgs A) {
    __shared__ DecOp s_op[kDecThreads];
    __shared__ DecSum s_sum[kDecThreads];
    __shared__ uint32_t s_code[kDecThreads];
    if (A.head->status) return;  // only the totals are written
    const uint32_t t = threadIdx.x;
    const uint64_t n = A.head->n;
    const uint64_t ntiles = (n + kDecTile - 1) / kDecTile;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const DecTileIn ti = A.tin[tile];
        uint32_t code[kDecPer], x[kDecPer];
        uint64_t hdr[kDecPer];
        DecOp loc = dec_ident();
        uint32_t cfirst = 0;  // this thread's first constant event
#pragma unroll
        for (uint32_t j = 0; j < kDecPer; ++j) {
            dec_load(A, tile * kDecTile + t * kDecPer + j, n, &code[j], &x[j], &hdr[j]);
            loc = dec_compose(loc, dec_event_op(code[j], x[j], hdr[j]));
            if (!cfirst && code[j] != kEvSkip && code[j] != kEvMiddle) cfirst = code[j];
        }
        DecOp total;
        DecOp s = dec_compose(ti.state, dec_scan<false>(loc, s_op, &total, dec_compose));
        DecVal v[kDecPer];
        uint64_t before[kDecPer];  // the open record's bytes before the entry, kDecNone: no open record
        DecSum sum{0, 0, 0, 0};
#pragma unroll
        for (uint32_t j = 0; j < kDecPer; ++j) {
            before[j] = (s.flags & kOpIn) ? s.size : kDecNone;
            if (s.flags & kOpStop) code[j] = kEvSkip;
            dec_step(code[j], x[j], hdr[j], &s, &v[j]);
            dec_accumulate(&sum, v[j]);
        }
        DecSum stotal;
        const DecSum ex = dec_scan<false>(sum, s_sum, &stotal, dec_add);
        uint32_t all;
        uint32_t next = dec_scan<true>(cfirst, s_code, &all, dec_nearer);
        if (!next) next = ti.next_code;
        uint32_t nx[kDecPer];
#pragma unroll
        for (int j = kDecPer - 1; j >= 0; --j) {
            nx[j] = next;
            if (code[j] != kEvSkip && code[j] != kEvMiddle) next = code[j];
        }
        uint64_t R = ti.recs + ex.recs, P = ti.pay + ex.pay, Q = ti.reps + ex.reps;
#pragma unroll
        for (uint32_t j = 0; j < kDecPer; ++j) {
            const uint64_t i = tile * kDecTile + t * kDecPer + j;
            if (i >= n) break;
            for (uint32_t r = 0; r < v[j].nrep; ++r, ++Q) {
                if (!A.out.d_rep_bytes || Q >= A.out.rep_cap) continue;  // (the status said it fits)
                A.out.d_rep_bytes[Q] = v[j].rb[r];
                A.out.d_rep_reason[Q] = v[j].rr[r];
                A.out.d_rep_log_off[Q] = hdr[j];
            }
            // a fragment is live when its record is emitted: a FULL, a LAST
            // that closes an open record, and a FIRST / MIDDLE of an open
            // record whose next constant event is a LAST
            uint64_t fp = kDecNone;
            if (code[j] == kEvFull)
                fp = P;
            else if (code[j] == kEvFirst && nx[j] == kEvLast)
                fp = P;
            else if (code[j] == kEvMiddle && before[j] != kDecNone && nx[j] == kEvLast)
                fp = P + before[j];
            else if (code[j] == kEvLast && before[j] != kDecNone)
                fp = P + before[j];
            A.fpos[i] = fp;
            if (v[j].emit) {
                if (R < A.out.rec_cap) {
                    A.out.d_rec_off[R] = P;
                    A.out.d_rec_len[R] = v[j].emit_len;
                    A.out.d_rec_log_off[R] = v[j].rec_log;
                }
                ++R;
                P += v[j].emit_len;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// wal_unframe_kernel: wal_frame_kernel the other way round.  The live
// fragments of consecutive records are adjacent in the output (only headers
// and trailers are squeezed out), so one log block's live fragments map to one
// contiguous output span and the blocks' spans tile d_payload[0, payload_bytes).
// A workgroup takes one log block at a time: a prefix sum of its live
// fragments' lengths gives each fragment's position in the span (16 bits, in
// LDS, with its position in the block), and then the work follows the output
// bytes -- the span is cut into the 16-byte granules of its own address
// alignment, one per lane per step; a lane finds the fragment under its
// granule with a binary search in LDS.  A granule wholly inside one fragment
// is one unaligned 16-B load and one aligned 16-B store; one that crosses
// fragments is composed byte by byte and stored whole; the span's ragged ends
// are stored byte by byte, so two workgroups never store the same byte.
__global__ __launch_bounds__(kDecThreads) void wal_unframe_kernel(const DecArgs A) {
    __shared__ uint16_t s_out[kWalMaxFrags + 1];
    __shared__ uint16_t s_src[kWalMaxFrags];
    __shared__ uint32_t s_wt[kDecThreads / 64];
    __shared__ uint64_t s_span;
    if (A.head->status) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t n = A.head->n;
    const uint64_t nblocks = A.nblocks < A.nb ? A.nblocks : A.nb;
    for (uint64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const uint32_t e0 = A.bfirst[blk], e1 = A.bend[blk];
        uint32_t cnt = 0;
        if (e0 != ~0u && e1 != ~0u && e1 > e0 && e1 <= n) cnt = e1 - e0 < kWalMaxFrags ? e1 - e0 : kWalMaxFrags;
        const uint64_t start = blk * kWalBlock;
        __syncthreads();  // the previous block's searches are done
        uint32_t carry = 0;
        for (uint32_t k0 = 0; k0 < cnt; k0 += kDecThreads) {  // block-uniform
            const uint32_t k = k0 + tid;
            uint32_t ll = 0;
            uint64_t fp = kDecNone;
            if (k < cnt) {
                const uint64_t i = static_cast<uint64_t>(e0) + k;
                fp = A.fpos[i];
                if (fp != kDecNone) ll = (A.ev[i] >> 8) & 0xffffu;
                s_src[k] = static_cast<uint16_t>(A.hdr_off[i] - start + kWalHeader);
            }
            const uint32_t inc = wg_incl_scan<kDecThreads / 64>(ll, s_wt);
            const uint32_t o = carry + inc - ll;
            if (k < cnt) {
                s_out[k] = static_cast<uint16_t>(o);
                if (fp != kDecNone && o == 0) s_span = fp;  // (every writer has the span's start)
            }
            uint32_t tot = 0;
#pragma unroll
            for (uint32_t w = 0; w < kDecThreads / 64; ++w) tot += s_wt[w];
            carry += tot;
            __syncthreads();  // s_wt is rewritten by the next chunk
        }
        if (tid == 0) s_out[cnt] = static_cast<uint16_t>(carry);
        __syncthreads();
        const uint32_t total = carry;  // bytes of this block's span (<= 32761)
        if (total == 0) continue;      // block-uniform
        const uint64_t span = s_span;
        if (span > A.out.payload_cap || total > A.out.payload_cap - span) continue;  // (never: the status said it fits)
        uint8_t *const dst = A.out.d_payload + span;
        const uint8_t *const src = A.log + start;
        const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst) & 15u);
        uint32_t head = (16u - mis) & 15u;  // bytes before the span's first aligned granule
        if (head > total) head = total;
        const uint32_t ngran = (head ? 1u : 0u) + (total - head + 15u) / 16u;
        for (uint32_t g = tid; g < ngran; g += kDecThreads) {
            uint32_t lo, hi;
            if (head && g == 0) {
                lo = 0;
                hi = head;
            } else {
                lo = head + (g - (head ? 1u : 0u)) * 16u;
                hi = lo + 16u < total ? lo + 16u : total;
            }
            // the fragment under lo: the last one with s_out <= lo (s_out[0] = 0)
            uint32_t f = count_le(s_out, cnt, lo) - 1;
            if (hi - lo == 16u && lo + 16u <= s_out[f + 1]) {
                u32x4 v;
                __builtin_memcpy(&v, src + s_src[f] + (lo - s_out[f]), 16);
                *reinterpret_cast<u32x4 *>(dst + lo) = v;
                continue;
            }
            uint64_t wlo = 0, whi = 0;
            for (uint32_t p = lo; p < hi; ++p) {
                while (s_out[f + 1] <= p) ++f;  // (p < total = s_out[cnt])
                const uint64_t byte = src[s_src[f] + (p - s_out[f])];
                const uint32_t q = p - lo;
                if (q < 8)
                    wlo |= byte << (8 * q);
                else
                    whi |= byte << (8 * (q - 8));
            }
            granule_store(dst + lo, wlo, whi, (1u << (hi - lo)) - 1u);  // whole: dst + lo is 16-B aligned
        }
    }
}

}  // namespace lvk

using namespace lvh;

namespace {

constexpr uint64_t kMaxScanCap = 0xfffffffeull;  // entry indices are 32-bit, ~0 means none

// The workspace for scan_cap = cap; returns the scan tiles.
uint64_t dec_carve(Carve &C, uint64_t cap, lvk::DecArgs &A) {
    const uint64_t tiles = (cap + lvk::kDecTile - 1) / lvk::kDecTile;
    A.nb = cap + 1;
    A.head = C.take<lvk::DecHead>(1);
    A.ev = C.take<uint32_t>(cap);
    A.fpos = C.take<uint64_t>(cap);
    A.fkill = C.take<uint32_t>(3 * A.nb);  // one region, set by one launch: fkill, bfirst, bend
    A.bfirst = A.fkill ? A.fkill + A.nb : nullptr;
    A.bend = A.fkill ? A.bfirst + A.nb : nullptr;
    A.tsum = C.take<lvk::DecTileSum>(tiles);
    A.tin = C.take<lvk::DecTileIn>(tiles);
    return tiles;
}

}  // namespace

// wal_dec_classify: a workgroup takes kDecThreads scan entries a trip.
uint64_t lvgpu_internal::wal_classify_grid(uint64_t scan_cap, uint64_t cus, uint64_t *per_trip) {
    if (per_trip) *per_trip = lvk::kDecThreads;
    return std::min<uint64_t>((scan_cap + lvk::kDecThreads - 1) / lvk::kDecThreads, 16 * cus);
}
// wal_dec_reduce / wal_dec_apply: a workgroup takes a tile of kDecTile entries a trip.
uint64_t lvgpu_internal::wal_tile_grid(uint64_t scan_cap, uint64_t cus, uint64_t *per_trip) {
    if (per_trip) *per_trip = lvk::kDecTile;
    return std::min<uint64_t>((scan_cap + lvk::kDecTile - 1) / lvk::kDecTile, 8 * cus);
}
// wal_unframe_kernel: a workgroup takes one log block a trip (blocks = min(the log's, scan_cap + 1)).
uint64_t lvgpu_internal::wal_unframe_grid(uint64_t blocks, uint64_t cus, uint64_t *per_trip) {
    if (per_trip) *per_trip = 1;
    return std::min<uint64_t>(blocks, 8 * cus);
}
// wal_dec_tiles scans kDecThreads tile summaries a round.
uint64_t lvgpu_internal::wal_dec_tiles_round() { return static_cast<uint64_t>(lvk::kDecThreads) * lvk::kDecTile; }

extern "C" {

size_t lv_wal_decode_workspace_bytes(size_t scan_cap) {
    lvk::DecArgs A{};
    Carve C{nullptr};
    dec_carve(C, scan_cap, A);
    return C.at;
}

int lv_wal_decode_device(const uint8_t *d_log, size_t bytes, const uint64_t *d_hdr_off, const uint32_t *d_crc,
                         const uint32_t *d_info, const uint64_t *d_count, size_t scan_cap,
                         const lv_wal_decode_out *out, uint32_t flags, void *d_workspace, size_t workspace_bytes,
                         void *stream) {
    g_err.clear();
    if (flags & ~static_cast<uint32_t>(LV_WAL_DECODE_NO_CHECKSUM)) return set_err(LV_ERR_INVALID, "unknown flag bits");
    const bool checksum = !(flags & LV_WAL_DECODE_NO_CHECKSUM);
    if (!out) return set_err(LV_ERR_INVALID, "null output descriptor");
    if (!out->d_totals) return set_err(LV_ERR_INVALID, "null d_totals");
    if (misaligned(out->d_totals, 8)) return set_err(LV_ERR_INVALID, "d_totals must be 8-byte aligned");
    if (!d_count) return set_err(LV_ERR_INVALID, "null count pointer");
    if (!d_log && bytes) return set_err(LV_ERR_INVALID, "null log pointer");
    if (scan_cap && (!d_hdr_off || !d_info)) return set_err(LV_ERR_INVALID, "null scan array");
    if (scan_cap && checksum && !d_crc) return set_err(LV_ERR_INVALID, "null d_crc (only LV_WAL_DECODE_NO_CHECKSUM allows it)");
    if (out->payload_cap && !out->d_payload) return set_err(LV_ERR_INVALID, "null d_payload");
    if (out->rec_cap && (!out->d_rec_off || !out->d_rec_len || !out->d_rec_log_off))
        return set_err(LV_ERR_INVALID, "null record array");
    {
        const int have = (out->d_rep_bytes != nullptr) + (out->d_rep_log_off != nullptr) + (out->d_rep_reason != nullptr);
        if (have != 0 && have != 3) return set_err(LV_ERR_INVALID, "null report array (all three or none)");
        if (have == 0 && out->rep_cap) return set_err(LV_ERR_INVALID, "null report array with rep_cap > 0");
    }
    if (misaligned(d_log, 8)) return set_err(LV_ERR_INVALID, "log must be 8-byte aligned");
    if (scan_cap > kMaxScanCap) return set_err(LV_ERR_INVALID, "scan_cap too large for one decode");
    if (!d_workspace) return set_err(LV_ERR_INVALID, "null workspace");
    if (misaligned(d_workspace, 16)) return set_err(LV_ERR_INVALID, "workspace must be 16-byte aligned");
    lvk::DecArgs A{};
    Carve C{static_cast<uint8_t *>(d_workspace)};
    dec_carve(C, scan_cap, A);
    if (workspace_bytes < C.at) return set_err(LV_ERR_INVALID, "workspace too small");
    if (overlaps(out->d_payload, out->payload_cap, d_log, bytes))
        return set_err(LV_ERR_INVALID, "d_payload overlaps d_log");
    DevCtx *c = nullptr;
    if (int rc = current_ctx(&c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    A.log = d_log;
    A.bytes = bytes;
    A.hdr_off = d_hdr_off;
    A.crc = checksum ? d_crc : nullptr;
    A.info = d_info;
    A.count = d_count;
    A.cap = scan_cap;
    A.nblocks = (static_cast<uint64_t>(bytes) + LV_WAL_BLOCK_SIZE - 1) / LV_WAL_BLOCK_SIZE;
    A.out = *out;
    if (!A.out.d_rep_bytes) A.out.rep_cap = 0;

    const uint64_t cus = static_cast<uint64_t>(c->cus > 0 ? c->cus : 1);
    const dim3 b(lvk::kDecThreads);
    if (scan_cap) {
        const uint64_t words = 3 * A.nb;
        const uint64_t g0 = std::min<uint64_t>((words + lvk::kDecThreads - 1) / lvk::kDecThreads, 8 * cus);
        hipLaunchKernelGGL(lvk::wal_dec_init, dim3(static_cast<uint32_t>(g0)), b, 0, s, A.fkill, words);
        const uint64_t g1 = lvgpu_internal::wal_classify_grid(scan_cap, cus);
        hipLaunchKernelGGL(lvk::wal_dec_classify, dim3(static_cast<uint32_t>(g1)), b, 0, s, A);
        const uint64_t g2 = lvgpu_internal::wal_tile_grid(scan_cap, cus);
        hipLaunchKernelGGL(lvk::wal_dec_reduce, dim3(static_cast<uint32_t>(g2)), b, 0, s, A);
    }
    hipLaunchKernelGGL(lvk::wal_dec_tiles, dim3(1), b, 0, s, A);
    if (scan_cap) {
        const uint64_t g4 = lvgpu_internal::wal_tile_grid(scan_cap, cus);
        hipLaunchKernelGGL(lvk::wal_dec_apply, dim3(static_cast<uint32_t>(g4)), b, 0, s, A);
        const uint64_t g5 = lvgpu_internal::wal_unframe_grid(std::min<uint64_t>(A.nblocks, A.nb), cus);
        if (g5) hipLaunchKernelGGL(lvk::wal_unframe_kernel, dim3(static_cast<uint32_t>(g5)), b, 0, s, A);
    }
    g_kernel = "wal_dec_classify+wal_dec_reduce+wal_dec_tiles+wal_dec_apply+wal_unframe_kernel";
    return check_launch();
}

}  // extern "C"
