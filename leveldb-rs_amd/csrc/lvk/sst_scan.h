// The SSTable scan's serial core (include/lvgpu/table.h, "Scan"): the walks
// over the index block, a data block's header, one restart run and one entry
// of it, over an image in memory.  One text for both halves, as lvk/sst_read.h
// is for the reader: sst_scan.cc compiles it for lv_sst_scan_host, sst_scan.hip
// gives a lane to every block and to every restart run, so the bounds logic the
// host check program (tools/sst_scan_host_check.cc) runs under a sanitizer is
// the logic a lane runs.  Everything here reads file[0, file_bytes) only,
// whatever the bytes say, by sst_read.h's rules: every offset is a u64 compared
// against its limit before the byte is touched.
//
// A run is walked twice with the same steps: once keeping only lengths (count)
// and once writing (emit).  Of the previous key the emit keeps its offset in
// the arena, its user key's length and its tag: the next key's shared bytes
// come from what was just written there, and from the tag where the shared
// prefix runs into it.  Positions are byte positions of the internal key, as
// in sst_read.h's Cursor.
#pragma once
#include <stdint.h>

#include "sst_read.h"

namespace lvs {
namespace {

using lvr::Entry;
using lvr::Restarts;

// The index block of *t over file[0, fb): false is CORRUPT.
LVR_FN bool index_header(const uint8_t *file, uint64_t fb, uint64_t io, uint64_t is, uint64_t want_n, Restarts *r) {
    if (!lvr::in_range(io, is, fb) || file[io + is] != LV_SST_NO_COMPRESSION) return false;
    return lvr::restarts(file + io, is, r) && r->n == want_n;
}

struct Block {
    uint64_t off, size;  // the handle
    uint64_t n, arr;     // its restart array: n runs
    // the empty BlockBuilder: its single run counts, and holds no entry
    LVR_FN bool empty() const { return n == 1 && arr == 0; }
};

// Data block b of the index (b < ir.n): its handle from the index entry at
// restart b and its header.  false is CORRUPT.
LVR_FN bool block_header(const uint8_t *file, uint64_t fb, uint64_t io, const Restarts &ir, uint64_t b, Block *k) {
    const uint8_t *idx = file + io;
    Entry e;
    if (!lvr::decode(idx, lvr::le32(idx + ir.arr + 4 * b), ir.arr, &e) || e.shared != 0 || e.non_shared < 8)
        return false;
    if (!lvr::handle(idx, e.value_at(), e.end(), &k->off, &k->size) || !lvr::in_range(k->off, k->size, fb))
        return false;
    if (file[k->off + k->size] != LV_SST_NO_COMPRESSION) return false;
    Restarts r;
    if (!lvr::restarts(file + k->off, k->size, &r)) return false;
    k->n = r.n;
    k->arr = r.arr;
    return true;
}

// One restart run while it is walked: raw[at, end) is what is left of it.
struct Walk {
    uint64_t at, end, klen;  // klen: the previous key's length, 0 before the first
    LVR_FN bool done() const { return at >= end; }
};

// Run r < k.n of the block raw[0, k.size): false is CORRUPT.  Each run checks
// its own two restarts, so all runs together check the whole array: restart[0]
// is 0, they strictly increase and the last is below arr.
LVR_FN bool run_begin(const uint8_t *raw, const Block &k, uint64_t r, Walk *w) {
    w->klen = 0;
    if (k.empty()) {
        w->at = w->end = 0;
        return true;
    }
    w->at = lvr::le32(raw + k.arr + 4 * r);
    w->end = r + 1 < k.n ? lvr::le32(raw + k.arr + 4 * (r + 1)) : k.arr;
    return (r != 0 || w->at == 0) && w->at < w->end && w->end <= k.arr;
}

// The next entry of a run that is not done: false is CORRUPT.  The run's end
// is the decode's limit, so the entries tile it or the last decode fails.
LVR_FN bool step(const uint8_t *raw, Walk *w, Entry *e) {
    if (!lvr::decode(raw, w->at, w->end, e) || e->shared > w->klen) return false;
    const uint64_t klen = static_cast<uint64_t>(e->shared) + e->non_shared;
    if (klen < 8) return false;
    w->klen = klen;  // at most the run's bytes so far: below 2^32
    w->at = e->end();
    return true;
}

// A run's entry count and the arena bytes its entries take: false is CORRUPT.
LVR_FN bool run_count(const uint8_t *raw, const Block &k, uint64_t r, uint64_t *entries, uint64_t *bytes) {
    Walk w;
    Entry e;
    *entries = *bytes = 0;
    if (!run_begin(raw, k, r, &w)) return false;
    while (!w.done()) {
        if (!step(raw, &w, &e)) return false;
        ++*entries;
        *bytes += w.klen - 8 + e.value_len;
    }
    return true;
}

// The previous entry of the run being emitted.
struct Prev {
    uint64_t koff = 0, tag = 0;  // its user key's offset in the arena
    uint32_t ulen = 0;
};

struct Copy {
    uint8_t *dst;
    const uint8_t *src;
    uint64_t len;
};

// Byte `pos` of the previous internal key, pos < its length.
LVR_FN uint32_t prev_byte(const uint8_t *arena, const Prev &p, uint64_t pos) {
    return pos < p.ulen ? arena[p.koff + pos] : static_cast<uint32_t>(p.tag >> (8 * (pos - p.ulen))) & 0xffu;
}

// Entry e (step() accepted it; w->klen is its key's length) to the arena at
// koff and to *op.  The bytes that come from the previous key's tag and the
// new tag are handled here; the three long pieces (the shared user-key bytes
// from the previous key in the arena, the key suffix and the value from the
// block) are returned as copy jobs, for the caller to run: memcpy on the host,
// the lane or its wave on the device.  jobs[0] reads what the previous entry's
// jobs wrote: they must have completed.  Returns the offset behind the entry.
LVR_FN uint64_t emit_entry(const uint8_t *raw, const Entry &e, uint64_t klen, uint8_t *arena, uint64_t koff, Prev *p,
                           lv_wb_op *op, Copy jobs[3]) {
    const uint64_t ulen = klen - 8, shared = e.shared;
    const uint64_t su = shared < ulen ? shared : ulen;     // shared bytes that are user-key bytes here
    const uint64_t from_arena = su < p->ulen ? su : p->ulen;
    jobs[0] = Copy{arena + koff, arena + p->koff, from_arena};
    for (uint64_t j = from_arena; j < su; ++j)  // the previous tag's bytes that became user-key bytes: at most 8
        arena[koff + j] = static_cast<uint8_t>(p->tag >> (8 * (j - p->ulen)));
    jobs[1] = Copy{arena + koff + su, raw + e.key_at, ulen - su};
    uint64_t tag = 0;
    for (uint32_t t = 0; t < 8; ++t) {
        const uint64_t pos = ulen + t;
        const uint64_t byte = pos < shared ? prev_byte(arena, *p, pos) : raw[e.key_at + (pos - shared)];
        tag |= byte << (8 * t);
    }
    jobs[2] = Copy{arena + koff + ulen, raw + e.value_at(), e.value_len};
    op->tag = tag;
    op->key_off = koff;
    op->val_off = koff + ulen;
    op->key_len = static_cast<uint32_t>(ulen);
    op->val_len = e.value_len;
    p->koff = koff;
    p->tag = tag;
    p->ulen = static_cast<uint32_t>(ulen);
    return koff + ulen + e.value_len;
}

// lv_internal_key_compare of two ops over the arena: -1 a first, 0 equal, +1 b
// first; *same_user: their user keys are equal.
LVR_FN int op_compare(const uint8_t *arena, const lv_wb_op &a, const lv_wb_op &b, bool *same_user) {
    const uint32_t m = a.key_len < b.key_len ? a.key_len : b.key_len;
    const uint32_t l = lvr::lcp(arena + a.key_off, arena + b.key_off, m);
    *same_user = l == m && a.key_len == b.key_len;
    if (l < m) return arena[a.key_off + l] < arena[b.key_off + l] ? -1 : 1;
    if (a.key_len != b.key_len) return a.key_len < b.key_len ? -1 : 1;
    return a.tag > b.tag ? -1 : a.tag < b.tag ? 1 : 0;  // tag descending
}

// no wrap: base + add > cap
LVR_FN bool over(uint64_t base, uint64_t add, uint64_t cap) { return base > cap || add > cap - base; }

}  // namespace
}  // namespace lvs
