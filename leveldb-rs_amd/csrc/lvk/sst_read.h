// The SSTable reader's serial core (include/lvgpu/table.h, "Open" and "Get"):
// Table::Open's checks and Table::InternalGet + SaveValue for one query, over
// an image in memory.  One text for both halves: sst_get.cc compiles it for
// the host twins, sst_get.hip for the kernels, so the bounds logic the host
// check program (tools/sst_get_host_check.cc) runs under a sanitizer is the
// logic a lane runs.  Everything here reads file[0, file_bytes) only, whatever
// the bytes say: every offset is a u64 compared against its limit before the
// byte is touched, and no length is added to a pointer unchecked.  The filter
// block's reader ("Bloom filter blocks": hash, bloom_open, may_match) is here
// too, and get() asks it when given one; the build's filter emit uses hash.
//
// Keys are never materialised.  While a restart run is scanned the cursor
// keeps, of the current internal key (prefix-compressed against its
// predecessor), only what the comparison with the target needs:
//   klen  its length;
//   l     the common-prefix length of its byte string and the query's user
//         key, capped at ql;
//   d     its byte at position l (when l < klen);
//   W     its bytes at [ql, ql + 8) as a little-endian word: the tag when its
//         user key has the query's length.
// An entry with shared = s leaves l and d alone when s > l (the bytes that
// decided are shared) and otherwise resumes the comparison at s; W keeps its
// bytes below s and takes the rest from the suffix.  This holds when a shared
// prefix runs from one key's tag into the next key's user bytes and the other
// way round, because the cursor speaks of byte positions, not of key parts.
#pragma once
#include <stdint.h>

#include "../../../include/lvgpu/table.h"

#if defined(__HIPCC__)
#define LVR_FN __host__ __device__ __forceinline__
#else
#define LVR_FN inline
#endif

namespace lvr {
namespace {

constexpr uint64_t kLarge = 0xffffffffull;  // raw block sizes from here on are refused (sst_in_range)

// a block {off, size} and its 5-byte trailer lie inside file[0, fb): u64, no wrap
LVR_FN bool in_range(uint64_t off, uint64_t size, uint64_t fb) {
    return size < kLarge && off <= fb && size <= fb - off && fb - off - size >= LV_SST_TRAILER_SIZE;
}

// a fixed32 at any byte alignment
LVR_FN uint32_t le32(const uint8_t *p) {
    return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 |
           static_cast<uint32_t>(p[3]) << 24;
}

// decode_varint_64_limit (sst_format.cc): at most 10 bytes of b[*at, limit)
LVR_FN bool varint64(const uint8_t *b, uint64_t *at, uint64_t limit, uint64_t *v) {
    uint64_t r = 0;
    for (uint32_t shift = 0; shift <= 63 && *at < limit; shift += 7) {
        const uint64_t c = b[(*at)++];
        r |= (c & 0x7f) << shift;
        if (!(c & 0x80)) {
            *v = r;
            return true;
        }
    }
    return false;
}

// lv_sst_block_handle_decode over b[at, limit); trailing bytes are the caller's
LVR_FN bool handle(const uint8_t *b, uint64_t at, uint64_t limit, uint64_t *off, uint64_t *size) {
    return varint64(b, &at, limit, off) && varint64(b, &at, limit, size);
}

// GetVarint32Ptr: at most 5 bytes of b[*at, limit); the fifth byte's bits
// beyond 2^32 are dropped, a sixth continuation byte fails.
LVR_FN bool varint32(const uint8_t *b, uint64_t *at, uint64_t limit, uint32_t *v) {
    uint32_t r = 0;
    for (uint32_t shift = 0; shift <= 28 && *at < limit; shift += 7) {
        const uint32_t c = b[(*at)++];
        r |= (c & 0x7f) << shift;
        if (!(c & 0x80)) {
            *v = r;
            return true;
        }
    }
    return false;
}

struct Entry {
    uint32_t shared, non_shared, value_len;
    uint64_t key_at;  // the key suffix's offset in the block; the value follows it
    LVR_FN uint64_t value_at() const { return key_at + non_shared; }
    LVR_FN uint64_t end() const { return key_at + non_shared + value_len; }
};

// DecodeEntry over raw[p, limit)
LVR_FN bool decode(const uint8_t *raw, uint64_t p, uint64_t limit, Entry *e) {
    if (p > limit || limit - p < 3) return false;
    if (!varint32(raw, &p, limit, &e->shared) || !varint32(raw, &p, limit, &e->non_shared) ||
        !varint32(raw, &p, limit, &e->value_len))
        return false;
    if (limit - p < static_cast<uint64_t>(e->non_shared) + e->value_len) return false;
    e->key_at = p;
    return true;
}

// the common-prefix length of a[0, n) and b[0, n)
LVR_FN uint32_t lcp(const uint8_t *a, const uint8_t *b, uint32_t n) {
    uint32_t i = 0;
    for (; i + 8 <= n; i += 8) {  // whole words lie inside both strings
        uint64_t x, y;
        __builtin_memcpy(&x, a + i, 8);
        __builtin_memcpy(&y, b + i, 8);
        if (x != y) return i + (static_cast<uint32_t>(__builtin_ctzll(x ^ y)) >> 3);
    }
    for (; i < n; ++i)
        if (a[i] != b[i]) break;
    return i;
}

struct Target {
    const uint8_t *q;  // the user key
    uint32_t ql;
    uint64_t tag;      // (seq << 8) | 1
};

struct Cursor {
    uint64_t klen = 0, W = 0;
    uint32_t l = 0, d = 0;

    // The next key: `shared` bytes of this one (shared <= klen, the caller's
    // check), then suf[0, ns).
    LVR_FN void advance(const Target &t, uint32_t shared, uint32_t ns, const uint8_t *suf) {
        const uint64_t len = static_cast<uint64_t>(shared) + ns;
        if (shared <= l) {  // <= ql
            const uint32_t room = t.ql - shared;
            const uint32_t i = lcp(suf, t.q + shared, ns < room ? ns : room);
            l = shared + i;
            d = i < ns ? suf[i] : 0u;
        }
        if (shared <= t.ql && len >= static_cast<uint64_t>(t.ql) + 8) {
            __builtin_memcpy(&W, suf + (t.ql - shared), 8);  // x86-64 and gfx950 are little-endian
        } else {
            for (uint32_t j = 0; j < 8; ++j) {
                const uint64_t pos = static_cast<uint64_t>(t.ql) + j;
                if (pos < shared) continue;
                const uint64_t byte = pos < len ? suf[pos - shared] : 0u;
                W = (W & ~(0xffull << (8 * j))) | (byte << (8 * j));
            }
        }
        klen = len;
    }

    // InternalKeyComparator of this key (klen >= 8) against the target: -1 it
    // is less; 0 it is not and its user key is the query's; +1 it is not and
    // its user key is greater.
    LVR_FN int compare(const Target &t) const {
        const uint64_t ulen = klen - 8, m = ulen < t.ql ? ulen : t.ql;
        if (l < m) return d < t.q[l] ? -1 : 1;
        if (ulen != t.ql) return ulen < t.ql ? -1 : 1;
        return W > t.tag ? -1 : 0;
    }
};

// A block's restart array: false for a corrupt header.  n == 0 is legal.
struct Restarts {
    uint64_t n, arr;
};
LVR_FN bool restarts(const uint8_t *raw, uint64_t size, Restarts *r) {
    if (size < 4) return false;
    r->n = le32(raw + size - 4);
    if (r->n > (size - 4) / 4) return false;
    r->arr = size - 4 - 4 * r->n;
    return true;
}

// The contiguous key of the entry at restart i against the target, into *c
// and *e: false for an entry that fails to decode, shares bytes or is shorter
// than a tag.
LVR_FN bool probe(const uint8_t *raw, const Restarts &r, uint64_t i, const Target &t, Cursor *c, Entry *e) {
    if (!decode(raw, le32(raw + r.arr + 4 * i), r.arr, e) || e->shared != 0 || e->non_shared < 8) return false;
    *c = Cursor();
    c->advance(t, 0, e->non_shared, raw + e->key_at);
    return true;
}

enum Seek { kSeekNone, kSeekHit, kSeekCorrupt };

// Block::Iter::Seek over a data block raw[0, size): the first entry not less
// than the target, in *c (its key) and *e.
LVR_FN Seek block_seek(const uint8_t *raw, uint64_t size, const Target &t, Cursor *c, Entry *e) {
    Restarts r;
    if (!restarts(raw, size, &r)) return kSeekCorrupt;
    if (!r.n) return kSeekNone;
    uint64_t left = 0, right = r.n - 1;
    while (left < right) {
        const uint64_t mid = (left + right + 1) / 2;
        if (!probe(raw, r, mid, t, c, e)) return kSeekCorrupt;
        if (c->compare(t) < 0)
            left = mid;
        else
            right = mid - 1;
    }
    uint64_t at = le32(raw + r.arr + 4 * left);
    *c = Cursor();
    for (;;) {  // every entry is at least 3 bytes: at most arr / 3 rounds
        if (at >= r.arr) return kSeekNone;
        if (!decode(raw, at, r.arr, e) || e->shared > c->klen ||
            static_cast<uint64_t>(e->shared) + e->non_shared < 8)
            return kSeekCorrupt;
        c->advance(t, e->shared, e->non_shared, raw + e->key_at);
        if (c->compare(t) >= 0) return kSeekHit;
        at = e->end();
    }
}

// ---- the filter block (table.h, "Bloom filter blocks") ----

constexpr uint32_t kBloomSeed = LV_SST_BLOOM_SEED;  // BloomHash(key) = Hash(key, this)

// util/hash.rs (upstream's Hash) for one key at any alignment: the 4-byte
// steps are assembled from bytes.
LVR_FN uint32_t hash(const uint8_t *d, uint64_t n, uint32_t seed) {
    constexpr uint32_t m = 0xc6a4a793u;
    uint32_t h = seed ^ (m * static_cast<uint32_t>(n));
    uint64_t i = 0;
    for (; i + 4 <= n; i += 4) {
        h += le32(d + i);
        h *= m;
        h ^= h >> 16;
    }
    const uint64_t rest = n - i;
    if (rest >= 3) h += static_cast<uint32_t>(d[i + 2]) << 16;
    if (rest >= 2) h += static_cast<uint32_t>(d[i + 1]) << 8;
    if (rest >= 1) {
        h += d[i];
        h *= m;
        h ^= h >> 24;
    }
    return h;
}

// BloomFilterPolicy::KeyMayMatch for a key's hash over the filter f[0, len).
LVR_FN bool bloom_may_match(const uint8_t *f, uint64_t len, uint32_t h) {
    if (len < 2) return false;
    const uint64_t bits = (len - 1) * 8;
    const uint32_t k = f[len - 1];
    if (k > 30) return true;  // reserved for other encodings
    const uint32_t delta = (h >> 17) | (h << 15);
    for (uint32_t j = 0; j < k; ++j) {
        const uint64_t pos = h % bits;
        if (!(f[pos / 8] & (1u << (pos % 8)))) return false;
        h += delta;
    }
    return true;
}

// Table::ReadMeta + ReadFilter over file[0, fb) whose metaindex block is
// {mo, ms}: every field of *b.  Any failure is "no filter", never an error.
LVR_FN void bloom_open(const uint8_t *file, uint64_t fb, uint64_t mo, uint64_t ms, lv_sst_bloom *b) {
    constexpr char name[] = LV_SST_BLOOM_NAME;
    constexpr uint32_t kName = sizeof(name) - 1;
    *b = lv_sst_bloom{};
    b->why = LV_SST_BLOOM_BAD_METAINDEX;
    Restarts r;
    if (!in_range(mo, ms, fb) || file[mo + ms] != LV_SST_NO_COMPRESSION || !restarts(file + mo, ms, &r)) return;
    const uint8_t *raw = file + mo;
    // the first entry not less than the name, walking from offset 0; of each
    // key only its first kName + 1 bytes are kept
    uint8_t key[kName + 1];
    uint64_t at = 0, klen = 0;
    Entry e{};
    bool hit = false;
    while (r.n && at < r.arr) {
        if (!decode(raw, at, r.arr, &e) || e.shared > klen) return;
        for (uint64_t i = e.shared; i < kName + 1 && i < static_cast<uint64_t>(e.shared) + e.non_shared; ++i)
            key[i] = raw[e.key_at + (i - e.shared)];
        klen = static_cast<uint64_t>(e.shared) + e.non_shared;
        const uint64_t m = klen < kName ? klen : kName;
        int c = 0;
        for (uint64_t i = 0; i < m && !c; ++i)
            c = key[i] < static_cast<uint8_t>(name[i]) ? -1 : key[i] > static_cast<uint8_t>(name[i]) ? 1 : 0;
        if (!c) c = klen < kName ? -1 : klen > kName ? 1 : 0;
        if (c >= 0) {
            hit = c == 0;
            break;
        }
        at = e.end();
    }
    b->why = LV_SST_BLOOM_NO_ENTRY;
    if (!hit) return;
    uint64_t fo, fs;
    b->why = LV_SST_BLOOM_BAD_HANDLE;
    if (!handle(raw, e.value_at(), e.end(), &fo, &fs) || !in_range(fo, fs, fb)) return;
    b->why = LV_SST_BLOOM_BAD_TYPE;
    if (file[fo + fs] != LV_SST_NO_COMPRESSION) return;
    b->why = LV_SST_BLOOM_SHORT;
    if (fs < 5) return;
    const uint64_t array = le32(file + fo + fs - 5);
    b->why = LV_SST_BLOOM_BAD_ARRAY;
    if (array > fs - 5) return;
    b->filter_offset = fo;
    b->filter_size = fs;
    b->array_offset = array;
    b->num = (fs - 5 - array) / 4;
    b->base_lg = file[fo + fs - 1];
    b->present = 1;
    b->why = 0;
}

// FilterBlockReader::KeyMayMatch.  Every offset of *b is range-checked again
// against fb: a *b that was not written for this file reads nothing outside
// it (and then answers "may match", as no filter does).
LVR_FN bool may_match(const uint8_t *file, uint64_t fb, const lv_sst_bloom &b, uint64_t block_offset,
                      const uint8_t *key, uint32_t klen) {
    const uint64_t fs = b.filter_size, array = b.array_offset;
    if (b.present != 1 || !in_range(b.filter_offset, fs, fb) || fs < 5 || array > fs - 5 ||
        b.num > (fs - 5 - array) / 4)
        return true;
    const uint8_t *data = file + b.filter_offset;
    const uint64_t i = b.base_lg < 64 ? block_offset >> b.base_lg : 0;
    if (i >= b.num) return true;  // errors are potential matches
    const uint64_t start = le32(data + array + 4 * i), limit = le32(data + array + 4 * i + 4);
    if (start <= limit && limit <= array) return bloom_may_match(data + start, limit - start, hash(key, klen, kBloomSeed));
    return start != limit;
}

// Table::InternalGet + SaveValue for one target over file[0, fb) whose index
// block is {io, is}.  *res arrives zeroed; the status is returned.  With a
// filter (bloom != nullptr) it is asked once the data block's handle is known
// to be in range and before anything of the block is read.
LVR_FN uint32_t get(const uint8_t *file, uint64_t fb, uint64_t io, uint64_t is, const Target &t,
                    lv_sst_get_result *res, const lv_sst_bloom *bloom = nullptr) {
    if (!fb) return LV_SST_GET_ABSENT;  // the empty table
    if (!in_range(io, is, fb)) return LV_SST_GET_CORRUPT;
    const uint8_t *idx = file + io;
    Restarts r;
    if (!restarts(idx, is, &r)) return LV_SST_GET_CORRUPT;
    Cursor c;
    Entry e;
    uint64_t lo = 0, hi = r.n;  // the first index entry not less than the target
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (!probe(idx, r, mid, t, &c, &e)) return LV_SST_GET_CORRUPT;
        if (c.compare(t) < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo >= r.n) return LV_SST_GET_ABSENT;
    if (!probe(idx, r, lo, t, &c, &e)) return LV_SST_GET_CORRUPT;
    uint64_t off, size;
    if (!handle(idx, e.value_at(), e.end(), &off, &size) || !in_range(off, size, fb)) return LV_SST_GET_CORRUPT;
    if (bloom && !may_match(file, fb, *bloom, off, t.q, t.ql)) {
        res->reserved = LV_SST_GET_FILTERED;
        return LV_SST_GET_ABSENT;
    }
    if (file[off + size] != LV_SST_NO_COMPRESSION) return LV_SST_GET_CORRUPT;
    const Seek s = block_seek(file + off, size, t, &c, &e);
    if (s == kSeekCorrupt) return LV_SST_GET_CORRUPT;
    if (s == kSeekNone || c.compare(t) != 0) return LV_SST_GET_ABSENT;
    const uint32_t type = static_cast<uint32_t>(c.W & 0xff);
    if (type > 1) return LV_SST_GET_CORRUPT;
    res->tag = c.W;
    res->block = static_cast<uint32_t>(lo);
    if (type == 0) return LV_SST_GET_DELETED;
    res->val_off = off + e.value_at();
    res->val_len = e.value_len;
    return LV_SST_GET_FOUND;
}

// ---- Table::Open ----

// The footer and the index block's header: every field of *t but the status
// bits the restarts decide.  fb is neither 0 nor beyond the buffer.
LVR_FN void open_header(const uint8_t *file, uint64_t fb, lv_sst_table *t) {
    *t = lv_sst_table{};
    t->file_bytes = fb;
    if (fb < LV_SST_FOOTER_SIZE) {
        t->status = LV_SST_OPEN_NOT_A_TABLE;
        return;
    }
    const uint8_t *foot = file + fb - LV_SST_FOOTER_SIZE;
    const uint64_t magic = static_cast<uint64_t>(le32(foot + 44)) << 32 | le32(foot + 40);
    if (magic != LV_SST_MAGIC) {
        t->status = LV_SST_OPEN_NOT_A_TABLE;
        return;
    }
    uint64_t at = 0, h[4];
    for (int i = 0; i < 4; ++i)
        if (!varint64(foot, &at, LV_SST_FOOTER_SIZE, &h[i])) {
            t->status = LV_SST_OPEN_BAD_FOOTER;
            return;
        }
    if (!in_range(h[0], h[1], fb) || !in_range(h[2], h[3], fb)) {
        t->status = LV_SST_OPEN_BAD_FOOTER;
        return;
    }
    t->metaindex_offset = h[0];
    t->metaindex_size = h[1];
    t->index_offset = h[2];
    t->index_size = h[3];
    Restarts r;
    if (file[h[2] + h[3]] != LV_SST_NO_COMPRESSION || !restarts(file + h[2], h[3], &r) || r.n < 1) {
        t->status = LV_SST_OPEN_BAD_INDEX;
        return;
    }
    t->data_blocks = r.n;
}

// Restart i < data_blocks of the index block: its status bits, and the handle
// of its first entry when that one is sound.
LVR_FN uint32_t open_restart(const uint8_t *file, const lv_sst_table &t, uint64_t i, uint64_t *off, uint64_t *size) {
    const uint8_t *idx = file + t.index_offset;
    const uint64_t n = t.data_blocks, arr = t.index_size - 4 - 4 * n;
    uint64_t at = le32(idx + arr + 4 * i);
    const uint64_t end = i + 1 < n ? le32(idx + arr + 4 * (i + 1)) : arr;
    if (end > arr || at >= end) return LV_SST_OPEN_BAD_INDEX;  // no entry, or one outside the entries
    uint64_t klen = 0, count = 0;
    while (at < end) {
        Entry e;
        uint64_t o, s;
        if (!decode(idx, at, end, &e) || e.shared > klen) return LV_SST_OPEN_BAD_INDEX;
        klen = static_cast<uint64_t>(e.shared) + e.non_shared;
        if (klen < 8 || !handle(idx, e.value_at(), e.end(), &o, &s) || !in_range(o, s, t.file_bytes))
            return LV_SST_OPEN_BAD_INDEX;
        if (!count) {
            *off = o;
            *size = s;
        }
        ++count;
        at = e.end();
    }
    return count > 1 ? LV_SST_OPEN_INDEX_SHAPE : 0u;
}

}  // namespace
}  // namespace lvr
