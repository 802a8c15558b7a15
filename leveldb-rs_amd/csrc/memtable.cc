// The host twins of memtable.hip (include/lvgpu/memtable.h): the comparator of
// internal keys (dbformat.rs:153-170), the op table sorted into memtable
// order with std::sort, MemTable::get (memtable.rs:105-143) and DBIter's
// forward walk (upstream db/db_iter.cc) over such a table.  Host only, no
// GPU; the model-independent check of the device path and the baseline of
// tools/bench_memtable.py and tools/bench_mt_range.py.
#include "../../include/lvgpu/memtable.h"

#include <algorithm>
#include <cstring>

#include "../../include/lvgpu/crc32c.h"

namespace {

constexpr uint64_t kMaxOps = 0xfffffffeull;

// BytewiseComparator: -1 / 0 / +1, a proper prefix first.
int user_key_compare(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len) {
    const size_t m = a_len < b_len ? a_len : b_len;
    const int c = m ? std::memcmp(a, b, m) : 0;
    if (c) return c < 0 ? -1 : 1;
    return a_len < b_len ? -1 : a_len > b_len ? 1 : 0;
}

bool extent_ok(uint64_t off, uint64_t len, uint64_t bytes) { return off <= bytes && len <= bytes - off; }  // no wrap

bool op_ok(const lv_wb_op &o, uint64_t bytes) {
    return extent_ok(o.key_off, o.key_len, bytes) && extent_ok(o.val_off, o.val_len, bytes);
}

}  // namespace

extern "C" {

int lv_internal_key_compare(const uint8_t *a, size_t a_len, uint64_t a_tag, const uint8_t *b, size_t b_len,
                            uint64_t b_tag) {
    const int c = user_key_compare(a, a_len, b, b_len);
    if (c) return c;
    return a_tag > b_tag ? -1 : a_tag < b_tag ? 1 : 0;  // tag descending
}

int lv_memtable_build_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops, size_t n,
                           uint32_t *order, lv_mt_totals *totals) {
    if (!totals || (n && (!ops || !order)) || (!payload && payload_bytes) || n > kMaxOps) return LV_ERR_INVALID;
    totals->entries = n;
    totals->user_keys = 0;
    totals->status = 0;
    for (size_t i = 0; i < n; ++i)
        if (!op_ok(ops[i], payload_bytes)) {
            totals->status = LV_MT_BUILD_BAD_OP;
            return 0;
        }
    for (size_t i = 0; i < n; ++i) order[i] = static_cast<uint32_t>(i);
    std::sort(order, order + n, [&](uint32_t x, uint32_t y) {
        const lv_wb_op &a = ops[x], &b = ops[y];
        const int c = lv_internal_key_compare(payload + a.key_off, a.key_len, a.tag, payload + b.key_off, b.key_len,
                                              b.tag);
        return c ? c < 0 : x > y;  // an exact duplicate: the later op first
    });
    uint64_t keys = n ? 1 : 0;
    for (size_t i = 1; i < n; ++i) {
        const lv_wb_op &a = ops[order[i - 1]], &b = ops[order[i]];
        keys += user_key_compare(payload + a.key_off, a.key_len, payload + b.key_off, b.key_len) != 0;
    }
    totals->user_keys = keys;
    return 0;
}

int lv_memtable_get_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops, const uint32_t *order,
                         const lv_mt_totals *totals, const uint8_t *qkey, size_t qkey_len, uint64_t seq,
                         lv_mt_get_result *result) {
    if (!totals || !result || (!payload && payload_bytes) || (!qkey && qkey_len)) return LV_ERR_INVALID;
    if (totals->entries && !totals->status && (!ops || !order)) return LV_ERR_INVALID;
    lv_mt_get_result r{0, 0, 0, LV_MT_GET_ABSENT, 0};
    if (totals->status) {
        r.status = LV_MT_GET_NO_TABLE;
    } else if (seq > LV_MT_MAX_SEQUENCE) {
        r.status = LV_MT_GET_BAD_SEQ;
    } else {
        const uint64_t qtag = (seq << 8) | LV_WB_TYPE_VALUE;
        uint64_t lo = 0, hi = totals->entries;  // the first entry not less than (qkey, qtag)
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            const lv_wb_op &o = ops[order[mid]];
            if (lv_internal_key_compare(payload + o.key_off, o.key_len, o.tag, qkey, qkey_len, qtag) < 0)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo < totals->entries) {
            const lv_wb_op &o = ops[order[lo]];
            if (user_key_compare(payload + o.key_off, o.key_len, qkey, qkey_len) == 0) {
                r.op = order[lo];
                if ((o.tag & 0xff) == LV_WB_TYPE_VALUE) {
                    r.status = LV_MT_GET_FOUND;
                    r.val_off = o.val_off;
                    r.val_len = o.val_len;
                } else {
                    r.status = LV_MT_GET_DELETED;
                }
            }
        }
    }
    *result = r;
    return 0;
}

// DBIter's forward walk (include/lvgpu/memtable.h, "Range"): the serial loop
// of the header with `seen` as its state, the two seeks plain binary
// searches.  Every entry is range-checked before its key is read.
int lv_memtable_range_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops, const uint32_t *order,
                           const lv_mt_totals *totals, size_t op_cap, const uint8_t *qkeys, size_t qkeys_bytes,
                           const lv_mt_range_query *query, uint32_t limit, uint64_t max_scan, uint32_t *hits,
                           lv_mt_range_result *result) {
    if (!totals || !query || !hits || !result || (!payload && payload_bytes) || (!qkeys && qkeys_bytes) || !limit ||
        !max_scan)
        return LV_ERR_INVALID;
    const lv_mt_range_query &Q = *query;
    const uint64_t n = totals->entries, s = Q.seq;
    lv_mt_range_result r{0, 0, 0, 0, LV_MT_RANGE_DONE, 0, 0};
    const bool resume = Q.flags & LV_MT_RANGE_RESUME, has_hi = Q.flags & LV_MT_RANGE_HAS_HI;
    if (totals->status || n > op_cap || (n && (!ops || !order))) {
        r.status = LV_MT_GET_NO_TABLE;
    } else if (s > LV_MT_MAX_SEQUENCE) {
        r.status = LV_MT_GET_BAD_SEQ;
    } else if ((Q.flags & ~(LV_MT_RANGE_HAS_HI | LV_MT_RANGE_RESUME | LV_MT_RANGE_SEEN)) ||
               ((Q.flags & LV_MT_RANGE_SEEN) && !resume) || (!resume && !extent_ok(Q.lo_off, Q.lo_len, qkeys_bytes)) ||
               (has_hi && !extent_ok(Q.hi_off, Q.hi_len, qkeys_bytes)) || (resume && Q.pos > n)) {
        r.status = LV_MT_GET_BAD_QUERY;
    }
    if (r.status) {
        *result = r;
        return 0;
    }
    bool table_ok = true;
    // entry i's op, or null (and the table is not the build's) if it is out of range
    auto entry = [&](uint64_t i) -> const lv_wb_op * {
        const uint32_t idx = order[i];
        if (idx >= op_cap || !extent_ok(ops[idx].key_off, ops[idx].key_len, payload_bytes)) {
            table_ok = false;
            return nullptr;
        }
        return &ops[idx];
    };
    // the first position whose entry is not less than (key, tag); with_tag false: whose user key is >= key
    auto lower = [&](const uint8_t *key, size_t len, uint64_t tag, bool with_tag) -> uint64_t {
        uint64_t lo = 0, hi = n;
        while (lo < hi && table_ok) {
            const uint64_t mid = lo + (hi - lo) / 2;
            const lv_wb_op *o = entry(mid);
            if (!o) break;
            const int c = user_key_compare(payload + o->key_off, o->key_len, key, len);
            if (c < 0 || (with_tag && c == 0 && o->tag > tag))
                lo = mid + 1;
            else
                hi = mid;
        }
        return lo;
    };
    uint64_t start = Q.pos, end = n;
    if (!resume) start = lower(qkeys + Q.lo_off, Q.lo_len, (s << 8) | LV_WB_TYPE_VALUE, true);
    if (has_hi && table_ok) end = lower(qkeys + Q.hi_off, Q.hi_len, 0, false);
    bool seen = resume && (Q.flags & LV_MT_RANGE_SEEN);
    uint64_t p = start, examined = 0, unparsed = 0;
    uint32_t count = 0, status = LV_MT_RANGE_DONE;
    const lv_wb_op *prev = nullptr;  // e_{p-1} once it has been checked
    while (table_ok) {
        if (count == limit) {
            status = LV_MT_RANGE_MORE_LIMIT;
            break;
        }
        if (p >= end) break;
        if (examined == max_scan) {
            status = LV_MT_RANGE_MORE_SCAN;
            break;
        }
        if (p && !prev && !(prev = entry(p - 1))) break;
        const lv_wb_op *e = entry(p);
        if (!e) break;
        ++p, ++examined;
        if (!prev || user_key_compare(payload + prev->key_off, prev->key_len, payload + e->key_off, e->key_len) != 0)
            seen = false;  // e starts a group
        prev = e;
        const uint64_t type = e->tag & 0xff;
        if (type > LV_WB_TYPE_VALUE) {
            ++unparsed;
            continue;
        }
        if ((e->tag >> 8) > s || seen) continue;
        seen = true;
        if (type != LV_WB_TYPE_VALUE) continue;
        hits[count++] = order[p - 1];
    }
    if (!table_ok) {
        r.status = LV_MT_GET_NO_TABLE;
    } else {
        r.seek_pos = start;
        r.next_pos = p;
        r.unparsed = unparsed;
        r.count = count;
        r.status = status;
        r.seen = seen;
    }
    *result = r;
    return 0;
}

}  // extern "C"
