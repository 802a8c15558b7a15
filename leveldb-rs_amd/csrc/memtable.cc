// The host twins of memtable.hip (include/lvgpu/memtable.h): the comparator of
// internal keys (dbformat.rs:153-170), the op table sorted into memtable
// order with std::sort, and MemTable::get (memtable.rs:105-143) over such a
// table.  Host only, no GPU; the model-independent check of the device path
// and the baseline of tools/bench_memtable.py.
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

}  // extern "C"
