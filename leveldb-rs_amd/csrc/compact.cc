// The host twin of compact.hip (include/lvgpu/compact.h): upstream's
// DoCompactionWork loop over a sorted memtable quadruple in host memory, with
// has_cur, cur and last_seq as its state.  The device decides every entry from
// its predecessor instead; this file deliberately does not, so that the two
// forms check each other.  Host only, no GPU; tools/compact_host_check.cc runs
// it under a sanitizer and tools/bench_compact.py times it as the
// copy-back route.
#include "../../include/lvgpu/compact.h"

#include <cstring>

#include "../../include/lvgpu/crc32c.h"

namespace {

bool extent_ok(uint64_t off, uint64_t len, uint64_t bytes) { return off <= bytes && len <= bytes - off; }  // no wrap

// BytewiseComparator: -1 / 0 / +1, a proper prefix first.
int key_compare(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len) {
    const size_t m = a_len < b_len ? a_len : b_len;
    const int c = m ? std::memcmp(a, b, m) : 0;
    if (c) return c < 0 ? -1 : 1;
    return a_len < b_len ? -1 : a_len > b_len ? 1 : 0;
}

struct Ranges {
    const lv_compact_range *r;
    size_t n;
    const uint8_t *keys;
    bool on;  // LV_COMPACT_BASE_LEVEL
};

// IsBaseLevelForKey: no range holds k.
bool base_level(const Ranges &R, const uint8_t *k, size_t k_len) {
    if (!R.on) return false;
    for (size_t i = 0; i < R.n; ++i) {
        const lv_compact_range &g = R.r[i];
        if (key_compare(k, k_len, R.keys + g.lo_off, g.lo_len) >= 0 &&
            key_compare(k, k_len, R.keys + g.hi_off, g.hi_len) <= 0)
            return false;
    }
    return true;
}

}  // namespace

extern "C" {

int lv_compact_filter_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops, const uint32_t *order,
                           const lv_mt_totals *mt_totals, size_t op_cap, uint64_t smallest_snapshot,
                           const lv_compact_range *ranges, size_t n_ranges, const uint8_t *range_keys,
                           size_t range_keys_bytes, uint32_t *order_out, lv_mt_totals *mt_totals_out,
                           lv_compact_totals *totals, uint32_t flags) {
    if (!mt_totals || !mt_totals_out || !totals || (!payload && payload_bytes) ||
        (op_cap && (!ops || !order || !order_out)) || (!ranges && n_ranges) || (!range_keys && range_keys_bytes))
        return LV_ERR_INVALID;
    if ((flags & ~LV_COMPACT_BASE_LEVEL) || op_cap > 0xfffffffeull || n_ranges > LV_COMPACT_MAX_RANGES ||
        (n_ranges && !(flags & LV_COMPACT_BASE_LEVEL)) || smallest_snapshot >= LV_MT_MAX_SEQUENCE)
        return LV_ERR_INVALID;
    const uint64_t S = smallest_snapshot, n = mt_totals->entries;
    lv_compact_totals t{};
    t.entries_in = n;
    if (mt_totals->status) {
        t.status = LV_COMPACT_UPSTREAM;
    } else {
        for (size_t i = 0; i < n_ranges; ++i) {
            const lv_compact_range &g = ranges[i];
            if (!extent_ok(g.lo_off, g.lo_len, range_keys_bytes) || !extent_ok(g.hi_off, g.hi_len, range_keys_bytes) ||
                key_compare(range_keys + g.lo_off, g.lo_len, range_keys + g.hi_off, g.hi_len) > 0) {
                t.status |= LV_COMPACT_BAD_RANGE;
                break;
            }
        }
        if (n > op_cap) t.status |= LV_COMPACT_BAD_INPUT;
    }
    if (!t.status)  // every entry is compared or kept: every index and key extent counts
        for (uint64_t i = 0; i < n; ++i)
            if (order[i] >= op_cap || !extent_ok(ops[order[i]].key_off, ops[order[i]].key_len, payload_bytes)) {
                t.status = LV_COMPACT_BAD_INPUT;
                break;
            }
    if (t.status) {
        *mt_totals_out = lv_mt_totals{0, 0, LV_MT_BUILD_UPSTREAM};
        *totals = t;
        return 0;
    }
    const Ranges R{ranges, n_ranges, range_keys, (flags & LV_COMPACT_BASE_LEVEL) != 0};
    bool has_cur = false, has_out = false;
    const uint8_t *cur = nullptr, *out_key = nullptr;  // the loop's current user key; the last kept entry's
    size_t cur_len = 0, out_len = 0;
    uint64_t last_seq = LV_MT_MAX_SEQUENCE;
    for (uint64_t i = 0; i < n; ++i) {
        const lv_wb_op &e = ops[order[i]];
        const uint8_t *k = payload + e.key_off;
        const uint32_t type = static_cast<uint32_t>(e.tag & 0xff);
        const uint64_t seq = e.tag >> 8;
        bool drop = false;
        if (type > 1) {  // ParseInternalKey fails: kept, and the state forgets its key
            has_cur = false;
            last_seq = LV_MT_MAX_SEQUENCE;
            ++t.unparsed;
        } else {
            if (!has_cur || key_compare(k, e.key_len, cur, cur_len) != 0) {
                cur = k;
                cur_len = e.key_len;
                has_cur = true;
                last_seq = LV_MT_MAX_SEQUENCE;
            }
            if (last_seq <= S) {  // rule A
                drop = true;
                ++t.dropped_hidden;
            } else if (type == 0 && seq <= S && base_level(R, k, e.key_len)) {  // rule B
                drop = true;
                ++t.dropped_deletions;
            }
            last_seq = seq;
        }
        if (drop) continue;
        if (!has_out || key_compare(k, e.key_len, out_key, out_len) != 0) ++t.user_keys;
        out_key = k;
        out_len = e.key_len;
        has_out = true;
        order_out[t.kept++] = order[i];
    }
    *mt_totals_out = lv_mt_totals{t.kept, t.user_keys, 0};
    *totals = t;
    return 0;
}

}  // extern "C"
