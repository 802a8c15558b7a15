// Stand-alone check of the compaction filter's host twin (csrc/compact.cc) for
// sanitizer builds on the CPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tools/compact_host_check.cc leveldb-rs_amd/csrc/compact.cc leveldb-rs_amd/csrc/memtable.cc
//       -o compact_host_check && ./compact_host_check
//
// tests/test_host_checks.py builds it this way and runs it with the CPU suite.
//
// Every payload, op array, order, range array and key block is a heap block of
// exactly its size, so a read or write one byte outside is a
// heap-buffer-overflow.  Three parts:
//   1. the corner cases of include/lvgpu/compact.h with their expected kept
//      entries written out by hand: snapshot thresholds, exact duplicates,
//      deletions with and without LV_COMPACT_BASE_LEVEL, unparsed type bytes,
//      the empty key and prefixes, ranges at their ends;
//   2. pseudo-random sorted tables against a second statement of the rule in
//      this file, the predecessor form the device computes;
//   3. orders, key extents and ranges that point outside: the status, nothing
//      written, nothing outside read.
// Exits 0 when everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lvgpu/compact.h"
#include "lvgpu/crc32c.h"

namespace {

int g_fail = 0;
long g_calls = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (g_fail < 50) std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                        \
        }                                                                    \
    } while (0)

struct Item {
    std::string key;
    uint64_t seq;
    uint32_t type;
};
using Range = std::pair<std::string, std::string>;

constexpr uint32_t kCanary = 0xA5A5A5A5u;

uint64_t g_rng = 0x2545f4914f6cdd1dull;
uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

// a heap copy of exactly n bytes (NULL for none)
template <class T>
T *exact(const T *p, size_t count) {
    if (!count) return nullptr;
    T *q = static_cast<T *>(std::malloc(count * sizeof(T)));
    std::memcpy(q, p, count * sizeof(T));
    return q;
}

struct Table {
    uint8_t *payload = nullptr;
    size_t payload_bytes = 0, n = 0;
    lv_wb_op *ops = nullptr;
    uint32_t *order = nullptr;
    lv_mt_totals mt{};
    lv_compact_range *ranges = nullptr;
    size_t n_ranges = 0;
    uint8_t *range_keys = nullptr;
    size_t range_keys_bytes = 0;
    void release() {
        std::free(payload);
        std::free(ops);
        std::free(order);
        std::free(ranges);
        std::free(range_keys);
    }
};

Table make(const std::vector<Item> &items, const std::vector<Range> &ranges) {
    Table t;
    std::string p, rk;
    std::vector<lv_wb_op> ops;
    for (const Item &it : items) {
        lv_wb_op o{};
        o.tag = (it.seq << 8) | it.type;
        o.key_off = p.size();
        o.key_len = static_cast<uint32_t>(it.key.size());
        p += it.key;
        o.val_off = p.size();
        ops.push_back(o);
    }
    std::vector<lv_compact_range> rr;
    for (const Range &r : ranges) {
        lv_compact_range g{};
        g.lo_off = rk.size();
        g.lo_len = static_cast<uint32_t>(r.first.size());
        rk += r.first;
        g.hi_off = rk.size();
        g.hi_len = static_cast<uint32_t>(r.second.size());
        rk += r.second;
        rr.push_back(g);
    }
    t.n = items.size();
    t.payload_bytes = p.size();
    t.payload = exact(reinterpret_cast<const uint8_t *>(p.data()), p.size());
    t.ops = exact(ops.data(), ops.size());
    std::vector<uint32_t> order(t.n ? t.n : 1);
    CHECK(lv_memtable_build_host(t.payload, t.payload_bytes, t.ops, t.n, t.n ? order.data() : nullptr, &t.mt) == 0);
    t.order = exact(order.data(), t.n);
    t.n_ranges = rr.size();
    t.ranges = exact(rr.data(), rr.size());
    t.range_keys_bytes = rk.size();
    t.range_keys = exact(reinterpret_cast<const uint8_t *>(rk.data()), rk.size());
    return t;
}

struct Out {
    lv_compact_totals t{};
    lv_mt_totals mt{};
    std::vector<uint32_t> order;  // order_out[0, kept)
};

// One call into an order_out of exactly n elements; checks the canaries beyond kept.
Out run(const Table &t, uint64_t S, uint32_t flags) {
    Out o;
    uint32_t *out = static_cast<uint32_t *>(t.n ? std::malloc(t.n * 4) : nullptr);
    for (size_t i = 0; i < t.n; ++i) out[i] = kCanary;
    std::memset(&o.t, 0xEE, sizeof o.t);
    std::memset(&o.mt, 0xEE, sizeof o.mt);
    CHECK(lv_compact_filter_host(t.payload, t.payload_bytes, t.ops, t.order, &t.mt, t.n, S, t.ranges, t.n_ranges,
                                 t.range_keys, t.range_keys_bytes, out, &o.mt, &o.t, flags) == 0);
    ++g_calls;
    CHECK(o.t.reserved == 0 && o.t.entries_in == t.mt.entries);
    if (o.t.status) {
        CHECK(o.t.kept == 0 && o.t.dropped_hidden == 0 && o.t.dropped_deletions == 0 && o.t.unparsed == 0 && o.t.user_keys == 0);
        CHECK(o.mt.entries == 0 && o.mt.user_keys == 0 && o.mt.status == LV_MT_BUILD_UPSTREAM);
        for (size_t i = 0; i < t.n; ++i) CHECK(out[i] == kCanary);
    } else {
        CHECK(o.t.kept + o.t.dropped_hidden + o.t.dropped_deletions == t.n && o.t.kept <= t.n);
        CHECK(o.mt.entries == o.t.kept && o.mt.user_keys == o.t.user_keys && o.mt.status == 0);
        for (size_t i = o.t.kept; i < t.n; ++i) CHECK(out[i] == kCanary);
        o.order.assign(out, out + (o.t.kept <= t.n ? o.t.kept : 0));
    }
    std::free(out);
    return o;
}

// The kept entries as "key@seq/type" in output order.
std::string show(const std::vector<Item> &items, const Out &o) {
    std::string s;
    for (uint32_t i : o.order) s += items[i].key + "@" + std::to_string(items[i].seq) + "/" + std::to_string(items[i].type) + " ";
    return s;
}

void expect(const std::vector<Item> &items, const std::vector<Range> &ranges, uint64_t S, uint32_t flags,
            const char *want) {
    Table t = make(items, ranges);
    const Out o = run(t, S, flags);
    const std::string got = show(items, o);
    if (o.t.status != 0 || got != want) {
        std::fprintf(stderr, "S=%llu flags=%u: got \"%s\" (status %llu), want \"%s\"\n", static_cast<unsigned long long>(S),
                     flags, got.c_str(), static_cast<unsigned long long>(o.t.status), want);
        ++g_fail;
    }
    t.release();
}

bool same_key(const Table &t, const lv_wb_op &a, const lv_wb_op &b) {
    return a.key_len == b.key_len && (!a.key_len || std::memcmp(t.payload + a.key_off, t.payload + b.key_off, a.key_len) == 0);
}

int cmp(const uint8_t *a, size_t al, const uint8_t *b, size_t bl) {
    const size_t m = al < bl ? al : bl;
    const int c = m ? std::memcmp(a, b, m) : 0;
    return c ? c : al < bl ? -1 : al > bl ? 1 : 0;
}

// The predecessor form (compact.h, "The same, entry by entry") against the twin's loop.
void check_predecessor_form(const std::vector<Item> &items, const std::vector<Range> &ranges, uint64_t S, uint32_t flags) {
    Table t = make(items, ranges);
    const Out o = run(t, S, flags);
    CHECK(o.t.status == 0);
    std::vector<uint32_t> kept;
    uint64_t hidden = 0, dels = 0, unparsed = 0, keys = 0;
    for (size_t i = 0; i < t.n; ++i) {
        const lv_wb_op &e = t.ops[t.order[i]];
        const uint32_t type = e.tag & 0xff;
        bool drop = false;
        if (type > 1) {
            ++unparsed;
        } else {
            uint64_t prev_seq = LV_MT_MAX_SEQUENCE;
            if (i) {
                const lv_wb_op &p = t.ops[t.order[i - 1]];
                if ((p.tag & 0xff) <= 1 && same_key(t, p, e)) prev_seq = p.tag >> 8;
            }
            if (prev_seq <= S) {
                drop = true;
                ++hidden;
            } else if (type == 0 && (e.tag >> 8) <= S && (flags & LV_COMPACT_BASE_LEVEL)) {
                bool held = false;
                for (size_t r = 0; r < t.n_ranges && !held; ++r) {
                    const lv_compact_range &g = t.ranges[r];
                    held = cmp(t.payload + e.key_off, e.key_len, t.range_keys + g.lo_off, g.lo_len) >= 0 &&
                           cmp(t.payload + e.key_off, e.key_len, t.range_keys + g.hi_off, g.hi_len) <= 0;
                }
                if (!held) {
                    drop = true;
                    ++dels;
                }
            }
        }
        if (drop) continue;
        keys += kept.empty() || !same_key(t, t.ops[kept.back()], e);
        kept.push_back(t.order[i]);
    }
    CHECK(kept == o.order);
    CHECK(o.t.dropped_hidden == hidden && o.t.dropped_deletions == dels && o.t.unparsed == unparsed && o.t.user_keys == keys);
    t.release();
}

void corner_cases() {
    const uint32_t B = LV_COMPACT_BASE_LEVEL;
    const uint64_t MAX = LV_MT_MAX_SEQUENCE;
    // snapshot thresholds: one key at sequences 1..6
    std::vector<Item> k;
    for (uint64_t s = 1; s <= 6; ++s) k.push_back({"k", s, 1});
    expect(k, {}, 0, 0, "k@6/1 k@5/1 k@4/1 k@3/1 k@2/1 k@1/1 ");
    expect(k, {}, 2, 0, "k@6/1 k@5/1 k@4/1 k@3/1 k@2/1 ");
    expect(k, {}, 3, 0, "k@6/1 k@5/1 k@4/1 k@3/1 ");
    expect(k, {}, 4, 0, "k@6/1 k@5/1 k@4/1 ");
    expect(k, {}, 6, 0, "k@6/1 ");
    expect(k, {}, 7, 0, "k@6/1 ");
    expect(k, {}, MAX - 1, B, "k@6/1 ");
    // exact duplicates on both sides of S
    const std::vector<Item> d = {{"d", 5, 1}, {"d", 9, 1}, {"d", 5, 1}, {"d", 9, 1}};
    expect(d, {}, 4, 0, "d@9/1 d@9/1 d@5/1 d@5/1 ");
    expect(d, {}, 5, 0, "d@9/1 d@9/1 d@5/1 ");
    expect(d, {}, 9, 0, "d@9/1 ");
    // deletions: first in its group, shadowed, shadowing, at S and at S + 1
    const std::vector<Item> del = {{"a", 5, 0}, {"a", 3, 1}, {"b", 7, 1}, {"b", 5, 0}, {"b", 2, 1},
                                   {"c", 6, 0}, {"c", 4, 1}, {"e", 5, 0}, {"f", 6, 0}};
    expect(del, {}, 5, 0, "a@5/0 b@7/1 b@5/0 c@6/0 c@4/1 e@5/0 f@6/0 ");
    expect(del, {}, 5, B, "b@7/1 c@6/0 c@4/1 f@6/0 ");
    expect(del, {}, 6, B, "b@7/1 ");
    expect(del, {{"a", "b"}}, 6, B, "a@5/0 b@7/1 b@5/0 ");
    // type bytes 2 and 0xff inside a group: kept, and the entry behind is a first entry again
    const std::vector<Item> u = {{"u", 6, 1}, {"u", 5, 1}, {"u", 4, 2}, {"u", 3, 1}, {"u", 2, 1},
                                 {"v", 9, 1}, {"v", 8, 0xff}, {"v", 7, 0}, {"v", 6, 1}};
    expect(u, {}, 9, 0, "u@6/1 u@4/2 u@3/1 v@9/1 v@8/255 v@7/0 ");
    expect(u, {}, 9, B, "u@6/1 u@4/2 u@3/1 v@9/1 v@8/255 ");
    // the empty key, prefixes, keys equal in 16 bytes
    const std::string p16 = "0123456789abcdef";
    std::vector<Item> keys;
    for (const std::string &key : {std::string(), std::string("a"), std::string("ab"), p16, p16 + "x", p16 + "y", p16 + "xx"})
        for (uint64_t s : {7, 3}) keys.push_back({key, s, 1});
    expect(keys, {}, 8, 0, "@7/1 0123456789abcdef@7/1 0123456789abcdefx@7/1 0123456789abcdefxx@7/1 0123456789abcdefy@7/1 a@7/1 ab@7/1 ");
    // ranges: lo and hi are inside, one byte outside each is not, nor is a prefix of lo
    std::vector<Item> r;
    for (const char *key : {"bbb", "ddd", "bba", "ddda", "bb", "ccc"}) r.push_back({key, 3, 0});
    expect(r, {}, 5, B, "");
    expect(r, {{"bbb", "ddd"}}, 5, B, "bbb@3/0 ccc@3/0 ddd@3/0 ");
    expect(r, {{"bbb", "ddd"}}, 2, B, "bb@3/0 bba@3/0 bbb@3/0 ccc@3/0 ddd@3/0 ddda@3/0 ");
    std::vector<Range> many;
    for (int i = 0; i < 4095; ++i) many.push_back({"r" + std::to_string(10000 + i), "r" + std::to_string(10000 + i) + "~"});
    many.push_back({"bbb", "ddd"});
    expect(r, many, 5, B, "bbb@3/0 ccc@3/0 ddd@3/0 ");
}

void random_tables() {
    for (int trial = 0; trial < 400; ++trial) {
        const unsigned sym = trial % 2 ? 2 : 3;
        const size_t n = rnd() % 200;
        std::vector<Item> items;
        for (size_t i = 0; i < n; ++i) {
            std::string key(rnd() % (trial % 5 == 0 ? 20 : 4), '\0');
            for (char &ch : key) ch = static_cast<char>('a' + rnd() % sym);
            const uint32_t type = rnd() % 40 == 0 ? 2 + rnd() % 254 : rnd() % 3 ? 1 : 0;
            items.push_back({key, rnd() % 12, type});
        }
        std::vector<Range> ranges;
        for (size_t i = 0, m = trial % 3 ? rnd() % 4 : 0; i < m; ++i) {
            std::string a(rnd() % 4, 'a'), b(rnd() % 4, 'a');
            for (char &ch : a) ch = static_cast<char>('a' + rnd() % sym);
            for (char &ch : b) ch = static_cast<char>('a' + rnd() % sym);
            if (a > b) std::swap(a, b);
            ranges.push_back({a, b});
        }
        check_predecessor_form(items, ranges, rnd() % 14, ranges.empty() ? trial % 2 : LV_COMPACT_BASE_LEVEL);
    }
}

void out_of_range() {
    const std::vector<Item> items = {{"a", 3, 1}, {"a", 2, 1}, {"b", 4, 0}, {"tail", 9, 1}};  // the payload ends with a key
    {
        Table t = make(items, {});
        t.order[2] = static_cast<uint32_t>(t.n);  // an index equal to op_cap
        CHECK(run(t, 5, 0).t.status == LV_COMPACT_BAD_INPUT);
        t.order[2] = 0xffffffffu;
        CHECK(run(t, 5, 0).t.status == LV_COMPACT_BAD_INPUT);
        t.release();
    }
    {
        Table t = make(items, {});
        uint8_t *shorter = exact(t.payload, t.payload_bytes - 1);  // the last key ends one byte past it
        std::free(t.payload);
        t.payload = shorter;
        --t.payload_bytes;
        CHECK(run(t, 5, LV_COMPACT_BASE_LEVEL).t.status == LV_COMPACT_BAD_INPUT);
        t.release();
    }
    for (int which = 0; which < 3; ++which) {  // key_off past the payload, key_len past it, a wrapping offset
        Table t = make(items, {});
        lv_wb_op &o = t.ops[1];
        if (which == 0) o.key_off = t.payload_bytes + 1;
        if (which == 1) o.key_len = static_cast<uint32_t>(t.payload_bytes + 1);
        if (which == 2) o.key_off = ~0ull;
        CHECK(run(t, 5, 0).t.status == LV_COMPACT_BAD_INPUT);
        t.release();
    }
    {
        Table t = make(items, {});
        t.mt.entries = t.n + 1;  // more entries than op_cap
        CHECK(run(t, 5, 0).t.status == LV_COMPACT_BAD_INPUT);
        t.mt.entries = t.n;
        t.mt.status = LV_MT_BUILD_BAD_OP;
        CHECK(run(t, 5, 0).t.status == LV_COMPACT_UPSTREAM);
        t.release();
    }
    for (int which = 0; which < 5; ++which) {
        Table t = make(items, {{"aaa", "zzz"}, {"b", "c"}});
        lv_compact_range &g = t.ranges[which % 2];
        if (which == 0) g.hi_len += 6;                    // hi runs past the keys
        if (which == 1) g.lo_off = t.range_keys_bytes + 1;
        if (which == 2) g.hi_off = ~0ull - 1;             // wraps
        if (which == 3) std::swap(g.lo_off, g.hi_off);    // lo > hi
        if (which == 4) g.lo_len = 0xffffffffu;
        const Out o = run(t, 5, LV_COMPACT_BASE_LEVEL);
        CHECK(o.t.status == LV_COMPACT_BAD_RANGE);
        t.order[0] = 77;  // with BAD_RANGE the entries are not examined
        CHECK(run(t, 5, LV_COMPACT_BASE_LEVEL).t.status == LV_COMPACT_BAD_RANGE);
        t.release();
    }
    // LV_ERR_INVALID: S, flags, ranges without the flag, too many ranges, op_cap
    Table t = make(items, {{"a", "b"}});
    std::vector<uint32_t> out(t.n);
    lv_mt_totals mo;
    lv_compact_totals ct;
    auto call = [&](uint64_t S, size_t n_ranges, uint32_t flags, size_t op_cap) {
        return lv_compact_filter_host(t.payload, t.payload_bytes, t.ops, t.order, &t.mt, op_cap, S, t.ranges, n_ranges,
                                      t.range_keys, t.range_keys_bytes, out.data(), &mo, &ct, flags);
    };
    CHECK(call(5, 1, LV_COMPACT_BASE_LEVEL, t.n) == 0);
    CHECK(call(LV_MT_MAX_SEQUENCE, 0, 0, t.n) == LV_ERR_INVALID);
    CHECK(call(5, 1, 0, t.n) == LV_ERR_INVALID);
    CHECK(call(5, 0, 2, t.n) == LV_ERR_INVALID);
    CHECK(call(5, LV_COMPACT_MAX_RANGES + 1, LV_COMPACT_BASE_LEVEL, t.n) == LV_ERR_INVALID);
    CHECK(call(5, 0, 0, 0xffffffffull) == LV_ERR_INVALID);
    t.release();
}

}  // namespace

int main() {
    corner_cases();
    random_tables();
    out_of_range();
    std::printf("%ld calls; %d failures\n", g_calls, g_fail);
    return g_fail ? 1 : 0;
}
