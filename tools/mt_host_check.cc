// Stand-alone check of the memtable host twins (csrc/memtable.cc) for
// sanitizer builds on the CPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tools/mt_host_check.cc leveldb-rs_amd/csrc/memtable.cc -o mt_host_check && ./mt_host_check
//
// tests/test_host_checks.py builds it this way and runs it with the CPU suite.
//
// Every payload is copied into a heap buffer of exactly its size, so a read
// one byte past it is a heap-buffer-overflow.  Inputs: corner keys (the empty
// key, lengths around 8, zero padding, bytes 0x7f / 0x80 / 0xff, long common
// prefixes), tags with their top bits set, exact duplicates, a few hundred
// pseudo-random op tables over small alphabets, and op tables with a bad
// extent.  The order lv_memtable_build_host writes is checked to be a
// permutation that is strictly increasing under the three rules, evaluated
// here by a bytewise loop of its own; lv_memtable_get_host is checked against
// a linear scan.  Exits 0 when everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lvgpu/memtable.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                        \
        }                                                                    \
    } while (0)

struct Item {
    std::string key, value;
    uint64_t tag;
};

struct Table {
    uint8_t *payload = nullptr;  // exactly `bytes` long
    size_t bytes = 0;
    std::vector<lv_wb_op> ops;
    ~Table() { std::free(payload); }
};

void make_table(const std::vector<Item> &items, size_t gap, Table *t) {
    std::string p;
    for (const Item &it : items) {
        p.append(gap, '\xEE');
        lv_wb_op o;
        o.tag = it.tag;
        o.key_off = p.size();
        o.key_len = static_cast<uint32_t>(it.key.size());
        p += it.key;
        o.val_off = p.size();
        o.val_len = static_cast<uint32_t>(it.value.size());
        p += it.value;
        t->ops.push_back(o);
    }
    t->bytes = p.size();
    t->payload = static_cast<uint8_t *>(std::malloc(p.size() ? p.size() : 1));
    if (p.size()) std::memcpy(t->payload, p.data(), p.size());
    if (!p.size()) {  // a zero-length payload: no byte may be read
        std::free(t->payload);
        t->payload = nullptr;
    }
}

// rules 1 and 2, bytewise
int slow_compare(const std::string &a, uint64_t ta, const std::string &b, uint64_t tb) {
    const size_t m = a.size() < b.size() ? a.size() : b.size();
    for (size_t i = 0; i < m; ++i) {
        const unsigned x = static_cast<unsigned char>(a[i]), y = static_cast<unsigned char>(b[i]);
        if (x != y) return x < y ? -1 : 1;
    }
    if (a.size() != b.size()) return a.size() < b.size() ? -1 : 1;
    return ta > tb ? -1 : ta < tb ? 1 : 0;
}

void check_table(const std::vector<Item> &items, size_t gap) {
    Table t;
    make_table(items, gap, &t);
    const size_t n = items.size();
    std::vector<uint32_t> order(n ? n : 1, 0xdeadbeef);
    lv_mt_totals tot{99, 99, 99};
    CHECK(lv_memtable_build_host(t.payload, t.bytes, n ? t.ops.data() : nullptr, n, n ? order.data() : nullptr, &tot) == 0);
    CHECK(tot.entries == n && tot.status == 0);
    std::vector<char> seen(n, 0);
    uint64_t keys = n ? 1 : 0;
    for (size_t i = 0; i < n; ++i) {
        CHECK(order[i] < n && !seen[order[i]]);
        if (order[i] >= n) return;
        seen[order[i]] = 1;
        if (!i) continue;
        const Item &a = items[order[i - 1]], &b = items[order[i]];
        const int c = slow_compare(a.key, a.tag, b.key, b.tag);
        CHECK(c < 0 || (c == 0 && order[i - 1] > order[i]));  // strictly increasing: the later duplicate first
        CHECK(lv_internal_key_compare(reinterpret_cast<const uint8_t *>(a.key.data()), a.key.size(), a.tag,
                                      reinterpret_cast<const uint8_t *>(b.key.data()), b.key.size(), b.tag) == c);
        keys += a.key != b.key;
    }
    CHECK(tot.user_keys == keys);
    // get: every stored key at its own sequence, one below, and the maximum; extended and cut keys
    for (size_t q = 0; q < n; ++q) {
        for (int variant = 0; variant < 5; ++variant) {
            std::string k = items[q].key;
            uint64_t seq = items[q].tag >> 8;
            if (variant == 1) seq = seq ? seq - 1 : 0;
            if (variant == 2) seq = LV_MT_MAX_SEQUENCE;
            if (variant == 3) k.push_back('\0');
            if (variant == 4 && !k.empty()) k.pop_back();
            lv_mt_get_result r{1, 1, 1, 99, 1};
            uint8_t *qk = static_cast<uint8_t *>(std::malloc(k.size() ? k.size() : 1));
            if (k.size()) std::memcpy(qk, k.data(), k.size());
            CHECK(lv_memtable_get_host(t.payload, t.bytes, t.ops.data(), order.data(), &tot, k.size() ? qk : nullptr,
                                       k.size(), seq, &r) == 0);
            std::free(qk);
            if (seq > LV_MT_MAX_SEQUENCE) {
                CHECK(r.status == LV_MT_GET_BAD_SEQ);
                continue;
            }
            // linear scan: the first entry not less than (k, (seq << 8) | 1)
            uint32_t want = LV_MT_GET_ABSENT, want_op = 0;
            for (size_t i = 0; i < n; ++i) {
                const Item &e = items[order[i]];
                if (slow_compare(e.key, e.tag, k, (seq << 8) | 1) < 0) continue;
                if (e.key == k) {
                    want = (e.tag & 0xff) == LV_WB_TYPE_VALUE ? LV_MT_GET_FOUND : LV_MT_GET_DELETED;
                    want_op = order[i];
                }
                break;
            }
            CHECK(r.status == want && r.op == want_op && r.reserved == 0);
            if (want == LV_MT_GET_FOUND)
                CHECK(r.val_off == t.ops[want_op].val_off && r.val_len == t.ops[want_op].val_len);
            else
                CHECK(r.val_off == 0 && r.val_len == 0);
        }
    }
}

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

uint64_t tag(uint64_t seq, uint32_t type) { return (seq << 8) | type; }

}  // namespace

int main() {
    // corner keys, all in one table and each pair alone
    const std::string p40(40, 'p'), big(4999, 'B');
    std::vector<std::string> corner = {
        "", std::string(1, '\0'), "a", std::string("a\0", 2), std::string("a\0\0", 3), "a" + std::string(8, '\0'),
        "prefix", "prefix_", "prefix_8", "prefix_89", "\x7fx", "\x80x", "\xffx", "12345678\x7f", "12345678\x80",
        "12345678\xff", "12345678", "ab", "ba", "abcdefghab", "abcdefghba", p40 + "a", p40 + "b", p40,
        big + "\x01", big + "\x02", big};
    std::vector<Item> all;
    for (size_t i = 0; i < corner.size(); ++i) all.push_back({corner[(i * 7) % corner.size()], "v", tag(100 + i, 1)});
    check_table(all, 0);
    check_table(all, 3);
    for (const std::string &a : corner)
        for (const std::string &b : corner) check_table({{a, "x", tag(1, 1)}, {b, "y", tag(1, 1)}}, 1);
    // tags: versions, VALUE and DELETION at one sequence, top bits, exact duplicates
    std::vector<Item> tags;
    for (uint64_t s : {5ull, 900ull, 1ull, 77ull, 900ull}) tags.push_back({"versions", "v", tag(s, 1)});
    tags.push_back({"versions", "", tag(77, 0)});
    for (uint64_t s : {1ull << 56, (1ull << 56) - 1, 1ull << 55, ~0ull >> 8, 3ull}) {
        tags.push_back({"top", "t", tag(s, 1)});
        tags.push_back({"top", "", tag(s, 0)});
    }
    for (int i = 0; i < 3; ++i) tags.push_back({"dup", "same", tag(42, 1)});
    tags.push_back({"dup", "", tag(42, 0)});
    check_table(tags, 0);
    check_table({}, 0);
    check_table({{"", "", tag(0, 0)}}, 0);
    // pseudo-random tables over small alphabets
    for (int trial = 0; trial < 300; ++trial) {
        const unsigned sym = trial % 3 == 0 ? 2 : trial % 3 == 1 ? 4 : 256;
        const size_t n = rnd() % 120;
        std::vector<Item> items;
        for (size_t i = 0; i < n; ++i) {
            std::string k(rnd() % (trial % 2 ? 24 : 11), '\0');
            for (char &c : k) c = static_cast<char>(rnd() % sym);
            const uint32_t type = rnd() % 4 ? 1 : 0;
            items.push_back({k, type ? std::string(rnd() % 5, 'v') : "", tag(rnd() % 6, type)});
        }
        check_table(items, trial % 4);
    }
    // bad extents: BAD_OP, no order written, nothing outside the payload read
    {
        Table t;
        make_table({{"alpha", "1", tag(1, 1)}, {"beta", "2", tag(2, 1)}, {"gamma", "3", tag(3, 1)}}, 0, &t);
        const lv_wb_op good = t.ops[1];
        const uint64_t offs[] = {t.bytes - 3, t.bytes + 1, ~0ull - 1, t.bytes};
        const uint32_t lens[] = {4, 0, 8, 1};
        for (int f = 0; f < 2; ++f)
            for (int k = 0; k < 4; ++k) {
                t.ops[1] = good;
                (f ? t.ops[1].val_off : t.ops[1].key_off) = offs[k];
                (f ? t.ops[1].val_len : t.ops[1].key_len) = lens[k];
                uint32_t order[3] = {7, 7, 7};
                lv_mt_totals tot{99, 99, 99};
                CHECK(lv_memtable_build_host(t.payload, t.bytes, t.ops.data(), 3, order, &tot) == 0);
                CHECK(tot.status == LV_MT_BUILD_BAD_OP && tot.entries == 3 && tot.user_keys == 0);
                CHECK(order[0] == 7 && order[1] == 7 && order[2] == 7);
                lv_mt_get_result r{};
                CHECK(lv_memtable_get_host(t.payload, t.bytes, t.ops.data(), order, &tot,
                                           reinterpret_cast<const uint8_t *>("beta"), 4, 9, &r) == 0);
                CHECK(r.status == LV_MT_GET_NO_TABLE);
            }
        lv_mt_totals tot{};
        CHECK(lv_memtable_build_host(t.payload, t.bytes, t.ops.data(), 3, nullptr, &tot) != 0);  // LV_ERR_INVALID
        CHECK(lv_memtable_build_host(t.payload, t.bytes, t.ops.data(), 3, nullptr, nullptr) != 0);
    }
    if (g_fail) {
        std::fprintf(stderr, "mt_host_check: %d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("mt_host_check: ok");
    return 0;
}
