// Stand-alone check of the SSTable build's host twin (csrc/sst_build.cc) for
// sanitizer builds on the CPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tools/sst_host_check.cc leveldb-rs_amd/csrc/sst_build.cc leveldb-rs_amd/csrc/sst_format.cc
//       leveldb-rs_amd/csrc/memtable.cc leveldb-rs_amd/csrc/crc32c_scalar.cc -o sst_host_check && ./sst_host_check
//
// tests/test_host_checks.py builds it this way and runs it with the CPU suite.
// (sst_format.cc reports its errors through lvgpu_internal::set_error, which
// lives in a HIP unit; this file supplies a stub.)  Every payload, file and
// handle array is a heap buffer of exactly its size, so a read or write one
// byte outside is a heap-buffer-overflow.  Inputs: the corner tables of the
// format (entry counts around the restart interval, a block end on a restart,
// one big entry, prefixes across the key / tag edge, exact duplicates, empty
// keys and values, every separator and successor branch, varint widths) and a
// few hundred pseudo-random tables over small block sizes.  Each image is
// opened again by a reader written here: footer, index block, every data
// block by its restart array, every trailer recomputed; the entries must be
// the memtable's in order and every index key must lie between its block's
// last key and the next block's first.  Then every status: exact and short
// capacities, a sizing pass, a failed memtable.  Exits 0 when everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lvgpu/crc32c.h"
#include "lvgpu/table.h"

namespace lvgpu_internal {
int set_error(int code, const char *) { return code; }
}  // namespace lvgpu_internal

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

uint64_t tag(uint64_t seq, uint32_t type) { return (seq << 8) | type; }

std::string ikey(const std::string &k, uint64_t t) {
    std::string s = k;
    for (int i = 0; i < 8; ++i) s.push_back(static_cast<char>(t >> (8 * i)));
    return s;
}

// a heap copy of exactly n bytes (NULL for none)
uint8_t *exact(const void *p, size_t n) {
    if (!n) return nullptr;
    uint8_t *q = static_cast<uint8_t *>(std::malloc(n));
    std::memcpy(q, p, n);
    return q;
}

bool get_varint(const std::string &b, size_t *at, uint64_t *v) {
    uint64_t r = 0;
    for (unsigned shift = 0; shift <= 63 && *at < b.size(); shift += 7) {
        const uint8_t c = static_cast<uint8_t>(b[(*at)++]);
        r |= static_cast<uint64_t>(c & 0x7f) << shift;
        if (!(c & 0x80)) {
            *v = r;
            return true;
        }
    }
    return false;
}

uint32_t fixed32(const std::string &b, size_t at) {
    uint32_t v = 0;
    for (int i = 3; i >= 0; --i) v = (v << 8) | static_cast<uint8_t>(b[at + i]);
    return v;
}

// the entries of a block, walked by its restart array
bool read_block(const std::string &file, uint64_t off, uint64_t size, std::vector<std::pair<std::string, std::string>> *out,
                size_t *restarts) {
    if (off + size + 5 > file.size() || size < 8) return false;
    const std::string raw = file.substr(off, size);
    const uint8_t type = static_cast<uint8_t>(file[off + size]);
    const uint32_t crc = lv_crc32c_extend(lv_crc32c_value(reinterpret_cast<const uint8_t *>(raw.data()), raw.size()), &type, 1);
    if (type != 0 || fixed32(file, off + size + 1) != lv_crc32c_mask(crc)) return false;
    const size_t n = fixed32(raw, raw.size() - 4);
    if (n < 1 || 4 + 4 * n > raw.size()) return false;
    const size_t arr = raw.size() - 4 - 4 * n;
    *restarts = n;
    for (size_t r = 0; r < n; ++r) {
        size_t at = fixed32(raw, arr + 4 * r);
        const size_t end = r + 1 < n ? fixed32(raw, arr + 4 * r + 4) : arr;
        if ((r == 0 && at != 0) || at > end || end > arr) return false;
        std::string key;
        bool first = true;
        while (at < end) {
            uint64_t shared, non_shared, vlen;
            if (!get_varint(raw, &at, &shared) || !get_varint(raw, &at, &non_shared) || !get_varint(raw, &at, &vlen))
                return false;
            if (shared > key.size() || (first && shared) || at + non_shared + vlen > end) return false;
            key = key.substr(0, shared) + raw.substr(at, non_shared);
            at += non_shared;
            out->emplace_back(key, raw.substr(at, vlen));
            at += vlen;
            first = false;
        }
        if (at != end) return false;
    }
    return true;
}

int cmp_ikey(const std::string &a, const std::string &b) {
    uint64_t ta = 0, tb = 0;
    for (int i = 7; i >= 0; --i) {
        ta = (ta << 8) | static_cast<uint8_t>(a[a.size() - 8 + i]);
        tb = (tb << 8) | static_cast<uint8_t>(b[b.size() - 8 + i]);
    }
    return lv_internal_key_compare(reinterpret_cast<const uint8_t *>(a.data()), a.size() - 8, ta,
                                   reinterpret_cast<const uint8_t *>(b.data()), b.size() - 8, tb);
}

void check_table(const std::vector<Item> &items, uint32_t bs, uint32_t ri, size_t gap) {
    std::string p;
    std::vector<lv_wb_op> ops;
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
        ops.push_back(o);
    }
    const size_t n = items.size();
    uint8_t *payload = exact(p.data(), p.size());
    std::vector<uint32_t> order(n ? n : 1);
    lv_mt_totals mt{};
    CHECK(lv_memtable_build_host(payload, p.size(), n ? ops.data() : nullptr, n, n ? order.data() : nullptr, &mt) == 0);
    CHECK(mt.status == 0);
    const lv_sst_build_options opt{bs, ri};
    // the sizing pass
    lv_sst_build_totals size{};
    CHECK(lv_sst_build_host(payload, p.size(), ops.data(), order.data(), &mt, &opt, nullptr, 0, nullptr, 0, &size) == 0);
    CHECK(size.status == 0 && size.entries == n);
    CHECK(lv_sst_build_file_bound(p.size(), n, &opt) >= size.file_bytes);
    // exact capacities
    const size_t nh = n ? size.data_blocks + 2 : 0;
    uint8_t *file = static_cast<uint8_t *>(std::malloc(size.file_bytes ? size.file_bytes : 1));
    uint64_t *handles = static_cast<uint64_t *>(std::malloc(16 * (size.data_blocks + 2)));
    lv_sst_build_totals tot{};
    CHECK(lv_sst_build_host(payload, p.size(), ops.data(), order.data(), &mt, &opt, size.file_bytes ? file : nullptr,
                            size.file_bytes, handles, size.data_blocks, &tot) == 0);
    CHECK(std::memcmp(&tot, &size, sizeof tot) == 0);
    if (n && !tot.status) {
        const std::string f(reinterpret_cast<const char *>(file), tot.file_bytes);
        uint64_t h[4];
        CHECK(lv_sst_footer_decode(file + tot.file_bytes - 48, 48, h) == 0);
        CHECK(h[0] == tot.metaindex_offset && h[1] == 8 && h[2] == tot.index_offset && h[3] == tot.index_size);
        CHECK(handles[2 * (nh - 2)] == h[0] && handles[2 * (nh - 1)] == h[2] && handles[2 * (nh - 1) + 1] == h[3]);
        std::vector<std::pair<std::string, std::string>> meta, index, all;
        size_t r = 0;
        CHECK(read_block(f, h[0], h[1], &meta, &r) && meta.empty());
        CHECK(read_block(f, h[2], h[3], &index, &r) && index.size() == tot.data_blocks && r == index.size());
        std::string prev_last;
        for (size_t b = 0; b < index.size(); ++b) {
            uint64_t off = 0, sz = 0;
            size_t used = 0;
            const std::string &hv = index[b].second;
            CHECK(lv_sst_block_handle_decode(reinterpret_cast<const uint8_t *>(hv.data()), hv.size(), &off, &sz, &used) == 0);
            CHECK(used == hv.size() && off == handles[2 * b] && sz == handles[2 * b + 1]);
            std::vector<std::pair<std::string, std::string>> ents;
            CHECK(read_block(f, off, sz, &ents, &r) && !ents.empty());
            if (ents.empty()) break;
            CHECK(r == (ents.size() + ri - 1) / ri);
            CHECK(cmp_ikey(ents.back().first, index[b].first) <= 0);
            if (b) CHECK(cmp_ikey(index[b - 1].first, ents.front().first) < 0 ||
                         (prev_last == index[b - 1].first && prev_last == ents.front().first));
            prev_last = ents.back().first;
            all.insert(all.end(), ents.begin(), ents.end());
        }
        CHECK(all.size() == n);
        for (size_t i = 0; i < n && i < all.size(); ++i) {
            const Item &it = items[order[i]];
            CHECK(all[i].first == ikey(it.key, it.tag) && all[i].second == it.value);
        }
        // one byte or one handle short: the status, the true totals
        lv_sst_build_totals t2{};
        uint8_t *small = static_cast<uint8_t *>(std::malloc(tot.file_bytes - 1));
        CHECK(lv_sst_build_host(payload, p.size(), ops.data(), order.data(), &mt, &opt, small, tot.file_bytes - 1, handles,
                                size.data_blocks, &t2) == 0);
        CHECK(t2.status == LV_SST_BUILD_FILE_OVER && t2.file_bytes == tot.file_bytes);
        CHECK(lv_sst_build_host(payload, p.size(), ops.data(), order.data(), &mt, &opt, file, tot.file_bytes, handles,
                                size.data_blocks - 1, &t2) == 0);
        CHECK(t2.status == LV_SST_BUILD_HANDLE_OVER && t2.data_blocks == tot.data_blocks);
        std::free(small);
    } else {
        CHECK(tot.file_bytes == 0 && tot.data_blocks == 0);
    }
    lv_mt_totals failed = mt;
    failed.status = LV_MT_BUILD_BAD_OP;
    lv_sst_build_totals t3{};
    CHECK(lv_sst_build_host(payload, p.size(), ops.data(), order.data(), &failed, &opt, nullptr, 0, nullptr, 0, &t3) == 0);
    CHECK(t3.status == LV_SST_BUILD_NO_TABLE && t3.entries == 0 && t3.file_bytes == 0);
    std::free(file);
    std::free(handles);
    std::free(payload);
}

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

std::vector<Item> seq_items(size_t n) {
    std::vector<Item> v;
    for (size_t i = 0; i < n; ++i) {
        char k[24];
        std::snprintf(k, sizeof k, "%06zu", i);
        v.push_back({k, "vvv", tag(100 + i, 1)});
    }
    return v;
}

}  // namespace

int main() {
    for (size_t n : {0, 1, 15, 16, 17, 32, 33}) check_table(seq_items(n), 4096, 16, n % 3);
    check_table(seq_items(40), 64, 4, 0);
    check_table({{"a", "s", tag(1, 1)}, {"big", std::string(9000, 'B'), tag(2, 1)}, {"c", "t", tag(3, 1)}}, 4096, 16, 1);
    std::vector<Item> high;
    for (uint64_t s : {1ull, 2ull, 3ull, 200ull}) high.push_back({"same", "v", tag((s << 40) | 7, 1)});
    check_table(high, 4096, 16, 0);
    check_table({{"a", "1", tag(5, 1)}, {std::string("a\x01\x05\0\0\0\0\0zz", 10), "2", tag(9, 1)},
                 {std::string("a\x01\x05", 3), "3", tag(1, 1)}}, 4096, 16, 2);
    check_table({{"dup", "same", tag(42, 1)}, {"dup", "same", tag(42, 1)}, {"dup", "same", tag(42, 1)},
                 {"dup", "", tag(42, 0)}, {"dup", "", tag(42, 0)}}, 4096, 16, 0);
    check_table({{"dup", "same", tag(42, 1)}, {"dup", "same", tag(42, 1)}, {"dup", "same", tag(42, 1)}}, 1, 16, 0);
    check_table({{"", "", tag(3, 1)}, {"", "", tag(2, 0)}, {"k", "", tag(1, 1)}, {"k", "", tag(9, 0)}, {"z", "val", tag(4, 1)}},
                4096, 16, 0);
    for (size_t w : {127, 128, 16383, 16384}) {
        const std::string base(w, 'P');
        check_table({{base + "a", "v", tag(1, 1)}, {base + "b", "w", tag(2, 1)}}, 1u << 20, 16, 0);
        check_table({{std::string(w - 8, 'K'), "v", tag(1, 1)}}, 1u << 20, 16, 0);
        check_table({{"k", std::string(w, 'V'), tag(1, 1)}, {"l", std::string(w, 'W'), tag(2, 1)}}, 1u << 20, 16, 1);
    }
    const std::vector<std::vector<std::string>> seps = {{"abc", "abcd"}, {"abcd", "abd"}, {"same", "same"},
                                                        {"ab\xffq", "ac"}, {"abc", "abd"}, {"abcd", "abz"}, {"a", "c"}};
    for (const auto &ks : seps) check_table({{ks[0], "v", tag(9, 1)}, {ks[1], "v", tag(8, 1)}}, 1, 16, 0);
    for (const std::string &k : {std::string(), std::string("\xff\xff\xff"), std::string("\xff\xff\x41\x42\x43"),
                                 std::string("k"), std::string("hello")})
        check_table({{k, "v", tag(1, 1)}}, 4096, 16, 0);
    // pseudo-random tables over small alphabets and small blocks
    for (int trial = 0; trial < 300; ++trial) {
        const unsigned sym = trial % 3 == 0 ? 2 : trial % 3 == 1 ? 4 : 256;
        const size_t n = rnd() % 150;
        std::vector<Item> items;
        for (size_t i = 0; i < n; ++i) {
            std::string k(rnd() % (trial % 2 ? 24 : 7), '\0');
            for (char &c : k) c = static_cast<char>(sym == 256 ? 250 + rnd() % 6 : rnd() % sym);
            const uint32_t type = rnd() % 4 ? 1 : 0;
            items.push_back({k, type ? std::string(rnd() % 40, 'v') : "", tag(rnd() % 6, type)});
        }
        const uint32_t bss[] = {1, 32, 64, 300, 4096};
        const uint32_t ris[] = {1, 2, 4, 16, 1024};
        check_table(items, bss[trial % 5], ris[(trial / 5) % 5], trial % 4);
    }
    // argument checks
    {
        lv_mt_totals mt{0, 0, 0};
        lv_sst_build_totals t{};
        const lv_sst_build_options bad[] = {{0, 16}, {(1u << 30) + 1, 16}, {4096, 0}, {4096, 1025}};
        for (const auto &o : bad) CHECK(lv_sst_build_host(nullptr, 0, nullptr, nullptr, &mt, &o, nullptr, 0, nullptr, 0, &t) != 0);
        CHECK(lv_sst_build_host(nullptr, 0, nullptr, nullptr, &mt, nullptr, nullptr, 0, nullptr, 0, nullptr) != 0);
        CHECK(lv_sst_build_host(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, &t) != 0);
        CHECK(lv_sst_build_host(nullptr, 0, nullptr, nullptr, &mt, nullptr, nullptr, 0, nullptr, 0, &t) == 0);
        CHECK(t.status == 0 && t.file_bytes == 0);
    }
    if (g_fail) {
        std::fprintf(stderr, "sst_host_check: %d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("sst_host_check: ok");
    return 0;
}
