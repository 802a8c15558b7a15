// Stand-alone check of the SSTable reader's host twins (csrc/sst_get.cc, whose
// core csrc/lvk/sst_read.h is the text the kernels compile too) for sanitizer
// builds on the CPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tools/sst_get_host_check.cc leveldb-rs_amd/csrc/sst_get.cc leveldb-rs_amd/csrc/sst_build.cc
//       leveldb-rs_amd/csrc/sst_format.cc leveldb-rs_amd/csrc/memtable.cc leveldb-rs_amd/csrc/crc32c_scalar.cc
//       -o sst_get_host_check && ./sst_get_host_check [cases.bin]
//
// tests/test_host_checks.py builds it this way and runs it on the dump with
// the CPU suite.
//
// Every image, handle array and query key is a heap block of exactly its
// size, so a read one byte outside is a heap-buffer-overflow.  Three parts:
//   1. tables built by lv_sst_build_host (the corner shapes of the format and
//      pseudo-random ones over small blocks): lv_sst_open_host must return the
//      build's totals and handles, and lv_sst_get_host must agree with
//      lv_memtable_get_host on the same op table for every stored version
//      around its snapshot, for neighbours of every key and for the index keys;
//   2. a few thousand random single-byte and multi-byte flips anywhere in an
//      image, through lv_sst_open_host and through lv_sst_get_host with the
//      damaged image's own table and with the sound image's (a table the open
//      did not write for this file): whatever the bytes say, the answers stay
//      inside the file;
//   3. with a file argument, the cases python tests/sst_get_cases.py dump FILE
//      wrote (every open status, every deterministic get corruption, the flips
//      the GPU suite replays, with the Python model's expected outputs): the
//      same inputs the GPU tests use, run here first.
// Exits 0 when everything agrees.
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
            if (g_fail < 50) std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                        \
        }                                                                    \
    } while (0)

struct Item {
    std::string key, value;
    uint64_t tag;
};

uint64_t tag(uint64_t seq, uint32_t type) { return (seq << 8) | type; }

// a heap copy of exactly n bytes (NULL for none)
uint8_t *exact(const void *p, size_t n) {
    if (!n) return nullptr;
    uint8_t *q = static_cast<uint8_t *>(std::malloc(n));
    std::memcpy(q, p, n);
    return q;
}

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

int get(const uint8_t *file, const lv_sst_table &t, const std::string &key, uint64_t seq, lv_sst_get_result *r) {
    uint8_t *k = exact(key.data(), key.size());
    std::memset(r, 0xEE, sizeof *r);
    const int rc = lv_sst_get_host(file, &t, k, key.size(), seq, r);
    std::free(k);
    return rc;
}

// whatever the image says, an answer lies inside it
void check_sane(const lv_sst_get_result &r, uint64_t fb) {
    CHECK(r.status <= LV_SST_GET_CORRUPT && r.reserved == 0);
    if (r.status == LV_SST_GET_FOUND) CHECK(r.val_off <= fb && r.val_len <= fb - r.val_off);
    if (r.status != LV_SST_GET_FOUND) CHECK(r.val_off == 0 && r.val_len == 0);
    if (r.status != LV_SST_GET_FOUND && r.status != LV_SST_GET_DELETED) CHECK(r.tag == 0 && r.block == 0);
}

void fuzz(const uint8_t *image, uint64_t fb, const lv_sst_table &sound, const std::vector<std::string> &keys, int rounds) {
    for (int round = 0; round < rounds; ++round) {
        uint8_t *bad = exact(image, fb);
        const int flips = round % 2 ? 1 + static_cast<int>(rnd() % 4) : 1;
        for (int f = 0; f < flips; ++f) bad[rnd() % fb] = static_cast<uint8_t>(rnd());
        const uint64_t cut = round % 16 == 15 ? rnd() % (fb + 1) : fb;  // now and then a truncated file
        uint8_t *file = cut == fb ? bad : exact(bad, cut);
        const size_t cap = round % 3 ? sound.data_blocks : rnd() % (sound.data_blocks + 1);
        uint64_t *handles = static_cast<uint64_t *>(std::malloc(16 * (cap + 2)));
        lv_sst_table t;
        CHECK(lv_sst_open_host(file, cut, handles, cap, &t) == 0);
        CHECK(t.reserved == 0 && (t.status & ~63ull) == 0);
        if (!t.status)
            for (uint64_t i = 0; i < t.data_blocks + 2; ++i)
                CHECK(handles[2 * i] <= cut && handles[2 * i + 1] + 5 <= cut - handles[2 * i]);
        lv_sst_table foreign = sound;
        foreign.file_bytes = cut;
        for (size_t q = 0; q < 6; ++q) {
            const std::string &k = keys[rnd() % keys.size()];
            lv_sst_get_result r;
            CHECK(get(file, t, k, rnd() % 8, &r) == 0);
            check_sane(r, cut);
            CHECK(get(file, foreign, k, rnd() % 8, &r) == 0);
            check_sane(r, cut);
        }
        std::free(handles);
        if (file != bad) std::free(file);
        std::free(bad);
    }
}

void check_table(const std::vector<Item> &items, uint32_t bs, uint32_t ri, int fuzz_rounds) {
    std::string p;
    std::vector<lv_wb_op> ops;
    for (const Item &it : items) {
        lv_wb_op o{};
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
    const lv_sst_build_options opt{bs, ri};
    lv_sst_build_totals size{}, tot{};
    CHECK(lv_sst_build_host(payload, p.size(), ops.data(), order.data(), &mt, &opt, nullptr, 0, nullptr, 0, &size) == 0);
    uint8_t *file = static_cast<uint8_t *>(std::malloc(size.file_bytes ? size.file_bytes : 1));
    uint64_t *built = static_cast<uint64_t *>(std::malloc(16 * (size.data_blocks + 2)));
    CHECK(lv_sst_build_host(payload, p.size(), ops.data(), order.data(), &mt, &opt, size.file_bytes ? file : nullptr,
                            size.file_bytes, built, size.data_blocks, &tot) == 0);
    CHECK(tot.status == 0);
    const uint64_t fb = tot.file_bytes;
    // the open: the build's totals and handles
    uint64_t *handles = static_cast<uint64_t *>(std::malloc(16 * (tot.data_blocks + 2)));
    std::memset(handles, 0xA5, 16 * (tot.data_blocks + 2));
    lv_sst_table t;
    CHECK(lv_sst_open_host(fb ? file : nullptr, fb, handles, tot.data_blocks, &t) == 0);
    CHECK(t.status == 0 && t.file_bytes == fb && t.data_blocks == tot.data_blocks && t.reserved == 0);
    CHECK(t.metaindex_offset == tot.metaindex_offset && t.metaindex_size == tot.metaindex_size);
    CHECK(t.index_offset == tot.index_offset && t.index_size == tot.index_size);
    if (fb) CHECK(std::memcmp(handles, built, 16 * (tot.data_blocks + 2)) == 0);
    if (tot.data_blocks) {  // one handle short
        lv_sst_table over;
        uint64_t *fewer = static_cast<uint64_t *>(std::malloc(16 * (tot.data_blocks + 1)));
        std::memset(fewer, 0xA5, 16 * (tot.data_blocks + 1));
        CHECK(lv_sst_open_host(file, fb, fewer, tot.data_blocks - 1, &over) == 0);
        CHECK(over.status == LV_SST_OPEN_HANDLE_OVER && over.data_blocks == tot.data_blocks && fewer[0] == 0xA5A5A5A5A5A5A5A5ull);
        std::free(fewer);
        CHECK(lv_sst_open_host(file, fb, nullptr, 0, &over) == 0 && over.status == 0);
    }
    // the gets: the memtable's answers
    std::vector<std::pair<std::string, uint64_t>> qs;
    std::vector<std::string> keys;
    for (const Item &it : items) {
        const uint64_t seq = it.tag >> 8;
        for (uint64_t s : {seq - 1, seq, seq + 1, uint64_t{0}, uint64_t{LV_MT_MAX_SEQUENCE}})
            if (s <= LV_MT_MAX_SEQUENCE) qs.emplace_back(it.key, s);
        std::string k = it.key;
        qs.emplace_back(k + std::string(1, '\0'), LV_MT_MAX_SEQUENCE);
        if (!k.empty()) {
            qs.emplace_back(k.substr(0, k.size() - 1), LV_MT_MAX_SEQUENCE);
            k.back() = static_cast<char>(k.back() + 1);
            qs.emplace_back(k, LV_MT_MAX_SEQUENCE);
            k.back() = static_cast<char>(k.back() - 2);
            qs.emplace_back(k, 3);
        }
        keys.push_back(it.key);
    }
    qs.emplace_back("", LV_MT_MAX_SEQUENCE);
    qs.emplace_back("\xff\xff\xff\xff", 1);
    keys.push_back("");
    for (const auto &q : qs) {
        lv_sst_get_result r;
        lv_mt_get_result m;
        CHECK(get(file, t, q.first, q.second, &r) == 0);
        uint8_t *k = exact(q.first.data(), q.first.size());
        CHECK(lv_memtable_get_host(payload, p.size(), ops.data(), order.data(), &mt, k, q.first.size(), q.second, &m) == 0);
        std::free(k);
        check_sane(r, fb);
        CHECK(r.status == m.status);
        if (r.status == m.status && (r.status == LV_SST_GET_FOUND || r.status == LV_SST_GET_DELETED)) {
            CHECK(r.tag == ops[m.op].tag && r.block < tot.data_blocks && r.val_len == m.val_len);
            CHECK(r.val_len == 0 || std::memcmp(file + r.val_off, payload + m.val_off, r.val_len) == 0);
        }
    }
    lv_sst_get_result r;
    CHECK(get(file, t, "k", LV_MT_MAX_SEQUENCE + 1, &r) == 0 && r.status == LV_SST_GET_BAD_SEQ);
    lv_sst_table failed = t;
    failed.status = LV_SST_OPEN_BAD_INDEX;
    CHECK(get(file, failed, "k", 1, &r) == 0 && r.status == LV_SST_GET_NO_TABLE && r.tag == 0);
    if (fb && fuzz_rounds) fuzz(file, fb, t, keys, fuzz_rounds);
    std::free(handles);
    std::free(built);
    std::free(file);
    std::free(payload);
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

// ---- the dumped cases (tests/sst_get_cases.py dump) ----
struct In {
    std::vector<uint8_t> b;
    size_t at = 0;
    bool ok = true;
    uint64_t u64() {
        uint64_t v = 0;
        if (at + 8 > b.size()) return ok = false, 0;
        std::memcpy(&v, b.data() + at, 8);
        at += 8;
        return v;
    }
    const uint8_t *bytes(size_t n) {
        if (at + n > b.size()) return ok = false, nullptr;
        at += n;
        return b.data() + at - n;
    }
};

int replay(const char *path) {
    In in;
    FILE *f = std::fopen(path, "rb");
    if (!f) return std::fprintf(stderr, "cannot open %s\n", path), 1;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) in.b.insert(in.b.end(), buf, buf + n);
    std::fclose(f);
    const uint64_t cases = in.u64();
    uint64_t queries = 0;
    for (uint64_t c = 0; c < cases && in.ok; ++c) {
        const uint64_t fb = in.u64();
        uint8_t *file = exact(in.bytes(fb), fb);
        const uint64_t with_handles = in.u64(), cap = in.u64();
        lv_sst_table want{}, t;
        std::memcpy(&want, in.bytes(sizeof want), sizeof want);
        const uint64_t nh = in.u64();  // pairs expected, ~0: none written
        uint64_t *handles = with_handles ? static_cast<uint64_t *>(std::malloc(16 * (cap + 2))) : nullptr;
        if (handles) std::memset(handles, 0xA5, 16 * (cap + 2));
        CHECK(lv_sst_open_host(file, fb, handles, cap, &t) == 0);
        CHECK(std::memcmp(&t, &want, sizeof t) == 0);
        const uint64_t written = nh == ~0ull ? 0 : nh;
        const uint8_t *wh = in.bytes(16 * written);
        if (handles) {
            CHECK(written <= cap + 2 && std::memcmp(handles, wh, 16 * written) == 0);
            for (uint64_t i = 2 * written; i < 2 * (cap + 2); ++i) CHECK(handles[i] == 0xA5A5A5A5A5A5A5A5ull);
        }
        lv_sst_table use{};
        std::memcpy(&use, in.bytes(sizeof use), sizeof use);  // the table the gets go by
        const uint64_t nq = in.u64();
        for (uint64_t q = 0; q < nq && in.ok; ++q) {
            const uint64_t kl = in.u64();
            const std::string key(reinterpret_cast<const char *>(in.bytes(kl)), kl);
            const uint64_t seq = in.u64();
            lv_sst_get_result want_r{}, r;
            std::memcpy(&want_r, in.bytes(sizeof want_r), sizeof want_r);
            CHECK(get(file, use, key, seq, &r) == 0);
            CHECK(std::memcmp(&r, &want_r, sizeof r) == 0);
            ++queries;
        }
        std::free(handles);
        std::free(file);
    }
    CHECK(in.ok && in.at == in.b.size());
    std::printf("sst_get_host_check: replayed %llu cases, %llu queries\n", static_cast<unsigned long long>(cases),
                static_cast<unsigned long long>(queries));
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    for (size_t n : {0, 1, 15, 16, 17, 32, 33}) check_table(seq_items(n), 4096, 16, 20);
    check_table(seq_items(40), 64, 4, 600);
    check_table(seq_items(40), 1, 1, 300);
    check_table({{"a", "s", tag(1, 1)}, {"big", std::string(9000, 'B'), tag(2, 1)}, {"c", "t", tag(3, 1)}}, 4096, 16, 50);
    std::vector<Item> high;
    for (uint64_t s : {1ull, 2ull, 3ull, 200ull}) high.push_back({"same", "v", tag((s << 40) | 7, 1)});
    for (uint32_t ri : {16u, 1u}) check_table(high, 4096, ri, 100);
    check_table(high, 1, 16, 100);
    const std::vector<Item> into = {{"a", "1", tag(5, 1)}, {std::string("a\x01\x05\0\0\0\0\0zz", 10), "2", tag(9, 1)},
                                    {std::string("a\x01\x05", 3), "3", tag(1, 1)}};
    for (uint32_t ri : {16u, 1u}) check_table(into, 4096, ri, 100);
    check_table({{"dup", "same", tag(42, 1)}, {"dup", "same", tag(42, 1)}, {"dup", "same", tag(42, 1)},
                 {"dup", "", tag(42, 0)}, {"dup", "", tag(42, 0)}}, 4096, 16, 50);
    check_table({{"", "", tag(3, 1)}, {"", "", tag(2, 0)}, {"k", "", tag(1, 1)}, {"k", "", tag(9, 0)}, {"z", "val", tag(4, 1)}},
                4096, 16, 50);
    std::vector<Item> versions;
    for (uint64_t s = 2; s < 40; s += 3) versions.push_back({"same", "v", tag(s, s % 4 ? 1 : 0)});
    check_table(versions, 1, 16, 100);
    for (size_t w : {127, 128, 16383, 16384}) {
        const std::string base(w, 'P');
        check_table({{base + "a", "v", tag(1, 1)}, {base + "b", "w", tag(2, 1)}}, 1u << 20, 16, 10);
        check_table({{"k", std::string(w, 'V'), tag(1, 1)}, {"l", std::string(w, 'W'), tag(2, 1)}}, 1u << 20, 16, 10);
    }
    const std::vector<std::vector<std::string>> seps = {{"abc", "abcd"}, {"abcd", "abd"}, {"same", "same"},
                                                        {"ab\xffq", "ac"}, {"abc", "abd"}, {"abcd", "abz"}, {"a", "c"}};
    for (const auto &ks : seps) check_table({{ks[0], "v", tag(9, 1)}, {ks[1], "v", tag(8, 1)}}, 1, 16, 20);
    {  // a 5,000-byte shared stem with 1-byte differences
        std::string stem(4999, '\0');
        for (size_t i = 0; i < stem.size(); ++i) stem[i] = static_cast<char>(i);
        std::vector<Item> items;
        for (int c = 1; c < 40; ++c) items.push_back({stem + static_cast<char>(c), "v", tag(10 + c, 1)});
        items.push_back({stem, "stem", tag(5, 1)});
        check_table(items, 4096, 16, 20);
        check_table(items, 1u << 20, 1024, 20);
    }
    // pseudo-random tables over small alphabets and small blocks
    for (int trial = 0; trial < 200; ++trial) {
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
        check_table(items, bss[trial % 5], ris[(trial / 5) % 5], 15);
    }
    if (argc > 1 && replay(argv[1])) return 1;
    if (g_fail) {
        std::fprintf(stderr, "sst_get_host_check: %d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("sst_get_host_check: ok");
    return 0;
}
