// Stand-alone check of the host WAL layout (leveldb-rs_amd/csrc/wal_layout.cc)
// for sanitizer builds: lv_wal_encode_size and wal_layout over the record
// lists of tests/test_wal_encode_size.py, with the layout's invariants
// asserted.  No GPU, no HIP:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/wal_layout_check.cc leveldb-rs_amd/csrc/wal_layout.cc -o wal_layout_check && ./wal_layout_check
// tests/test_host_checks.py builds it this way and runs it with the CPU suite.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/lvgpu/wal.h"
#include "../leveldb-rs_amd/csrc/lv_internal.h"

namespace {

constexpr uint64_t B = LV_WAL_BLOCK_SIZE, H = LV_WAL_HEADER_SIZE;
long g_checked = 0;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

void check(const std::vector<uint64_t> &len, uint64_t dest) {
    std::vector<uint64_t> off(len.size());
    uint64_t tot = 0;
    for (size_t i = 0; i < len.size(); ++i) {
        off[i] = tot;
        tot += len[i];
    }
    size_t frags = ~size_t{0};
    const size_t bytes = lv_wal_encode_size(len.data(), len.size(), dest, &frags);
    CHECK(lv_wal_encode_size(len.data(), len.size(), dest, nullptr) == bytes);
    lvgpu_internal::WalLayout lay;
    lvgpu_internal::wal_layout(off.data(), len.data(), len.size(), dest, true, &lay);
    CHECK(lay.out_len == bytes && lay.fragments == frags && lay.frags.size() == frags);
    const uint64_t first = dest % B;
    uint64_t pos = 0, payload = 0, pad = 0;
    size_t pi = 0;
    for (size_t i = 0; i < frags; ++i) {
        const lvgpu_internal::WalFrag &f = lay.frags[i];
        if (pi < lay.pads.size() && lay.pads[pi].first == pos) {  // a zero trailer ends its block
            CHECK(lay.pads[pi].second < H && (first + pos + lay.pads[pi].second) % B == 0);
            pos += lay.pads[pi].second;
            pad += lay.pads[pi++].second;
        }
        CHECK(f.out_pos == pos && f.type >= 1 && f.type <= 4);
        CHECK((first + pos) / B == (first + pos + H + f.len - 1) / B);  // never straddles a block
        pos += H + f.len;
        payload += f.len;
    }
    CHECK(pi == lay.pads.size() && pos == bytes && payload == tot && bytes == frags * H + tot + pad);
    if (len.empty()) {
        CHECK(lay.block_first.empty() && bytes == 0);
    } else {
        const uint64_t nblocks = (first + bytes + B - 1) / B;
        CHECK(lay.block_first.size() == nblocks + 1 && lay.block_first[0] == 0 && lay.block_first[nblocks] == frags);
        for (uint64_t k = 0; k < nblocks; ++k) {
            CHECK(lay.block_first[k] <= lay.block_first[k + 1]);
            for (uint64_t i = lay.block_first[k]; i < lay.block_first[k + 1]; ++i)
                CHECK((first + lay.frags[i].out_pos) / B == k);
        }
    }
    ++g_checked;
}

}  // namespace

int main() {
    const uint64_t dests[] = {0, 1, B - H - 1, B - H, B - H + 1, B - 1, B, 5 * B + 17};
    uint64_t x = 88172645463325252ull;  // xorshift64: skewed lengths like the tests' recipe
    auto rnd = [&] {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (uint64_t dest : dests) {
        check({}, dest);
        check(std::vector<uint64_t>(5, 0), dest);
        std::vector<uint64_t> recipe{0, 3};
        for (int i = 0; i < 200; ++i) recipe.push_back(rnd() % (1ull << (rnd() % 18)));
        recipe.push_back(3 * B + 5);
        recipe.push_back(0);
        check(recipe, dest);
        for (uint64_t k = 0; k <= 8; ++k) {
            uint64_t bo = dest % B;
            if (B - bo < H) bo = 0;
            uint64_t firstlen = B - bo - H >= k ? B - bo - H - k : (B - bo - H) + (B - H - k);
            check({firstlen, 0, 1, 2 * B + 3}, dest);
        }
        check(std::vector<uint64_t>(20000, 1), dest);
    }
    CHECK(lv_wal_encode_size(nullptr, 0, 0, nullptr) == 0);
    std::printf("wal_layout_check: %ld layouts ok\n", g_checked);
    return 0;
}
