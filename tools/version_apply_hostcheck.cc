// Stand-alone check of the version builder's host twin (lv_version_apply_host,
// csrc/version_set.cc) for sanitizer builds on the CPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tools/version_apply_hostcheck.cc leveldb-rs_amd/csrc/version_set.cc
//       -o version_apply_hostcheck && ./version_apply_hostcheck cases.bin
//
// tests/test_version_apply_hostcheck.py builds it this way and runs it over the
// dump tests/version_apply_cases.py writes (dump() there is the layout): the
// empty input, the worked example and its prefixes, random histories with and
// without a directory and with leading rows no record covers, and the damaged
// inputs -- bounds out of order or beyond the capacity, levels and numbers out
// of range, extents outside the source, short keys, duplicates, directories
// out of order -- each with the model's totals, rows and directory indices.
//
// Every input is a heap block of exactly its size, so a read one byte outside
// is a heap-buffer-overflow; every output lies between two guards of canary
// bytes.  A case is applied with the dump's files_cap and, when it has live
// files, once more with one row less (FILE_OVER, nothing written, the totals
// the true ones) and once without d_dir_index.  Exits 0 when everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lvgpu/crc32c.h"
#include "lvgpu/version_set.h"

namespace {

int g_fail = 0;
std::string g_case;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            if (g_fail < 50) std::fprintf(stderr, "%s:%d: %s: %s failed\n", __FILE__, __LINE__, g_case.c_str(), #cond); \
            ++g_fail;                                                                                        \
        }                                                                                                    \
    } while (0)

constexpr uint8_t kCanary = 0xA5;
constexpr size_t kGuard = 64;

// `bytes` output bytes between two guards, all canary; p() is the output.
struct Guarded {
    uint8_t *block;
    size_t bytes;
    explicit Guarded(size_t n) : block(static_cast<uint8_t *>(std::malloc(n + 2 * kGuard))), bytes(n) {
        std::memset(block, kCanary, n + 2 * kGuard);
    }
    ~Guarded() { std::free(block); }
    Guarded(const Guarded &) = delete;
    uint8_t *p() const { return block + kGuard; }
    bool guards_whole() const {
        for (size_t i = 0; i < kGuard; ++i)
            if (block[i] != kCanary || block[kGuard + bytes + i] != kCanary) return false;
        return true;
    }
    bool untouched() const {
        for (size_t i = 0; i < bytes; ++i)
            if (p()[i] != kCanary) return false;
        return guards_whole();
    }
};

// An input of exactly `bytes` bytes on the heap (null when empty).
struct Exact {
    uint8_t *p = nullptr;
    bool read(std::FILE *f, size_t bytes) {
        if (!bytes) return true;
        p = static_cast<uint8_t *>(std::malloc(bytes));
        return p && std::fread(p, 1, bytes, f) == bytes;
    }
    ~Exact() { std::free(p); }
    Exact() = default;
    Exact(const Exact &) = delete;
    template <class T>
    const T *as() const { return reinterpret_cast<const T *>(p); }
};

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    int cases = 0, refused = 0, overs = 0;
    uint64_t live_rows = 0;
    for (;;) {
        uint64_t h[8];
        const size_t got = std::fread(h, 1, sizeof h, f);
        if (got == 0) break;
        if (got != sizeof h) {
            std::fprintf(stderr, "truncated dump\n");
            return 2;
        }
        g_case = "case " + std::to_string(cases);
        const uint64_t src_bytes = h[0], records = h[1], nf = h[2], nd = h[3], np = h[4], dir_n = h[5], files_cap = h[6],
                       want_rows = h[7];
        Exact src, edits, files, bf, deleted, bd, pointers, bp, dir, want_t, want_r, want_i;
        const bool ok = src.read(f, src_bytes) && edits.read(f, records * sizeof(lv_ve_edit)) &&
                        files.read(f, nf * sizeof(lv_ve_file)) && bf.read(f, (records + 1) * 8) &&
                        deleted.read(f, nd * sizeof(lv_ve_deleted)) && bd.read(f, (records + 1) * 8) &&
                        pointers.read(f, np * sizeof(lv_ve_pointer)) && bp.read(f, (records + 1) * 8) &&
                        dir.read(f, dir_n * sizeof(lv_vs_placement)) && want_t.read(f, sizeof(lv_vs_totals)) &&
                        want_r.read(f, want_rows * sizeof(lv_version_file)) && want_i.read(f, want_rows * 4);
        if (!ok) {
            std::fprintf(stderr, "truncated dump in %s\n", g_case.c_str());
            return 2;
        }
        lv_ve_encode_in in{};
        in.d_edits = edits.as<lv_ve_edit>();
        in.d_files = files.as<lv_ve_file>();
        in.file_cap = nf;
        in.d_rec_file = bf.as<uint64_t>();
        in.d_deleted = deleted.as<lv_ve_deleted>();
        in.deleted_cap = nd;
        in.d_rec_deleted = bd.as<uint64_t>();
        in.d_pointers = pointers.as<lv_ve_pointer>();
        in.pointer_cap = np;
        in.d_rec_pointer = bp.as<uint64_t>();
        const lv_vs_totals &want = *want_t.as<lv_vs_totals>();

        auto apply = [&](uint64_t cap, bool with_index, lv_vs_totals *t, Guarded &rows, Guarded &index) {
            lv_vs_out out{};
            out.d_files_out = cap ? reinterpret_cast<lv_version_file *>(rows.p()) : nullptr;
            out.files_cap = cap;
            out.d_dir_index = with_index ? reinterpret_cast<uint32_t *>(index.p()) : nullptr;
            out.d_totals = t;
            return lv_version_apply_host(src.p, src_bytes, &in, records, dir.as<lv_vs_placement>(), dir_n, &out);
        };
        {
            Guarded rows(files_cap * sizeof(lv_version_file)), index(files_cap * 4);
            lv_vs_totals t;
            std::memset(&t, kCanary, sizeof t);
            CHECK(apply(files_cap, true, &t, rows, index) == 0);
            CHECK(std::memcmp(&t, &want, sizeof t) == 0);
            CHECK(rows.guards_whole() && index.guards_whole());
            if (want.status) {
                ++refused;
                CHECK(want_rows == 0 && rows.untouched() && index.untouched());
            } else {
                CHECK(want_rows == want.live);
                CHECK(!want_rows || std::memcmp(rows.p(), want_r.p, want_rows * sizeof(lv_version_file)) == 0);
                CHECK(!want_rows || std::memcmp(index.p(), want_i.p, want_rows * 4) == 0);
                for (size_t i = want_rows * sizeof(lv_version_file); i < rows.bytes; ++i) CHECK(rows.p()[i] == kCanary);
                live_rows += want_rows;
            }
        }
        if (!want.status && want.live) {
            {  // one row less: FILE_OVER, nothing written, the totals the true ones
                Guarded rows((want.live - 1) * sizeof(lv_version_file)), index((want.live - 1) * 4);
                lv_vs_totals t;
                CHECK(apply(want.live - 1, true, &t, rows, index) == 0);
                lv_vs_totals w = want;
                w.status = LV_VS_FILE_OVER;
                CHECK(std::memcmp(&t, &w, sizeof t) == 0);
                CHECK(rows.untouched() && index.untouched());
                ++overs;
            }
            {  // exactly the live rows, no d_dir_index
                Guarded rows(want.live * sizeof(lv_version_file)), index(0);
                lv_vs_totals t;
                CHECK(apply(want.live, false, &t, rows, index) == 0);
                CHECK(std::memcmp(&t, &want, sizeof t) == 0);
                CHECK(std::memcmp(rows.p(), want_r.p, want_rows * sizeof(lv_version_file)) == 0 && rows.guards_whole());
            }
        }
        ++cases;
    }
    std::fclose(f);
    std::printf("version_apply_hostcheck: %d cases replayed, %d refused, %d retried one row short, %llu live rows, %d failures\n",
                cases, refused, overs, static_cast<unsigned long long>(live_rows), g_fail);
    return g_fail ? 1 : 0;
}
