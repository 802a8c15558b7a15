// Stand-alone check of the compaction output's host twin (csrc/compact_output.cc)
// for sanitizer builds on the CPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tools/compact_output_hostcheck.cc leveldb-rs_amd/csrc/compact_output.cc leveldb-rs_amd/csrc/sst_build.cc
//       leveldb-rs_amd/csrc/sst_get.cc leveldb-rs_amd/csrc/sst_format.cc leveldb-rs_amd/csrc/version.cc
//       leveldb-rs_amd/csrc/memtable.cc leveldb-rs_amd/csrc/crc32c_scalar.cc
//       -o compact_output_hostcheck && ./compact_output_hostcheck cases.bin
//
// tests/test_compact_output_hostcheck.py builds it this way and runs it over the
// dump tests/compact_output_cases.py writes (its dump() documents the layout):
// the inputs the CPU and GPU tests use, capacities one short of the counts for
// every status, an upstream status, hostile ops and order indices that point
// outside the payload and the op table (NO_TABLE), and a value of 2^32 - 1
// bytes claimed inside a payload that is larger than the bytes dumped
// (BLOCK_LARGE with ARENA_OVER: decided from sizes, so no byte of it is read,
// which the exact-size heap block of the payload proves).
//
// Every input is a heap block of exactly its size, so a read one byte outside
// is a heap-buffer-overflow.  Every output lies between two guards of canary
// bytes inside its heap block and is filled with the canary first: after the
// call the guards must be whole, with a status every output byte must still
// be the canary, and with status 0 so must every byte outside the ranges the
// totals report (behind arena_bytes, in the gaps between two files, behind
// the handle pairs, the records of `files` files and the bound keys).  With
// status 0 every file is then held to the twins that define it: the slice rule
// (lv_sst_build_host / lv_sst_build_bloom_host over the order slice) and the
// records (lv_sst_open_host, lv_sst_bloom_open_host, lv_version_file_host).
// Exits 0 when everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lvgpu/compact.h"
#include "lvgpu/crc32c.h"

// (sst_format.cc reports its errors through lvgpu_internal::set_error, which
// lives in a HIP unit; this file supplies a stub.)
namespace lvgpu_internal {
int set_error(int code, const char *) { return code; }
}  // namespace lvgpu_internal

namespace {

int g_fail = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            if (g_fail < 50) std::fprintf(stderr, "%s:%d: %s: %s failed\n", __FILE__, __LINE__, g_case.c_str(), #cond); \
            ++g_fail;                                                                                        \
        }                                                                                                    \
    } while (0)

std::string g_case;
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
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p()); }
    bool canary(size_t from, size_t to) const {  // output bytes [from, to)
        for (size_t i = from; i < to; ++i)
            if (p()[i] != kCanary) return false;
        return true;
    }
    bool guards() const {
        for (size_t i = 0; i < kGuard; ++i)
            if (block[i] != kCanary || block[kGuard + bytes + i] != kCanary) return false;
        return true;
    }
};

template <class T>
T *exact(const T *p, size_t count) {  // a heap copy of exactly count elements (NULL for none)
    if (!count) return nullptr;
    T *q = static_cast<T *>(std::malloc(count * sizeof(T)));
    std::memcpy(q, p, count * sizeof(T));
    return q;
}

struct Reader {
    const std::vector<uint8_t> &b;
    size_t at = 0;
    bool ok = true;
    const uint8_t *take(size_t n) {
        if (n > b.size() - at) {
            ok = false;
            return nullptr;
        }
        const uint8_t *p = b.data() + at;
        at += n;
        return p;
    }
    uint64_t u(size_t n) {
        const uint8_t *p = take(n);
        uint64_t v = 0;
        for (size_t i = 0; p && i < n; ++i) v |= static_cast<uint64_t>(p[i]) << (8 * i);
        return v;
    }
};

struct Case {
    uint8_t *payload = nullptr;
    lv_wb_op *ops = nullptr;
    uint32_t *order = nullptr;
    size_t payload_alloc = 0, n_ops = 0, n = 0;
    uint64_t payload_bytes = 0, mf = 0;
    lv_mt_totals mt{};
    lv_sst_build_options opt{};
    lv_sst_bloom_options bloom{};
    bool has_caps = false;
    uint64_t caps[4] = {};
    ~Case() {
        std::free(payload);
        std::free(ops);
        std::free(order);
    }
};

constexpr uint64_t kUsed = 3, kNumber = 9, kImagesOff = 4096;
constexpr uint32_t kLevel = 4;

int run(const Case &c, uint8_t *arena, uint64_t arena_cap, uint64_t *handles, size_t block_cap,
        lv_compact_output_file *files, lv_sst_table *tables, lv_sst_bloom *blooms, lv_version_file *vfiles, size_t files_cap,
        uint8_t *keys, uint64_t keys_cap, uint64_t *used, lv_compact_output_totals *t) {
    return lv_compact_output_host(c.payload, c.payload_bytes, c.ops, c.order, &c.mt, c.n_ops, &c.opt,
                                  c.bloom.bits_per_key ? &c.bloom : nullptr, c.mf, kNumber, kLevel, kImagesOff, arena,
                                  arena_cap, handles, block_cap, files, tables, blooms, vfiles, files_cap, keys, keys_cap,
                                  used, t);
}

void check_case(const Case &c, long *written, long *large) {
    const uint64_t extra = c.bloom.bits_per_key ? 3 : 2;
    lv_compact_output_totals sized{};
    lv_version_file probe{};  // (non-NULL: the bound bytes are counted)
    CHECK(run(c, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, &probe, 0, nullptr, 0, nullptr, &sized) == 0);
    uint64_t acap = sized.arena_bytes, bcap = sized.data_blocks, fcap = sized.files, kcap = kUsed + sized.bound_bytes;
    if (c.has_caps) acap = c.caps[0], bcap = c.caps[1], fcap = c.caps[2], kcap = kUsed + c.caps[3];
    Guarded arena(acap), handles(16 * (bcap + 3 * fcap)), files(64 * fcap), tables(64 * fcap), blooms(64 * fcap),
        vfiles(64 * fcap), keys(kcap);
    uint64_t used = kUsed;
    lv_compact_output_totals t{};
    CHECK(run(c, acap ? arena.p() : nullptr, acap, handles.as<uint64_t>(), bcap, files.as<lv_compact_output_file>(),
              tables.as<lv_sst_table>(), blooms.as<lv_sst_bloom>(), vfiles.as<lv_version_file>(), fcap, keys.p(), kcap,
              &used, &t) == 0);
    for (const Guarded *g : {&arena, &handles, &files, &tables, &blooms, &vfiles, &keys}) CHECK(g->guards());
    // a sizing pass judges no capacity: NO_TABLE alone, BLOCK_LARGE alone, or nothing
    CHECK(sized.status == 0 || sized.status == LV_COMPACT_OUT_NO_TABLE || sized.status == LV_COMPACT_OUT_BLOCK_LARGE);
    if (sized.status & LV_COMPACT_OUT_NO_TABLE) {  // nothing is counted
        CHECK(t.status == LV_COMPACT_OUT_NO_TABLE);
        CHECK(!t.entries && !t.files && !t.data_blocks && !t.arena_bytes && !t.handle_pairs && !t.bound_bytes);
    } else {
        CHECK(t.entries == sized.entries && t.files == sized.files && t.data_blocks == sized.data_blocks &&
              t.arena_bytes == sized.arena_bytes && t.handle_pairs == sized.handle_pairs &&
              t.bound_bytes == sized.bound_bytes && t.handle_pairs == t.data_blocks + extra * t.files);
        uint64_t want = sized.status;  // BLOCK_LARGE stays, with the true counts, beside the capacities' bits
        if (sized.status) {
            ++*large;
            CHECK(t.arena_bytes > 0xffffffffull && t.files >= 2);  // the large block closed its file: another follows
        }
        if (t.data_blocks > bcap) want |= LV_COMPACT_OUT_HANDLE_OVER;
        if (t.arena_bytes > acap) want |= LV_COMPACT_OUT_ARENA_OVER;
        if (t.files > fcap) want |= LV_COMPACT_OUT_FILES_OVER;
        if (t.entries && t.bound_bytes > kcap - kUsed) want |= LV_COMPACT_OUT_BOUND_OVER;
        CHECK(t.status == want);
    }
    if (t.status) {
        for (const Guarded *g : {&arena, &handles, &files, &tables, &blooms, &vfiles, &keys}) CHECK(g->canary(0, g->bytes));
        CHECK(used == kUsed);
        return;
    }
    ++*written;
    // nothing outside the reported ranges
    CHECK(arena.canary(t.arena_bytes, arena.bytes) && handles.canary(16 * t.handle_pairs, handles.bytes));
    for (const Guarded *g : {&files, &tables, &blooms, &vfiles}) CHECK(g->canary(64 * t.files, g->bytes));
    CHECK(used == kUsed + t.bound_bytes && keys.canary(0, kUsed) && keys.canary(used, keys.bytes));
    uint64_t off = 0, pair = 0, entry = 0, cursor = kUsed;
    Guarded keys2(kcap);
    for (uint64_t k = 0; k < t.files; ++k) {
        const lv_compact_output_file &f = files.as<lv_compact_output_file>()[k];
        CHECK(f.file_off == off && f.first_handle == pair && f.first_entry == entry && f.entries >= 1 && !f.reserved);
        CHECK(f.file_off % 16 == 0 && f.file_off + f.file_bytes <= t.arena_bytes);
        if (k) {  // the gap behind the file before is never written
            const lv_compact_output_file &p = files.as<lv_compact_output_file>()[k - 1];
            CHECK(off - (p.file_off + p.file_bytes) < 16 && arena.canary(p.file_off + p.file_bytes, off));
        }
        // the slice rule
        lv_mt_totals smt{f.entries, 0, 0};
        lv_sst_build_totals bt{};
        lv_sst_bloom_totals ft{};
        uint32_t *slice = exact(c.order + f.first_entry, f.entries);
        Guarded image(f.file_bytes), hs(16 * (f.data_blocks + extra));
        const int rc = c.bloom.bits_per_key
                           ? lv_sst_build_bloom_host(c.payload, c.payload_bytes, c.ops, slice, &smt, &c.opt, &c.bloom, image.p(),
                                                     f.file_bytes, hs.as<uint64_t>(), f.data_blocks, &bt, &ft)
                           : lv_sst_build_host(c.payload, c.payload_bytes, c.ops, slice, &smt, &c.opt, image.p(), f.file_bytes,
                                               hs.as<uint64_t>(), f.data_blocks, &bt);
        std::free(slice);
        CHECK(rc == 0 && !bt.status && bt.file_bytes == f.file_bytes && bt.data_blocks == f.data_blocks);
        CHECK(!std::memcmp(image.p(), arena.p() + off, f.file_bytes));
        CHECK(!std::memcmp(hs.p(), handles.p() + 16 * pair, 16 * (f.data_blocks + extra)));
        CHECK(f.filter_keys == (c.bloom.bits_per_key ? ft.filter_keys : 0));
        // the records
        lv_sst_table tb{};
        lv_sst_bloom bl{};
        lv_version_file vf{};
        CHECK(lv_sst_open_host(image.p(), f.file_bytes, nullptr, 0, &tb) == 0 && !tb.status);
        CHECK(!std::memcmp(&tb, &tables.as<lv_sst_table>()[k], sizeof tb));
        CHECK(lv_sst_bloom_open_host(image.p(), &tb, &bl) == 0 && bl.present == (c.bloom.bits_per_key ? 1u : 0u));
        CHECK(!std::memcmp(&bl, &blooms.as<lv_sst_bloom>()[k], sizeof bl));
        CHECK(lv_version_file_host(arena.p(), acap, off, f.file_bytes, &tb, kNumber + k, kLevel, keys2.p(), kcap, &cursor,
                                   &vf) == 0 && !vf.status);
        vf.file_off += kImagesOff;
        CHECK(!std::memcmp(&vf, &vfiles.as<lv_version_file>()[k], sizeof vf));
        pair += f.data_blocks + extra;
        entry += f.entries;
        off = (off + f.file_bytes + 15) & ~15ull;
    }
    CHECK(entry == t.entries && pair == t.handle_pairs && cursor == used);
    CHECK(!std::memcmp(keys2.p(), keys.p(), kcap));
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s cases.bin (tests/compact_output_cases.py: dump)\n", argv[0]);
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    std::vector<uint8_t> bytes;
    uint8_t buf[65536];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + got);
    std::fclose(f);
    Reader r{bytes};
    const uint64_t cases = r.u(4);
    long replayed = 0, written = 0, statuses = 0, large = 0;
    for (uint64_t i = 0; i < cases && r.ok; ++i) {
        Case c;
        const size_t nl = r.u(4);
        const uint8_t *nm = r.take(nl);
        if (!nm) break;
        g_case.assign(reinterpret_cast<const char *>(nm), nl);
        c.payload_alloc = r.u(8);
        c.payload = exact(r.take(c.payload_alloc), r.ok ? c.payload_alloc : 0);
        c.n_ops = r.u(4);
        c.ops = exact(reinterpret_cast<const lv_wb_op *>(r.take(32 * c.n_ops)), r.ok ? c.n_ops : 0);
        c.n = r.u(4);
        c.order = exact(reinterpret_cast<const uint32_t *>(r.take(4 * c.n)), r.ok ? c.n : 0);
        c.mt.entries = c.n;
        c.mt.status = r.u(8);
        c.payload_bytes = r.u(8);
        c.opt.block_size = static_cast<uint32_t>(r.u(4));
        c.opt.restart_interval = static_cast<uint32_t>(r.u(4));
        c.bloom.bits_per_key = static_cast<uint32_t>(r.u(4));
        c.mf = r.u(8);
        c.has_caps = r.u(4) != 0;
        for (uint64_t &cap : c.caps) cap = r.u(8);
        if (!r.ok || c.payload_bytes < c.payload_alloc) break;
        const long before = written;
        check_case(c, &written, &large);
        statuses += written == before;
        ++replayed;
    }
    if (!r.ok || replayed != static_cast<long>(cases) || r.at != bytes.size()) {
        std::fprintf(stderr, "%s: malformed dump\n", argv[1]);
        return 2;
    }
    std::printf("compact_output_hostcheck: %ld cases replayed, %ld written, %ld with a status or empty, %ld BLOCK_LARGE, "
                "%d failures\n",
                replayed, written, statuses, large, g_fail);
    return g_fail ? 1 : 0;
}
