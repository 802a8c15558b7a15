// Stand-alone check of the VersionEdit host twins (lv_version_edit_decode_host,
// lv_version_edit_encode_host, csrc/version_edit.cc) for sanitizer builds on
// the CPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tools/version_edit_hostcheck.cc leveldb-rs_amd/csrc/version_edit.cc
//       -o version_edit_hostcheck && ./version_edit_hostcheck cases.bin
//
// tests/test_version_edit_hostcheck.py builds it this way and runs it over the
// dump tests/version_edit_cases.py writes (dump_cases() there is the layout):
// records with the model's answer -- the worked example, its 55 prefixes and
// its single-byte flips, the quirks, every status, random edits -- and encode
// inputs with the model's verdict and bytes, among them damaged ones (bounds
// out of order or beyond the capacity, extents outside the source, bad levels
// and has bits, deleted rows out of order).
//
// Every input is a heap block of exactly its size, so a read one byte outside
// is a heap-buffer-overflow; every output lies between two guards of canary
// bytes.  A record is decoded three times: counting (no tables), with exactly
// the rows' capacities, and with one row less of each kind; an encode input is
// sized without a source, encoded into exactly out_bytes, and refused with one
// byte less (OUT_OVER, nothing written).  Exits 0 when everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lvgpu/crc32c.h"
#include "lvgpu/version_edit.h"

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

// An input of exactly n bytes on the heap (a one-byte block for n = 0, never read).
struct Exact {
    uint8_t *p;
    size_t n;
    Exact(const uint8_t *src, size_t len) : p(static_cast<uint8_t *>(std::malloc(len ? len : 1))), n(len) {
        if (len) std::memcpy(p, src, len);
    }
    ~Exact() { std::free(p); }
    Exact(const Exact &) = delete;
    template <class T>
    const T *as() const { return reinterpret_cast<const T *>(p); }
};

struct Reader {
    const std::vector<uint8_t> &d;
    size_t at = 0;
    bool ok = true;
    uint64_t u64() {
        if (at + 8 > d.size()) {
            ok = false;
            return 0;
        }
        uint64_t v;
        std::memcpy(&v, d.data() + at, 8);
        at += 8;
        return v;
    }
    std::vector<uint8_t> blob() {
        const uint64_t n = u64();
        if (!ok || n > d.size() - at) {
            ok = false;
            return {};
        }
        std::vector<uint8_t> b(d.begin() + at, d.begin() + at + n);
        at += (n + 7) & ~static_cast<uint64_t>(7);
        return b;
    }
};

size_t min_sz(size_t a, size_t b) { return a < b ? a : b; }

// memcmp == 0, for n that may be 0 with pointers that may then be null.
bool same(const void *a, const void *b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

void decode_case(Reader &R) {
    const std::vector<uint8_t> rec = R.blob();
    const uint32_t want_status = static_cast<uint32_t>(R.u64());
    const std::vector<uint8_t> edit = R.blob(), F = R.blob(), D = R.blob(), P = R.blob();
    if (!R.ok) return;
    CHECK(edit.size() == sizeof(lv_ve_edit));
    const size_t want[3] = {F.size() / sizeof(lv_ve_file), D.size() / sizeof(lv_ve_deleted), P.size() / sizeof(lv_ve_pointer)};
    const Exact in(rec.data(), rec.size());
    // counting: no tables
    size_t counts[3] = {99, 99, 99};
    CHECK(lv_version_edit_decode_host(in.p, in.n, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, counts) == want_status);
    CHECK(counts[0] == want[0] && counts[1] == want[1] && counts[2] == want[2]);
    CHECK(lv_version_edit_decode_host(in.p, in.n, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr) == want_status);
    // exactly the capacities, then one row less of each kind
    for (size_t less = 0; less < 2; ++less) {
        const size_t cap[3] = {want[0] - min_sz(less, want[0]), want[1] - min_sz(less, want[1]), want[2] - min_sz(less, want[2])};
        Guarded e(sizeof(lv_ve_edit)), f(cap[0] * sizeof(lv_ve_file)), d(cap[1] * sizeof(lv_ve_deleted)),
            p(cap[2] * sizeof(lv_ve_pointer));
        size_t c[3] = {99, 99, 99};
        const uint32_t st = lv_version_edit_decode_host(in.p, in.n, reinterpret_cast<lv_ve_edit *>(e.p()),
                                                        reinterpret_cast<lv_ve_file *>(f.p()), cap[0],
                                                        reinterpret_cast<lv_ve_deleted *>(d.p()), cap[1],
                                                        reinterpret_cast<lv_ve_pointer *>(p.p()), cap[2], c);
        CHECK(st == want_status && st <= LV_VE_BAD_LEVEL);
        CHECK(c[0] == want[0] && c[1] == want[1] && c[2] == want[2]);
        CHECK(e.guards_whole() && f.guards_whole() && d.guards_whole() && p.guards_whole());
        CHECK(same(e.p(), edit.data(), sizeof(lv_ve_edit)));
        CHECK(same(f.p(), F.data(), f.bytes) && same(d.p(), D.data(), d.bytes) &&
              same(p.p(), P.data(), p.bytes));
        const lv_ve_edit *ed = reinterpret_cast<const lv_ve_edit *>(e.p());
        CHECK(ed->status == st && ed->reserved == 0);
        if (st != LV_VE_OK) CHECK(ed->has == 0 && ed->flags == 0 && c[0] + c[1] + c[2] == 0);
    }
}

bool encode_case(Reader &R) {
    const std::vector<uint8_t> src = R.blob();
    const size_t records = R.u64();
    const std::vector<uint8_t> E = R.blob(), F = R.blob();
    const size_t file_cap = R.u64();
    const std::vector<uint8_t> bf = R.blob(), D = R.blob();
    const size_t deleted_cap = R.u64();
    const std::vector<uint8_t> bd = R.blob(), P = R.blob();
    const size_t pointer_cap = R.u64();
    const std::vector<uint8_t> bp = R.blob(), totals = R.blob(), out = R.blob(), ro = R.blob(), rl = R.blob();
    if (!R.ok) return false;
    CHECK(totals.size() == sizeof(lv_ve_encode_totals));
    lv_ve_encode_totals want;
    std::memcpy(&want, totals.data(), sizeof want);
    const Exact xs(src.data(), src.size()), xe(E.data(), E.size()), xf(F.data(), F.size()), xbf(bf.data(), bf.size()),
        xd(D.data(), D.size()), xbd(bd.data(), bd.size()), xp(P.data(), P.size()), xbp(bp.data(), bp.size());
    lv_ve_encode_in in{};
    in.d_edits = xe.as<lv_ve_edit>();
    in.d_files = xf.n ? xf.as<lv_ve_file>() : nullptr;
    in.file_cap = file_cap;
    in.d_rec_file = xbf.as<uint64_t>();
    in.d_deleted = xd.n ? xd.as<lv_ve_deleted>() : nullptr;
    in.deleted_cap = deleted_cap;
    in.d_rec_deleted = xbd.as<uint64_t>();
    in.d_pointers = xp.n ? xp.as<lv_ve_pointer>() : nullptr;
    in.pointer_cap = pointer_cap;
    in.d_rec_pointer = xbp.as<uint64_t>();
    CHECK(xf.n >= file_cap * sizeof(lv_ve_file) && xd.n >= deleted_cap * sizeof(lv_ve_deleted) &&
          xp.n >= pointer_cap * sizeof(lv_ve_pointer) && xbf.n == (records + 1) * 8);
    // sizing: no source, no output
    {
        Guarded off(records * 8), len(records * 8), tot(sizeof(lv_ve_encode_totals));
        lv_ve_encode_out o{nullptr, 0, reinterpret_cast<uint64_t *>(off.p()), reinterpret_cast<uint64_t *>(len.p()),
                           reinterpret_cast<lv_ve_encode_totals *>(tot.p())};
        CHECK(lv_version_edit_encode_host(nullptr, xs.n, &in, records, &o) == 0);
        CHECK(off.guards_whole() && len.guards_whole() && tot.guards_whole());
        CHECK(same(tot.p(), &want, sizeof want));
        if (want.status)
            CHECK(off.untouched() && len.untouched());
        else
            CHECK(same(off.p(), ro.data(), off.bytes) && same(len.p(), rl.data(), len.bytes));
    }
    // exactly out_bytes, then one byte less
    for (size_t less = 0; less < 2; ++less) {
        if (less && (want.status || !want.out_bytes)) break;
        const size_t cap = want.status ? 16 : want.out_bytes - less;
        Guarded dst(cap), off(records * 8), len(records * 8), tot(sizeof(lv_ve_encode_totals));
        lv_ve_encode_out o{dst.p(), cap, reinterpret_cast<uint64_t *>(off.p()), reinterpret_cast<uint64_t *>(len.p()),
                           reinterpret_cast<lv_ve_encode_totals *>(tot.p())};
        CHECK(lv_version_edit_encode_host(xs.p, xs.n, &in, records, &o) == 0);
        CHECK(dst.guards_whole() && off.guards_whole() && len.guards_whole() && tot.guards_whole());
        lv_ve_encode_totals got;
        std::memcpy(&got, tot.p(), sizeof got);
        if (less) {
            lv_ve_encode_totals over = want;
            over.status = LV_VE_ENCODE_OUT_OVER;
            CHECK(same(&got, &over, sizeof got));
            CHECK(dst.untouched() && off.untouched() && len.untouched());
        } else {
            CHECK(same(&got, &want, sizeof got));
            if (want.status) {
                CHECK(dst.untouched() && off.untouched() && len.untouched());
            } else {
                CHECK(out.size() == want.out_bytes && same(dst.p(), out.data(), out.size()));
                CHECK(same(off.p(), ro.data(), off.bytes) && same(len.p(), rl.data(), len.bytes));
            }
        }
    }
    return want.status != 0;
}

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
    std::vector<uint8_t> data;
    uint8_t chunk[65536];
    for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) data.insert(data.end(), chunk, chunk + n);
    std::fclose(f);
    if (data.size() < 16 || std::memcmp(data.data(), "VEDUMP01", 8) != 0) {
        std::fprintf(stderr, "not a version_edit dump\n");
        return 2;
    }
    Reader R{data, 8};
    const uint64_t cases = R.u64();
    uint64_t decodes = 0, encodes = 0, refused = 0;
    for (uint64_t i = 0; i < cases && R.ok; ++i) {
        const std::vector<uint8_t> name = R.blob();
        g_case.assign(name.begin(), name.end());
        const uint64_t kind = R.u64();
        if (kind == 0) {
            decode_case(R);
            ++decodes;
        } else if (kind == 1) {
            refused += encode_case(R);
            ++encodes;
        } else {
            R.ok = false;
        }
    }
    if (!R.ok || R.at != data.size()) {
        std::fprintf(stderr, "the dump is cut short or malformed (case %s)\n", g_case.c_str());
        return 2;
    }
    std::printf("version_edit_hostcheck: %llu cases replayed, %llu decodes, %llu encodes (%llu refused), %d failures\n",
                static_cast<unsigned long long>(cases), static_cast<unsigned long long>(decodes),
                static_cast<unsigned long long>(encodes), static_cast<unsigned long long>(refused), g_fail);
    return g_fail ? 1 : 0;
}
