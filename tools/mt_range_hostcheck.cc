// Stand-alone check of the range read's host twin (lv_memtable_range_host,
// csrc/memtable.cc) for sanitizer builds on the CPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tools/mt_range_hostcheck.cc leveldb-rs_amd/csrc/memtable.cc
//       -o mt_range_hostcheck && ./mt_range_hostcheck cases.bin
//
// tests/test_mt_range_hostcheck.py builds it this way and runs it over the
// dump tests/mt_range_cases.py writes (its dump() documents the layout): the
// cases the CPU and GPU tests use, each with the model's answer for every
// query, and damaged quadruples (order indices out of range, key extents
// outside the payload, an unsorted and a reversed order, entries > op_cap and
// entries beyond the order's length under a status) that carry no answer.
//
// Every input is a heap block of exactly its size, so a read one byte outside
// is a heap-buffer-overflow.  The hit slot and the result lie between two
// guards of canary bytes and are filled with the canary first.  After every
// call: the guards are whole, every result field was written (reserved is 0),
// the status is one of the six, count <= limit, and the slot beyond count is
// untouched unless the walk met a damaged entry (NO_TABLE over a table whose
// totals are fine); with a status above MORE_SCAN every other field is 0.
// Where the dump has an answer, the result and the hits equal it.  For the
// damaged quadruples termination is checked too: next_pos - seek_pos never
// exceeds max_scan, and a chain of resumes from each result ends within
// entries / min(limit, max_scan) + 2 calls.  Exits 0 when everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lvgpu/crc32c.h"
#include "lvgpu/memtable.h"

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
constexpr uint32_t kCanary32 = 0xA5A5A5A5u;
constexpr size_t kGuard = 64;

// `bytes` output bytes between two guards, all canary; p() is the output.
struct Guarded {
    uint8_t *block;
    size_t bytes;
    explicit Guarded(size_t n) : block(static_cast<uint8_t *>(std::malloc(n + 2 * kGuard))), bytes(n) { fill(); }
    ~Guarded() { std::free(block); }
    Guarded(const Guarded &) = delete;
    void fill() { std::memset(block, kCanary, bytes + 2 * kGuard); }
    uint8_t *p() const { return block + kGuard; }
    bool guards_whole() const {
        for (size_t i = 0; i < kGuard; ++i)
            if (block[i] != kCanary || block[kGuard + bytes + i] != kCanary) return false;
        return true;
    }
};

// An input of exactly n bytes on the heap (a one-byte block for n = 0, never read).
struct Exact {
    uint8_t *p;
    size_t n;
    Exact(const uint8_t *src, size_t bytes) : p(static_cast<uint8_t *>(std::malloc(bytes ? bytes : 1))), n(bytes) {
        if (bytes) std::memcpy(p, src, bytes);
    }
    ~Exact() { std::free(p); }
    Exact(const Exact &) = delete;
    const uint8_t *get() const { return n ? p : nullptr; }
};

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
    template <class T>
    T num() {
        T v{};
        if (const uint8_t *p = take(sizeof(T))) std::memcpy(&v, p, sizeof(T));
        return v;
    }
};

struct Table {
    const uint8_t *payload;
    size_t payload_bytes;
    const lv_wb_op *ops;
    const uint32_t *order;
    lv_mt_totals totals;
    size_t op_cap;
    const uint8_t *qkeys;
    size_t qkeys_bytes;
};

// One call with guarded outputs; the generic checks.  Returns the result.
lv_mt_range_result call(const Table &T, const lv_mt_range_query &q, uint32_t limit, uint64_t max_scan, bool damaged,
                        std::vector<uint32_t> *hits_out) {
    Guarded slot(static_cast<size_t>(limit) * 4), res(sizeof(lv_mt_range_result));
    Exact query(reinterpret_cast<const uint8_t *>(&q), sizeof q);
    uint32_t *hits = reinterpret_cast<uint32_t *>(slot.p());
    lv_mt_range_result *out = reinterpret_cast<lv_mt_range_result *>(res.p());
    const int rc = lv_memtable_range_host(T.payload, T.payload_bytes, T.ops, T.order, &T.totals, T.op_cap, T.qkeys,
                                          T.qkeys_bytes, reinterpret_cast<const lv_mt_range_query *>(query.p), limit,
                                          max_scan, hits, out);
    CHECK(rc == 0);
    CHECK(slot.guards_whole() && res.guards_whole());
    lv_mt_range_result r;
    std::memcpy(&r, out, sizeof r);
    CHECK(r.reserved == 0 && r.seen <= 1);
    CHECK(r.status <= LV_MT_GET_BAD_QUERY);
    CHECK(r.count <= limit);
    if (r.status > LV_MT_RANGE_MORE_SCAN)
        CHECK(r.count == 0 && r.seek_pos == 0 && r.next_pos == 0 && r.unparsed == 0 && r.seen == 0);
    const bool met_damage = damaged && r.status == LV_MT_GET_NO_TABLE && !T.totals.status && T.totals.entries <= T.op_cap;
    if (!met_damage)
        for (uint32_t i = r.count <= limit ? r.count : limit; i < limit; ++i) CHECK(hits[i] == kCanary32);
    if (r.status <= LV_MT_RANGE_MORE_SCAN) {
        CHECK(r.next_pos >= r.seek_pos && r.next_pos - r.seek_pos <= max_scan && r.next_pos <= T.totals.entries);
        CHECK(r.unparsed <= r.next_pos - r.seek_pos && r.count <= r.next_pos - r.seek_pos);
        for (uint32_t i = 0; i < r.count && i < limit; ++i) CHECK(hits[i] < T.op_cap);
    }
    if (hits_out) hits_out->assign(hits, hits + (r.count <= limit ? r.count : 0));
    return r;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> file;
    if (FILE *f = std::fopen(argv[1], "rb")) {
        uint8_t buf[65536];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + n);
        std::fclose(f);
    }
    Reader R{file};
    const uint8_t *magic = R.take(4);
    if (!magic || std::memcmp(magic, "MTRG", 4) != 0) {
        std::fprintf(stderr, "not a dump of tests/mt_range_cases.py\n");
        return 2;
    }
    const uint32_t ncases = R.num<uint32_t>();
    uint64_t queries = 0, compared = 0, damaged_calls = 0, no_table = 0, chains = 0;
    uint32_t done = 0;
    for (; done < ncases && R.ok; ++done) {
        const uint32_t nl = R.num<uint32_t>();
        const uint8_t *nm = R.take(nl);
        g_case = nm ? std::string(reinterpret_cast<const char *>(nm), nl) : "?";
        const uint64_t pbytes = R.num<uint64_t>();
        const uint8_t *pp = R.take(pbytes);
        const uint64_t nops = R.num<uint64_t>();
        const uint8_t *op = R.take(nops * sizeof(lv_wb_op));
        const uint64_t nord = R.num<uint64_t>();
        const uint8_t *od = R.take(nord * 4);
        lv_mt_totals tot;
        tot.entries = R.num<uint64_t>();
        tot.user_keys = R.num<uint64_t>();
        tot.status = R.num<uint64_t>();
        const uint64_t cap = R.num<uint64_t>();
        const uint64_t kbytes = R.num<uint64_t>();
        const uint8_t *kp = R.take(kbytes);
        const uint32_t nq = R.num<uint32_t>();
        const uint32_t limit = R.num<uint32_t>();
        const uint64_t max_scan = R.num<uint64_t>();
        const uint32_t has_want = R.num<uint32_t>();
        const uint8_t *qp = R.take(static_cast<size_t>(nq) * sizeof(lv_mt_range_query));
        if (!R.ok) break;
        // (the twin reads order[i] only for i < entries <= op_cap: a dump whose order is shorter says so in its totals)
        Exact payload(pp, pbytes), ops(op, nops * sizeof(lv_wb_op)), order(od, nord * 4), qkeys(kp, kbytes);
        Table T{payload.get(), static_cast<size_t>(pbytes), reinterpret_cast<const lv_wb_op *>(ops.get()),
                reinterpret_cast<const uint32_t *>(order.get()), tot, static_cast<size_t>(cap), qkeys.get(),
                static_cast<size_t>(kbytes)};
        CHECK(cap <= nops && (tot.entries <= nord || tot.entries > cap || tot.status));
        for (uint32_t i = 0; i < nq && R.ok; ++i) {
            lv_mt_range_query q;
            std::memcpy(&q, qp + static_cast<size_t>(i) * sizeof q, sizeof q);
            std::vector<uint32_t> hits;
            const lv_mt_range_result r = call(T, q, limit, max_scan, !has_want, &hits);
            ++queries;
            no_table += r.status == LV_MT_GET_NO_TABLE;
            if (has_want) {
                lv_mt_range_result w;
                if (const uint8_t *wp = R.take(sizeof w)) std::memcpy(&w, wp, sizeof w);
                if (!R.ok) break;
                const uint8_t *wh = R.take(static_cast<size_t>(w.count) * 4);
                if (!R.ok) break;
                CHECK(std::memcmp(&r, &w, sizeof r) == 0);
                CHECK(hits.size() == w.count && (w.count == 0 || std::memcmp(hits.data(), wh, hits.size() * 4) == 0));
                ++compared;
                continue;
            }
            // a damaged quadruple: the chain of resumes from this result ends
            ++damaged_calls;
            const uint64_t step = limit < max_scan ? limit : max_scan;
            const uint64_t most = tot.entries / step + 2;
            lv_mt_range_result c = r;
            uint64_t calls = 1;
            while ((c.status == LV_MT_RANGE_MORE_LIMIT || c.status == LV_MT_RANGE_MORE_SCAN) && calls <= most) {
                lv_mt_range_query n{};
                n.hi_off = q.hi_off;
                n.hi_len = q.hi_len;
                n.seq = q.seq;
                n.pos = c.next_pos;
                n.flags = (q.flags & LV_MT_RANGE_HAS_HI) | LV_MT_RANGE_RESUME | (c.seen ? LV_MT_RANGE_SEEN : 0u);
                const uint64_t before = c.next_pos;
                c = call(T, n, limit, max_scan, true, nullptr);
                ++calls;
                if (c.status <= LV_MT_RANGE_MORE_SCAN) CHECK(c.seek_pos == before);
                if (c.status == LV_MT_RANGE_MORE_LIMIT || c.status == LV_MT_RANGE_MORE_SCAN) CHECK(c.next_pos > before);
            }
            CHECK(calls <= most);
            ++chains;
        }
    }
    if (!R.ok || done != ncases || R.at != file.size()) {
        std::fprintf(stderr, "the dump is cut short or has a tail (case %u of %u)\n", done, ncases);
        return 2;
    }
    std::printf("mt_range_hostcheck: %u cases replayed, %llu queries, %llu compared with the model, %llu over damaged "
                "quadruples (%llu chains), %llu NO_TABLE, %d failures\n",
                ncases, static_cast<unsigned long long>(queries), static_cast<unsigned long long>(compared),
                static_cast<unsigned long long>(damaged_calls), static_cast<unsigned long long>(chains),
                static_cast<unsigned long long>(no_table), g_fail);
    return g_fail ? 1 : 0;
}
