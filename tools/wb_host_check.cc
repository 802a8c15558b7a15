// Stand-alone check of lv_write_batch_iterate (csrc/write_batch.cc) for
// sanitizer builds on the CPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tools/wb_host_check.cc leveldb-rs_amd/csrc/write_batch.cc -o wb_host_check && ./wb_host_check
//
// tests/test_host_checks.py builds it this way and runs it with the CPU suite.
//
// Every input is copied into a heap buffer of exactly its size, so a read one
// byte past a rep is a heap-buffer-overflow.  Inputs: the reference's four
// test cases (write_batch.rs:240-297), every truncation of a multi-op batch,
// and a few thousand pseudo-random byte strings; each with an ample op_cap,
// with op_cap 0 (ops == NULL) and with op_cap = found - 1.  Exits 0 when every
// run agrees with itself and the reference cases give what the reference
// expects.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lvgpu/write_batch.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                        \
        }                                                                    \
    } while (0)

struct Batch {  // write_batch.rs:57-90, :131-161
    std::vector<uint8_t> rep = std::vector<uint8_t>(LV_WB_HEADER_SIZE, 0);
    uint32_t count() const { return rep[8] | rep[9] << 8 | rep[10] << 16 | static_cast<uint32_t>(rep[11]) << 24; }
    void set_count(uint32_t n) {
        for (int i = 0; i < 4; ++i) rep[8 + i] = static_cast<uint8_t>(n >> (8 * i));
    }
    void set_sequence(uint64_t s) {
        for (int i = 0; i < 8; ++i) rep[i] = static_cast<uint8_t>(s >> (8 * i));
    }
    void varstring(const std::string &s) {
        uint32_t v = static_cast<uint32_t>(s.size());
        while (v >= 128) {
            rep.push_back(static_cast<uint8_t>(v | 0x80));
            v >>= 7;
        }
        rep.push_back(static_cast<uint8_t>(v));
        rep.insert(rep.end(), s.begin(), s.end());
    }
    void put(const std::string &k, const std::string &v) {
        set_count(count() + 1);
        rep.push_back(LV_WB_TYPE_VALUE);
        varstring(k);
        varstring(v);
    }
    void del(const std::string &k) {
        set_count(count() + 1);
        rep.push_back(LV_WB_TYPE_DELETION);
        varstring(k);
    }
    void clear() { rep.assign(LV_WB_HEADER_SIZE, 0); }
    void append(const Batch &src) {
        set_count(count() + src.count());
        rep.insert(rep.end(), src.rep.begin() + LV_WB_HEADER_SIZE, src.rep.end());
    }
};

struct Result {
    uint32_t status;
    size_t found;
    uint64_t seq;
    uint32_t count;
    std::vector<lv_wb_op> ops;
};

// One call over an exact-size heap copy of the input.
Result call(const std::vector<uint8_t> &in, size_t n, size_t op_cap, bool null_ops) {
    uint8_t *buf = static_cast<uint8_t *>(std::malloc(n ? n : 1));
    if (n) std::memcpy(buf, in.data(), n);
    lv_wb_op *ops = null_ops ? nullptr : static_cast<lv_wb_op *>(std::malloc(op_cap ? op_cap * sizeof(lv_wb_op) : 1));
    Result r{};
    r.status = lv_write_batch_iterate(buf, n, ops, op_cap, &r.found, &r.seq, &r.count);
    if (ops) r.ops.assign(ops, ops + (r.found < op_cap ? r.found : op_cap));
    std::free(ops);
    std::free(buf);
    return r;
}

bool same_op(const lv_wb_op &a, const lv_wb_op &b) {
    return a.tag == b.tag && a.key_off == b.key_off && a.val_off == b.val_off && a.key_len == b.key_len &&
           a.val_len == b.val_len;
}

// Ample op_cap, op_cap 0 and op_cap = found - 1 agree; every op lies inside the input.
Result run(const std::vector<uint8_t> &in, size_t n) {
    const Result full = call(in, n, n / 2 + 1, false);
    CHECK(full.found <= n / 2 && full.ops.size() == full.found);
    const Result none = call(in, n, 0, true);
    CHECK(none.status == full.status && none.found == full.found && none.seq == full.seq && none.count == full.count);
    if (full.found) {
        const Result shy = call(in, n, full.found - 1, false);
        CHECK(shy.status == full.status && shy.found == full.found && shy.ops.size() == full.found - 1);
        for (size_t i = 0; i < shy.ops.size(); ++i) CHECK(same_op(shy.ops[i], full.ops[i]));
    }
    for (size_t i = 0; i < full.ops.size(); ++i) {
        const lv_wb_op &o = full.ops[i];
        CHECK(o.tag == (((full.seq + i) << 8) | (o.tag & 0xff)) && (o.tag & 0xff) <= 1);
        CHECK(o.key_off >= LV_WB_HEADER_SIZE + 2 && o.key_off + o.key_len <= n);
        CHECK(o.val_off >= o.key_off + o.key_len && o.val_off + o.val_len <= n);
        if ((o.tag & 0xff) == LV_WB_TYPE_DELETION) CHECK(o.val_off == o.key_off + o.key_len && o.val_len == 0);
    }
    if (n < LV_WB_HEADER_SIZE) CHECK(full.status == LV_WB_TOO_SMALL && full.found == 0);
    return full;
}

std::string key_of(const std::vector<uint8_t> &rep, const lv_wb_op &o) {
    return std::string(rep.begin() + o.key_off, rep.begin() + o.key_off + o.key_len);
}
std::string val_of(const std::vector<uint8_t> &rep, const lv_wb_op &o) {
    return std::string(rep.begin() + o.val_off, rep.begin() + o.val_off + o.val_len);
}

void reference_cases() {
    {  // empty
        Batch b;
        const Result r = run(b.rep, b.rep.size());
        CHECK(r.status == LV_WB_OK && r.found == 0 && r.count == 0);
    }
    {  // multiple
        Batch b;
        b.put("foo", "bar");
        b.del("box");
        b.put("baz", "boo");
        b.set_sequence(100);
        const Result r = run(b.rep, b.rep.size());
        CHECK(r.status == LV_WB_OK && r.found == 3 && r.seq == 100 && r.count == 3);
        if (r.ops.size() == 3) {
            CHECK(r.ops[0].tag == ((100ull << 8) | 1) && key_of(b.rep, r.ops[0]) == "foo" && val_of(b.rep, r.ops[0]) == "bar");
            CHECK(r.ops[1].tag == ((101ull << 8) | 0) && key_of(b.rep, r.ops[1]) == "box" && r.ops[1].val_len == 0);
            CHECK(r.ops[2].tag == ((102ull << 8) | 1) && key_of(b.rep, r.ops[2]) == "baz" && val_of(b.rep, r.ops[2]) == "boo");
        }
    }
    {  // corruption: Put(foo, bar)@200ParseError()
        Batch b;
        b.put("foo", "bar");
        b.del("box");
        b.set_sequence(200);
        const Result r = run(b.rep, b.rep.size() - 1);
        CHECK(r.status == LV_WB_BAD_LENGTH && r.found == 1);
        if (r.ops.size() == 1) CHECK(r.ops[0].tag == ((200ull << 8) | 1) && key_of(b.rep, r.ops[0]) == "foo");
    }
    {  // append
        Batch b1, b2;
        b1.set_sequence(200);
        b2.set_sequence(300);
        b1.append(b2);
        CHECK(run(b1.rep, b1.rep.size()).found == 0);
        b2.put("a", "va");
        b1.append(b2);
        CHECK(run(b1.rep, b1.rep.size()).found == 1);
        b2.clear();
        b2.put("b", "vb");
        b1.append(b2);
        CHECK(run(b1.rep, b1.rep.size()).found == 2);
        b2.del("foo");
        b1.append(b2);
        const Result r = run(b1.rep, b1.rep.size());
        CHECK(r.status == LV_WB_OK && r.found == 4 && r.seq == 200);
        if (r.ops.size() == 4) {
            CHECK(r.ops[3].tag == ((203ull << 8) | 0) && key_of(b1.rep, r.ops[3]) == "foo");
            CHECK(r.ops[2].tag == ((202ull << 8) | 1) && key_of(b1.rep, r.ops[2]) == "b");
        }
    }
}

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint64_t next_random() {  // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

}  // namespace

int main() {
    reference_cases();
    // every truncation of a multi-op batch (a long key and value among them: two-byte varints)
    Batch b;
    b.set_sequence((1ull << 56) - 2);  // the tags wrap inside the batch
    for (int i = 0; i < 24; ++i) {
        const std::string k(static_cast<size_t>(i % 5 == 4 ? 130 + i : i), static_cast<char>('a' + i));
        if (i % 3 == 0)
            b.del(k);
        else
            b.put(k, std::string(static_cast<size_t>(i % 7 == 6 ? 200 : i * 2), 'v'));
    }
    size_t statuses[7] = {};
    for (size_t n = 0; n <= b.rep.size(); ++n) ++statuses[run(b.rep, n).status];
    CHECK(statuses[LV_WB_OK] == 1 && statuses[LV_WB_TOO_SMALL] == 12 && statuses[LV_WB_BAD_VARINT] > 0 &&
          statuses[LV_WB_BAD_LENGTH] > 0 && statuses[LV_WB_WRONG_COUNT] > 0);
    // pseudo-random byte strings; every other one with small bytes after the header so that it parses further
    size_t seen[7] = {};
    for (int i = 0; i < 6000; ++i) {
        const size_t n = next_random() % 96;
        std::vector<uint8_t> in(n);
        for (size_t j = 0; j < n; ++j) {
            in[j] = static_cast<uint8_t>(next_random());
            if ((i & 1) && j >= LV_WB_HEADER_SIZE) in[j] &= (next_random() % 10 == 0) ? 0x83 : 0x07;
        }
        if ((i & 3) == 3 && n >= LV_WB_HEADER_SIZE) in[8] = static_cast<uint8_t>(next_random() % 8), in[9] = in[10] = in[11] = 0;
        ++seen[run(in, n).status];
    }
    for (uint32_t s = LV_WB_TOO_SMALL; s <= LV_WB_BAD_TAG; ++s) CHECK(seen[s] > 0);
    if (g_fail) {
        std::fprintf(stderr, "wb_host_check: %d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("wb_host_check ok\n");
    return 0;
}
