// Stand-alone check of lv_write_batch_iterate and lv_write_batch_encode_host
// (csrc/write_batch.cc) for sanitizer builds on the CPU:
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
//
// The encoder gets heap buffers of exactly the sizes needed for src, out and
// every array: the reference's cases, every status at its smallest input and a
// few thousand pseudo-random op tables, each in sizing mode, with the exact
// out_cap and with out_cap - 1; every encoded record goes back through
// lv_write_batch_iterate, and a call that raises a status must leave every
// array as it was.
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

// ---- lv_write_batch_encode_host ----
constexpr uint8_t kFill = 0xA5;

template <class T>
T *exact(const std::vector<T> &v) {  // a heap copy of exactly v's size (1 byte when empty)
    T *p = static_cast<T *>(std::malloc(v.empty() ? 1 : v.size() * sizeof(T)));
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
template <class T>
T *filled(size_t n) {
    T *p = static_cast<T *>(std::malloc(n ? n * sizeof(T) : 1));
    std::memset(p, kFill, n ? n * sizeof(T) : 1);
    return p;
}
bool still_filled(const void *p, size_t bytes) {
    for (size_t i = 0; i < bytes; ++i)
        if (static_cast<const uint8_t *>(p)[i] != kFill) return false;
    return true;
}

struct Table {
    std::vector<uint8_t> src;
    std::vector<lv_wb_op> ops;
    std::vector<uint64_t> rec_op;  // records + 1
    size_t op_cap = 0;
    size_t records() const { return rec_op.size() - 1; }
};

struct Encoded {
    lv_wb_encode_totals t;
    std::vector<uint8_t> out;
    std::vector<uint64_t> off, len;
    std::vector<lv_wb_op> ops;
    bool untouched;
};

// One call.  out_cap < 0: the sizing mode (out == NULL, out_cap == 0).
Encoded encode(const Table &tb, uint64_t first, long long out_cap, size_t nops) {
    uint8_t *src = exact(tb.src);
    lv_wb_op *ops = exact(tb.ops);
    uint64_t *rec_op = exact(tb.rec_op);
    const size_t n = tb.records(), cap = out_cap < 0 ? 0 : static_cast<size_t>(out_cap);
    uint8_t *out = out_cap < 0 ? nullptr : filled<uint8_t>(cap);
    uint64_t *off = filled<uint64_t>(n), *len = filled<uint64_t>(n);
    lv_wb_op *oo = filled<lv_wb_op>(nops);
    Encoded e{};
    const int rc = lv_write_batch_encode_host(tb.src.empty() ? nullptr : src, tb.src.size(), tb.op_cap ? ops : nullptr,
                                              tb.op_cap, rec_op, n, first, out, cap, off, len, oo, &e.t);
    CHECK(rc == 0);
    e.untouched = (!out || still_filled(out, cap)) && still_filled(off, n * 8) && still_filled(len, n * 8) &&
                  still_filled(oo, nops * sizeof(lv_wb_op));
    if (out) e.out.assign(out, out + cap);
    e.off.assign(off, off + n);
    e.len.assign(len, len + n);
    e.ops.assign(oo, oo + nops);
    std::free(src);
    std::free(ops);
    std::free(rec_op);
    std::free(out);
    std::free(off);
    std::free(len);
    std::free(oo);
    return e;
}

bool same_totals(const lv_wb_encode_totals &a, const lv_wb_encode_totals &b, bool but_status = false) {
    return a.records == b.records && a.ops == b.ops && a.key_bytes == b.key_bytes && a.value_bytes == b.value_bytes &&
           a.out_bytes == b.out_bytes && a.last_sequence == b.last_sequence && (but_status || a.status == b.status) &&
           a.bad_record == b.bad_record && a.bad_op == b.bad_op;
}

// Sizing, exact and one short; the records back through the iterate.  Returns the exact call.
Encoded run_encode(const Table &tb, uint64_t first, uint64_t want_status) {
    const size_t n = tb.records();
    bool bounds_ok = true;
    for (size_t r = 0; r < n; ++r) bounds_ok = bounds_ok && tb.rec_op[r] <= tb.rec_op[r + 1] && tb.rec_op[r + 1] <= tb.op_cap;
    const size_t nops = bounds_ok && n ? static_cast<size_t>(tb.rec_op[n] - tb.rec_op[0]) : 0;
    const Encoded size = encode(tb, first, -1, nops);
    CHECK(size.t.status == want_status);
    if (size.t.status) {
        CHECK(size.untouched && size.t.ops == 0 && size.t.out_bytes == 0 && size.t.last_sequence == first - 1);
        const Encoded again = encode(tb, first, 64, nops);
        CHECK(again.untouched && same_totals(again.t, size.t));
        return again;
    }
    CHECK(size.t.records == n && size.t.ops == nops && size.t.last_sequence == first - 1 + nops &&
          size.t.bad_record == ~0ull && size.t.bad_op == ~0ull);
    CHECK(size.t.out_bytes <= 12 * n + 11 * nops + size.t.key_bytes + size.t.value_bytes);
    const Encoded full = encode(tb, first, static_cast<long long>(size.t.out_bytes), nops);
    CHECK(same_totals(full.t, size.t) && full.off == size.off && full.len == size.len);
    for (size_t j = 0; j < nops; ++j) CHECK(same_op(full.ops[j], size.ops[j]));
    if (size.t.out_bytes) {
        const Encoded shy = encode(tb, first, static_cast<long long>(size.t.out_bytes) - 1, nops);
        CHECK(shy.t.status == LV_WB_ENCODE_OUT_OVER && same_totals(shy.t, size.t, true) && shy.untouched);
    }
    uint64_t at = 0;
    const uint64_t base = n ? tb.rec_op[0] : 0;
    for (size_t r = 0; r < n; ++r) {
        CHECK(full.off[r] == at);
        const std::vector<uint8_t> rep(full.out.begin() + at, full.out.begin() + at + full.len[r]);
        const Result it = call(rep, rep.size(), rep.size() / 2 + 1, false);
        const uint64_t a = tb.rec_op[r] - base, b = tb.rec_op[r + 1] - base;
        CHECK(it.status == LV_WB_OK && it.seq == first + a && it.count == b - a && it.found == b - a);
        for (size_t k = 0; k < it.ops.size() && a + k < nops; ++k) {
            lv_wb_op o = it.ops[k];
            o.key_off += at;
            o.val_off += at;
            CHECK(same_op(o, full.ops[a + k]));
            const lv_wb_op &in = tb.ops[tb.rec_op[r] + k];
            CHECK((o.tag & 0xff) == (in.tag & 0xff) && o.key_len == in.key_len);
            if (in.key_len) CHECK(std::memcmp(full.out.data() + o.key_off, tb.src.data() + in.key_off, in.key_len) == 0);
            if ((in.tag & 0xff) == LV_WB_TYPE_VALUE) {
                CHECK(o.val_len == in.val_len);
                if (in.val_len) CHECK(std::memcmp(full.out.data() + o.val_off, tb.src.data() + in.val_off, in.val_len) == 0);
            }
        }
        at += full.len[r];
    }
    CHECK(at == full.t.out_bytes);
    return full;
}

// A table of one record per inner vector of Puts (key, value) and Deletes (key).
struct Spec {
    std::string key, value;
    bool del;
};
Table table_of(const std::vector<std::vector<Spec>> &recs) {
    Table tb;
    tb.rec_op.push_back(0);
    for (const auto &rec : recs) {
        for (const Spec &s : rec) {
            lv_wb_op o{};
            o.tag = (0xabcdefull << 8) | (s.del ? LV_WB_TYPE_DELETION : LV_WB_TYPE_VALUE);  // the upper bits are ignored
            o.key_off = tb.src.size();
            o.key_len = static_cast<uint32_t>(s.key.size());
            tb.src.insert(tb.src.end(), s.key.begin(), s.key.end());
            o.val_off = s.del ? ~0ull - 7 : tb.src.size();  // a DELETION's value fields are not read
            o.val_len = s.del ? 0xffffffffu : static_cast<uint32_t>(s.value.size());
            if (!s.del) tb.src.insert(tb.src.end(), s.value.begin(), s.value.end());
            tb.ops.push_back(o);
        }
        tb.rec_op.push_back(tb.ops.size());
    }
    tb.op_cap = tb.ops.size();
    return tb;
}

void encode_reference_cases() {
    {  // multiple: [Put foo bar, Delete box, Put baz boo] at 100
        Batch b;
        b.put("foo", "bar");
        b.del("box");
        b.put("baz", "boo");
        b.set_sequence(100);
        const Encoded e = run_encode(table_of({{{"foo", "bar", false}, {"box", "", true}, {"baz", "boo", false}}}), 100, 0);
        CHECK(e.out == b.rep && e.t.last_sequence == 102);
    }
    {  // append: each stage's concatenated ops as one record at 200
        Batch b1, b2;
        b1.set_sequence(200);
        b2.set_sequence(300);
        b1.append(b2);
        CHECK(run_encode(table_of({{}}), 200, 0).out == b1.rep && b1.rep.size() == LV_WB_HEADER_SIZE);
        b2.put("a", "va");
        b1.append(b2);
        CHECK(run_encode(table_of({{{"a", "va", false}}}), 200, 0).out == b1.rep);
        b2.clear();
        b2.put("b", "vb");
        b1.append(b2);
        CHECK(run_encode(table_of({{{"a", "va", false}, {"b", "vb", false}}}), 200, 0).out == b1.rep);
        b2.del("foo");
        b1.append(b2);
        CHECK(run_encode(table_of({{{"a", "va", false}, {"b", "vb", false}, {"b", "vb", false}, {"foo", "", true}}}), 200, 0)
                  .out == b1.rep);
    }
    {  // no records; empty records around full ones; the sequence wraps
        Table none;
        none.rec_op.push_back(0);
        CHECK(run_encode(none, 1, 0).t.last_sequence == 0);
        const Encoded e = run_encode(table_of({{}, {{"k", "v", false}, {"", "", false}}, {}, {}, {{"d", "", true}}, {}}), ~0ull - 1, 0);
        CHECK(e.t.records == 6 && e.t.ops == 3 && e.t.last_sequence == 0 && e.t.out_bytes == 6 * 12 + 5 + 3 + 3);
    }
    {  // two- and three-byte varints
        const Encoded e = run_encode(table_of({{{std::string(128, 'k'), std::string(16384, 'v'), false},
                                                {std::string(127, 'k'), std::string(16383, 'v'), false}}}), 5, 0);
        CHECK(e.t.out_bytes == 12 + (1 + 2 + 128 + 3 + 16384) + (1 + 1 + 127 + 2 + 16383));
    }
}

void encode_status_cases() {
    const Table good = table_of({{{"0123", "456789", false}}, {{"0123", "", true}}});  // src: 14 bytes
    {
        Table t = good;
        t.ops[1].tag = 2;
        const Encoded e = run_encode(t, 9, LV_WB_ENCODE_BAD_OP);
        CHECK(e.t.bad_op == 1 && e.t.bad_record == 1 && e.t.records == 2);
    }
    {
        Table t = good;
        t.ops[0].key_off = 11;  // [11, 15): one byte over
        CHECK(run_encode(t, 9, LV_WB_ENCODE_BAD_OP).t.bad_op == 0);
        t.ops[0].key_off = 10;  // [10, 14): exact
        run_encode(t, 9, 0);
    }
    {
        Table t = good;
        t.ops[0].val_len = 11;  // [4, 15)
        CHECK(run_encode(t, 9, LV_WB_ENCODE_BAD_OP).t.bad_record == 0);
    }
    {
        Table t = good;
        t.ops[1].key_off = ~0ull;  // 2^64 - 1 with length 2: the sum wraps
        t.ops[1].key_len = 2;
        CHECK(run_encode(t, 9, LV_WB_ENCODE_BAD_OP).t.bad_op == 1);
        t = good;
        t.ops[0].val_off = ~0ull;
        t.ops[0].val_len = 2;
        CHECK(run_encode(t, 9, LV_WB_ENCODE_BAD_OP).t.bad_op == 0);
    }
    {
        Table t = good;
        t.rec_op = {0, 2, 1};  // the bounds fall
        const Encoded e = run_encode(t, 9, LV_WB_ENCODE_BAD_BOUNDS);
        CHECK(e.t.bad_record == 1 && e.t.bad_op == ~0ull);
        t.rec_op = {0, 1, 3};  // the last bound is op_cap + 1
        CHECK(run_encode(t, 9, LV_WB_ENCODE_BAD_BOUNDS).t.bad_record == 1);
        t.rec_op = {3, 3, 3};
        CHECK(run_encode(t, 9, LV_WB_ENCODE_BAD_BOUNDS).t.bad_record == 0);
        t.rec_op = {0, 2, 1};  // the bounds are judged first: no op is read
        t.ops[0].tag = 7;
        CHECK(run_encode(t, 9, LV_WB_ENCODE_BAD_BOUNDS).t.bad_record == 1);
    }
}

void encode_random_tables() {
    size_t seen[3] = {};
    for (int i = 0; i < 4000; ++i) {
        Table tb;
        tb.src.resize(next_random() % 70);
        for (auto &b : tb.src) b = static_cast<uint8_t>(next_random());
        const size_t lead = next_random() % 3, n = next_random() % 7;
        tb.rec_op.push_back(lead);
        size_t total = lead;
        for (size_t r = 0; r < n; ++r) {
            total += (next_random() % 3 == 0) ? 0 : next_random() % 6;
            tb.rec_op.push_back(total);
        }
        const bool wild = i % 4 == 3;  // one op or bound in four tables goes wrong
        for (size_t k = 0; k < total; ++k) {
            lv_wb_op o{};
            const uint64_t S = tb.src.size();
            o.tag = (next_random() << 8) | (next_random() % 3 ? LV_WB_TYPE_VALUE : LV_WB_TYPE_DELETION);
            o.key_off = next_random() % (S + 1);
            o.key_len = static_cast<uint32_t>(next_random() % (S - o.key_off + 1));
            o.val_off = next_random() % (S + 1);
            o.val_len = static_cast<uint32_t>(next_random() % (S - o.val_off + 1));
            if ((o.tag & 0xff) == LV_WB_TYPE_DELETION) o.val_off = next_random(), o.val_len = static_cast<uint32_t>(next_random());
            if (k < lead) o.tag = 9, o.key_off = ~0ull;  // in front of the first record: never read
            tb.ops.push_back(o);
        }
        tb.op_cap = total;
        uint64_t want = 0;
        if (wild && total > lead && next_random() % 2) {
            lv_wb_op &o = tb.ops[lead + next_random() % (total - lead)];
            switch (next_random() % 3) {
                case 0: o.tag = (o.tag & ~0xffull) | (2 + next_random() % 250); break;
                case 1: o.key_len = static_cast<uint32_t>(tb.src.size() - o.key_off + 1 + next_random() % 5); break;
                default: o.tag |= 1, o.val_off = tb.src.size() + 1 + next_random() % 3; break;
            }
            want = LV_WB_ENCODE_BAD_OP;
        } else if (wild && n) {
            const size_t r = 1 + next_random() % n;
            if (next_random() % 2 || tb.rec_op[r] == 0) {
                tb.rec_op[n] = total + 1 + next_random() % 3;
            } else {
                tb.rec_op[r - 1] = tb.rec_op[r] + 1;
            }
            want = LV_WB_ENCODE_BAD_BOUNDS;
        }
        ++seen[want == 0 ? 0 : want == LV_WB_ENCODE_BAD_OP ? 1 : 2];
        run_encode(tb, next_random(), want);
    }
    CHECK(seen[0] > 2000 && seen[1] > 100 && seen[2] > 100);
}

}  // namespace

int main() {
    reference_cases();
    encode_reference_cases();
    encode_status_cases();
    encode_random_tables();
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
