// lv_write_batch_iterate: WriteBatch::iterate with a MemTableInserter as its
// Handler (write_batch.rs:92-122, :178-188), one rep at a time on the host.
// The scalar twin of the device walk in write_batch.hip; host only, no GPU.
// lv_write_batch_encode_host: the inverse, WriteBatch::put / delete /
// set_sequence (write_batch.rs:57-78) over an op table, record after record;
// the scalar twin of write_batch_encode.hip.
#include "../../include/lvgpu/write_batch.h"

#include <cstring>

#include "../../include/lvgpu/crc32c.h"

namespace {

// coding.rs:186-204 (decode_varint_32_limit over the remaining input) and
// :294-305 (decode_length_prefixed_slice): LV_WB_OK and (*len, *pos past the
// length), or the error.
uint32_t varstring(const uint8_t *rep, size_t n, size_t *pos, uint32_t *len) {
    uint32_t result = 0;
    size_t p = *pos;
    bool done = false;
    for (uint32_t shift = 0; shift <= 28 && p < n; shift += 7) {
        const uint8_t byte = rep[p++];
        result |= static_cast<uint32_t>(byte & 0x7f) << shift;  // bits above 31 of the fifth byte fall off
        if (!(byte & 0x80)) {
            done = true;
            break;
        }
    }
    if (!done) return LV_WB_BAD_VARINT;
    if (n - p < result) return LV_WB_BAD_LENGTH;
    *pos = p;
    *len = result;
    return LV_WB_OK;
}

}  // namespace

extern "C" uint32_t lv_write_batch_iterate(const uint8_t *rep, size_t n, lv_wb_op *ops, size_t op_cap, size_t *found,
                                           uint64_t *sequence, uint32_t *count) {
    if (found) *found = 0;
    if (sequence) *sequence = 0;
    if (count) *count = 0;
    if (n < LV_WB_HEADER_SIZE) return LV_WB_TOO_SMALL;  // write_batch.rs:94-96
    uint64_t seq = 0;
    uint32_t cnt = 0;
    for (int i = 0; i < 8; ++i) seq |= static_cast<uint64_t>(rep[i]) << (8 * i);
    for (int i = 0; i < 4; ++i) cnt |= static_cast<uint32_t>(rep[8 + i]) << (8 * i);
    if (sequence) *sequence = seq;
    if (count) *count = cnt;
    size_t pos = LV_WB_HEADER_SIZE, emitted = 0;
    uint32_t status = LV_WB_OK;
    while (pos < n) {
        const uint32_t tag = rep[pos++];
        if (tag > LV_WB_TYPE_VALUE) {
            status = LV_WB_BAD_TAG;
            break;
        }
        uint32_t klen = 0, vlen = 0;
        if ((status = varstring(rep, n, &pos, &klen)) != LV_WB_OK) break;
        const size_t koff = pos;
        pos += klen;
        size_t voff = pos;
        if (tag == LV_WB_TYPE_VALUE) {
            if ((status = varstring(rep, n, &pos, &vlen)) != LV_WB_OK) break;
            voff = pos;
            pos += vlen;
        }
        if (emitted < op_cap && ops) {
            lv_wb_op &o = ops[emitted];
            o.tag = ((seq + emitted) << 8) | tag;
            o.key_off = koff;
            o.val_off = voff;
            o.key_len = klen;
            o.val_len = vlen;
        }
        ++emitted;
    }
    if (found) *found = emitted;
    if (status == LV_WB_OK && emitted != cnt) status = LV_WB_WRONG_COUNT;  // write_batch.rs:117-119
    return status;
}

namespace {

constexpr uint64_t kEncMaxRecords = 0xfffffffeull;
constexpr uint64_t kEncMaxOps = 1ull << 30;

// [off, off + len) lies inside [0, bytes).  All u64: nothing wraps.
bool extent_ok(uint64_t off, uint64_t len, uint64_t bytes) { return off <= bytes && len <= bytes - off; }

uint32_t varint_len(uint32_t v) {
    uint32_t n = 1;
    for (; v >= 128; v >>= 7) ++n;
    return n;
}

// coding.rs' encode_varint_32 at out + at (out may be null: sizing); returns the bytes.
uint32_t put_varint(uint8_t *out, uint64_t at, uint32_t v) {
    uint32_t n = 0;
    for (; v >= 128; v >>= 7, ++n)
        if (out) out[at + n] = static_cast<uint8_t>(v | 0x80);
    if (out) out[at + n] = static_cast<uint8_t>(v);
    return n + 1;
}

}  // namespace

extern "C" int lv_write_batch_encode_host(const uint8_t *src, size_t src_bytes, const lv_wb_op *ops, size_t op_cap,
                                          const uint64_t *rec_op, size_t records, uint64_t first_sequence, uint8_t *out,
                                          size_t out_cap, uint64_t *rec_off, uint64_t *rec_len, lv_wb_op *ops_out,
                                          lv_wb_encode_totals *totals) {
    const bool sizing = !out && !out_cap;  // src is then never read and may be null
    if (!totals || !rec_op || (!src && src_bytes && !sizing) || (!ops && op_cap) || (!out && out_cap) ||
        (records && (!rec_off || !rec_len)) || records > kEncMaxRecords || op_cap > kEncMaxOps)
        return LV_ERR_INVALID;
    lv_wb_encode_totals t{};
    t.records = records;
    t.last_sequence = first_sequence - 1;
    t.bad_record = t.bad_op = ~0ull;
    // the bounds, before any op is read
    for (size_t r = 0; r < records; ++r)
        if (!(rec_op[r] <= rec_op[r + 1] && rec_op[r + 1] <= op_cap)) {
            t.status = LV_WB_ENCODE_BAD_BOUNDS;
            t.bad_record = r;
            *totals = t;
            return 0;
        }
    const uint64_t base = records ? rec_op[0] : 0, nops = records ? rec_op[records] - base : 0;
    // every op, before any byte of src is read
    uint64_t kb = 0, vb = 0, bytes = static_cast<uint64_t>(LV_WB_HEADER_SIZE) * records;
    for (size_t r = 0; r < records; ++r)
        for (uint64_t i = rec_op[r]; i < rec_op[r + 1]; ++i) {
            const lv_wb_op &o = ops[i];
            const uint32_t type = static_cast<uint32_t>(o.tag & 0xff);
            if (type > LV_WB_TYPE_VALUE || !extent_ok(o.key_off, o.key_len, src_bytes) ||
                (type == LV_WB_TYPE_VALUE && !extent_ok(o.val_off, o.val_len, src_bytes))) {
                t.status = LV_WB_ENCODE_BAD_OP;
                t.bad_record = r;
                t.bad_op = i;
                *totals = t;
                return 0;
            }
            kb += o.key_len;
            bytes += 1 + varint_len(o.key_len) + static_cast<uint64_t>(o.key_len);
            if (type == LV_WB_TYPE_VALUE) {
                vb += o.val_len;
                bytes += varint_len(o.val_len) + static_cast<uint64_t>(o.val_len);
            }
        }
    t.ops = nops;
    t.key_bytes = kb;
    t.value_bytes = vb;
    t.out_bytes = bytes;
    t.last_sequence = first_sequence - 1 + nops;
    if (!sizing && bytes > out_cap) {
        t.status = LV_WB_ENCODE_OUT_OVER;
        *totals = t;
        return 0;
    }
    uint64_t at = 0;
    for (size_t r = 0; r < records; ++r) {
        const uint64_t begin = at, seq = first_sequence + (rec_op[r] - base);
        const uint32_t count = static_cast<uint32_t>(rec_op[r + 1] - rec_op[r]);
        if (out) {
            for (int i = 0; i < 8; ++i) out[at + i] = static_cast<uint8_t>(seq >> (8 * i));
            for (int i = 0; i < 4; ++i) out[at + 8 + i] = static_cast<uint8_t>(count >> (8 * i));
        }
        at += LV_WB_HEADER_SIZE;
        for (uint64_t i = rec_op[r]; i < rec_op[r + 1]; ++i) {
            const lv_wb_op &o = ops[i];
            const uint32_t type = static_cast<uint32_t>(o.tag & 0xff);
            lv_wb_op w;
            w.tag = ((first_sequence + (i - base)) << 8) | type;
            if (out) out[at] = static_cast<uint8_t>(type);
            ++at;
            at += put_varint(out, at, o.key_len);
            w.key_off = at;
            w.key_len = o.key_len;
            if (out && o.key_len) std::memcpy(out + at, src + o.key_off, o.key_len);
            at += o.key_len;
            w.val_off = at;
            w.val_len = 0;
            if (type == LV_WB_TYPE_VALUE) {
                at += put_varint(out, at, o.val_len);
                w.val_off = at;
                w.val_len = o.val_len;
                if (out && o.val_len) std::memcpy(out + at, src + o.val_off, o.val_len);
                at += o.val_len;
            }
            if (ops_out) ops_out[i - base] = w;
        }
        rec_off[r] = begin;
        rec_len[r] = at - begin;
    }
    *totals = t;
    return 0;
}
