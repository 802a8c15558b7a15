// lv_write_batch_iterate: WriteBatch::iterate with a MemTableInserter as its
// Handler (write_batch.rs:92-122, :178-188), one rep at a time on the host.
// The scalar twin of the device walk in write_batch.hip; host only, no GPU.
#include "../../include/lvgpu/write_batch.h"

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
