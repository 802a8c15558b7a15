// The layout of Writer::add_record (log_writer.rs:62-110) for many records at
// once, host only: the fragment table, the zero trailers and the first
// fragment of every 32 KiB block of the appended span.  Shared by
// lv_wal_encode_host (wal_host.cc), lv_wal_encode_device (wal_encode.hip) and
// lv_wal_encode_size below.  No GPU, no HIP: builds and runs anywhere.
#include "../../include/lvgpu/wal.h"
#include "lv_internal.h"

namespace lvgpu_internal {

namespace {
constexpr uint64_t kBlock = LV_WAL_BLOCK_SIZE;
constexpr uint64_t kHeader = LV_WAL_HEADER_SIZE;
enum : uint8_t { kFull = 1, kFirst = 2, kMiddle = 3, kLast = 4 };  // log_format.rs:22-29
}  // namespace

void wal_layout(const uint64_t *rec_off, const uint64_t *rec_len, size_t n, uint64_t dest_length, bool table,
                WalLayout *out) {
    out->frags.clear();
    out->pads.clear();
    out->block_first.clear();
    uint64_t block_offset = dest_length % kBlock;  // log_writer.rs:48-56
    uint64_t pos = 0, count = 0;
    // Block k of the appended span holds the log bytes [k * kBlock - first, ...)
    // of it (first = dest_length % kBlock); block_first[k] is the first
    // fragment whose header lies in block k.  Every block but block 0 starts
    // with a header, so the entries ascend and block k's fragments are
    // [block_first[k], block_first[k + 1]).
    if (table && n) out->block_first.push_back(0);
    if (table) out->frags.reserve(n + n / 4 + 16);
    for (size_t r = 0; r < n; ++r) {
        uint64_t left = rec_len[r];
        uint64_t src = rec_off ? rec_off[r] : 0;
        bool begin = true;
        for (;;) {
            const uint64_t leftover = kBlock - block_offset;
            if (leftover < kHeader) {
                if (leftover > 0) {
                    if (table) out->pads.emplace_back(pos, leftover);
                    pos += leftover;
                }
                block_offset = 0;
            }
            if (block_offset == 0 && pos > 0 && table) out->block_first.push_back(count);
            const uint64_t avail = kBlock - block_offset - kHeader;
            const uint64_t frag_len = left < avail ? left : avail;
            const bool end = left == frag_len;
            const uint8_t type = begin && end ? kFull : begin ? kFirst : end ? kLast : kMiddle;
            if (table) out->frags.push_back({pos, src, static_cast<uint32_t>(frag_len), type});
            ++count;
            pos += kHeader + frag_len;
            block_offset += kHeader + frag_len;
            src += frag_len;
            left -= frag_len;
            begin = false;
            if (left == 0) break;
        }
    }
    if (table && n) out->block_first.push_back(count);  // the end of the last block's fragments
    out->out_len = pos;
    out->fragments = count;
}

}  // namespace lvgpu_internal

extern "C" size_t lv_wal_encode_size(const uint64_t *rec_len, size_t n, uint64_t dest_length, size_t *fragments) {
    lvgpu_internal::WalLayout lay;
    if (!rec_len) n = 0;
    lvgpu_internal::wal_layout(nullptr, rec_len, n, dest_length, false, &lay);
    if (fragments) *fragments = static_cast<size_t>(lay.fragments);
    return static_cast<size_t>(lay.out_len);
}
