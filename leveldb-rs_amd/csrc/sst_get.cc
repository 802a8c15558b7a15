// The host twins of sst_get.hip (include/lvgpu/table.h, "Open" and "Get"):
// Table::Open and Table::InternalGet + SaveValue over an image in host memory,
// serial, by the core both halves compile (lvk/sst_read.h).  Host only, no
// GPU; the check of the device path that tools/sst_get_host_check.cc runs
// under a sanitizer and the one-core baseline of tools/bench_sst_get.py.
#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/table.h"
#include "lvk/sst_read.h"

extern "C" {

int lv_sst_open_host(const uint8_t *file, uint64_t file_bytes, uint64_t *handles, size_t block_cap,
                     lv_sst_table *table) {
    if (!table || (!file && file_bytes) || (!handles && block_cap)) return LV_ERR_INVALID;
    if (!file_bytes) {  // the empty table
        *table = lv_sst_table{};
        return 0;
    }
    lv_sst_table t;
    lvr::open_header(file, file_bytes, &t);
    uint64_t off = 0, size = 0;
    for (uint64_t i = 0; i < t.data_blocks; ++i) t.status |= lvr::open_restart(file, t, i, &off, &size);
    if (handles && t.data_blocks > block_cap) t.status |= LV_SST_OPEN_HANDLE_OVER;
    if (!t.status && handles) {
        const uint64_t n = t.data_blocks;
        for (uint64_t i = 0; i < n; ++i) lvr::open_restart(file, t, i, &handles[2 * i], &handles[2 * i + 1]);
        handles[2 * n] = t.metaindex_offset;
        handles[2 * n + 1] = t.metaindex_size;
        handles[2 * n + 2] = t.index_offset;
        handles[2 * n + 3] = t.index_size;
    }
    *table = t;
    return 0;
}

int lv_sst_get_host(const uint8_t *file, const lv_sst_table *table, const uint8_t *qkey, size_t qkey_len,
                    uint64_t seq, lv_sst_get_result *result) {
    if (!table || !result || (!file && table->file_bytes) || (!qkey && qkey_len) || qkey_len > 0xffffffffull)
        return LV_ERR_INVALID;
    lv_sst_get_result r{};
    if (table->status) {
        r.status = LV_SST_GET_NO_TABLE;
    } else if (seq > LV_MT_MAX_SEQUENCE) {
        r.status = LV_SST_GET_BAD_SEQ;
    } else {
        const lvr::Target t{qkey, static_cast<uint32_t>(qkey_len), (seq << 8) | LV_WB_TYPE_VALUE};
        r.status = lvr::get(file, table->file_bytes, table->index_offset, table->index_size, t, &r);
    }
    *result = r;
    return 0;
}

// ---- the filter block ("Bloom filter blocks") ----

uint32_t lv_bloom_hash(const uint8_t *key, size_t n) { return lvr::hash(key, n, lvr::kBloomSeed); }

int lv_bloom_key_may_match(const uint8_t *key, size_t key_len, const uint8_t *filter, size_t filter_len) {
    if (filter_len < 2) return 0;
    return lvr::bloom_may_match(filter, filter_len, lv_bloom_hash(key, key_len)) ? 1 : 0;
}

int lv_sst_bloom_open_host(const uint8_t *file, const lv_sst_table *table, lv_sst_bloom *bloom) {
    if (!table || !bloom || (!file && table->file_bytes)) return LV_ERR_INVALID;
    lv_sst_bloom b{};
    if (table->status)
        b.why = LV_SST_BLOOM_TABLE;
    else if (!table->file_bytes)
        b.why = LV_SST_BLOOM_EMPTY;
    else
        lvr::bloom_open(file, table->file_bytes, table->metaindex_offset, table->metaindex_size, &b);
    *bloom = b;
    return 0;
}

int lv_sst_get_bloom_host(const uint8_t *file, const lv_sst_table *table, const lv_sst_bloom *bloom,
                          const uint8_t *qkey, size_t qkey_len, uint64_t seq, lv_sst_get_result *result) {
    if (!table || !bloom || !result || (!file && table->file_bytes) || (!qkey && qkey_len) || qkey_len > 0xffffffffull)
        return LV_ERR_INVALID;
    lv_sst_get_result r{};
    if (table->status) {
        r.status = LV_SST_GET_NO_TABLE;
    } else if (seq > LV_MT_MAX_SEQUENCE) {
        r.status = LV_SST_GET_BAD_SEQ;
    } else {
        const lvr::Target t{qkey, static_cast<uint32_t>(qkey_len), (seq << 8) | LV_WB_TYPE_VALUE};
        r.status = lvr::get(file, table->file_bytes, table->index_offset, table->index_size, t, &r,
                            bloom->present == 1 ? bloom : nullptr);
    }
    *result = r;
    return 0;
}

}  // extern "C"
