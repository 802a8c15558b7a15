// The host twin of compact_output.hip (include/lvgpu/compact.h): the output of
// a compaction as a run of tables, as upstream's DoCompactionWork writes it.
// The serial loop with a real builder per file: a fresh TableBuilder (and
// FilterBlockBuilder) is fed entry after entry and closed after the add that
// brought its flushed bytes to max_file_bytes (sst_build.cc's walk); the
// records of a file are what the host opens and lv_version_file_host read back
// from its image.  Nothing of the device's scans is here, so that the two
// check each other.  Host only, no GPU.  Two passes, one walk per file each:
// the first sizes every file and decides the status, the second writes (the
// index block's place in a file is known only after the first).
#include <vector>

#include "../../include/lvgpu/compact.h"
#include "../../include/lvgpu/crc32c.h"
#include "sst_build_host.h"

namespace {

constexpr uint64_t kMaxOps = 0xfffffffeull;

bool extent_ok(uint64_t off, uint64_t len, uint64_t bytes) { return off <= bytes && len <= bytes - off; }

struct Cut {  // one output file, from the sizing pass
    uint64_t first, entries, file_bytes, data_blocks, index_offset;
};

}  // namespace

extern "C" {

uint64_t lv_compact_output_arena_bound(uint64_t payload_bytes, uint64_t op_cap, const lv_sst_build_options *opt,
                                       const lv_sst_bloom_options *bloom) {
    (void)opt;  // the bound holds for every block_size and restart_interval (compact.h)
    if (!op_cap || (bloom && (bloom->bits_per_key < 1 || bloom->bits_per_key > 64 || bloom->reserved))) return 0;
    const unsigned __int128 n = op_cap, p = payload_bytes;
    unsigned __int128 b = p * 2 + n * 75 + n * (70 + 15);
    if (bloom) b += n * bloom->bits_per_key / 8 + n * 9 + (p + n * 36) / 512 + n * 72;
    return b > ~0ull ? ~0ull : static_cast<uint64_t>(b);
}

int lv_compact_output_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops, const uint32_t *order,
                           const lv_mt_totals *mt_totals, size_t op_cap, const lv_sst_build_options *opt,
                           const lv_sst_bloom_options *bloom, uint64_t max_file_bytes, uint64_t first_number,
                           uint32_t level, uint64_t images_off, uint8_t *arena, uint64_t arena_cap, uint64_t *handles,
                           size_t block_cap, lv_compact_output_file *files, lv_sst_table *tables, lv_sst_bloom *blooms,
                           lv_version_file *version_files, size_t files_cap, uint8_t *bound_keys,
                           uint64_t bound_keys_cap, uint64_t *bound_used, lv_compact_output_totals *totals) {
    const uint64_t bs = opt ? opt->block_size : LV_SST_DEFAULT_BLOCK_SIZE;
    const uint64_t ri = opt ? opt->restart_interval : LV_SST_DEFAULT_RESTART_INTERVAL;
    if (!totals || !mt_totals || bs < 1 || bs > LV_SST_MAX_BLOCK_SIZE || ri < 1 || ri > LV_SST_MAX_RESTART_INTERVAL)
        return LV_ERR_INVALID;
    if (bloom && (bloom->bits_per_key < 1 || bloom->bits_per_key > 64 || bloom->reserved)) return LV_ERR_INVALID;
    if (!max_file_bytes || level < 1 || level >= LV_NUM_LEVELS || files_cap > LV_VERSION_MAX_FILES ||
        first_number + files_cap < first_number || op_cap > kMaxOps)
        return LV_ERR_INVALID;
    if ((!payload && payload_bytes) || (!arena && arena_cap) || (op_cap && (!ops || !order))) return LV_ERR_INVALID;
    const bool sizing = !arena && !arena_cap;
    if (!sizing && (!handles || (files_cap && (!files || !tables)))) return LV_ERR_INVALID;
    if (!sizing && version_files && (!bound_used || (!bound_keys && bound_keys_cap))) return LV_ERR_INVALID;
    const uint32_t bpk = bloom ? bloom->bits_per_key : 0;
    const uint64_t extra = bpk ? 3 : 2;
    lv_compact_output_totals t{};
    const uint64_t n = mt_totals->entries;
    if (mt_totals->status || n > op_cap) t.status = LV_COMPACT_OUT_NO_TABLE;
    for (uint64_t i = 0; i < n && !t.status; ++i) {  // not the memtable build's arguments: no table
        if (order[i] >= op_cap) {
            t.status = LV_COMPACT_OUT_NO_TABLE;
            break;
        }
        const lv_wb_op &o = ops[order[i]];
        if (!extent_ok(o.key_off, o.key_len, payload_bytes) || !extent_ok(o.val_off, o.val_len, payload_bytes))
            t.status = LV_COMPACT_OUT_NO_TABLE;
    }
    if (t.status) {
        *totals = t;
        return 0;
    }
    // pass 1: upstream's loop, every file sized
    std::vector<Cut> cuts;
    uint64_t at = 0, arena_bytes = 0;
    for (uint64_t i = 0; i < n;) {
        lv_sst_build_totals bt{};
        lv_sst_bloom_totals ft{};
        const uint64_t took = lvgpu_host::sst_build_prefix(payload, ops, order + i, n - i, bs, ri, bpk, max_file_bytes,
                                                           nullptr, 0, nullptr, &bt, &ft);
        if (bt.status) t.status |= LV_COMPACT_OUT_BLOCK_LARGE;
        cuts.push_back(Cut{i, took, bt.file_bytes, bt.data_blocks, bt.index_offset});
        at = (arena_bytes + 15) & ~15ull;  // file_off
        arena_bytes = at + bt.file_bytes;
        t.data_blocks += bt.data_blocks;
        if (version_files) t.bound_bytes += 16ull + ops[order[i]].key_len + ops[order[i + took - 1]].key_len;
        i += took;
    }
    t.entries = n;
    t.files = cuts.size();
    t.arena_bytes = arena_bytes;
    t.handle_pairs = t.data_blocks + extra * t.files;
    if (!sizing) {
        if (t.data_blocks > block_cap) t.status |= LV_COMPACT_OUT_HANDLE_OVER;
        if (t.arena_bytes > arena_cap) t.status |= LV_COMPACT_OUT_ARENA_OVER;
        if (t.files > files_cap) t.status |= LV_COMPACT_OUT_FILES_OVER;
        if (version_files && n && (*bound_used > bound_keys_cap || t.bound_bytes > bound_keys_cap - *bound_used))
            t.status |= LV_COMPACT_OUT_BOUND_OVER;
    }
    *totals = t;
    if (t.status || sizing) return 0;
    // pass 2: the images, and what the readers find in them
    uint64_t off = 0, pair = 0;
    for (size_t k = 0; k < cuts.size(); ++k) {
        const Cut &c = cuts[k];
        lv_sst_build_totals bt{};
        lv_sst_bloom_totals ft{};
        lvgpu_host::sst_build_prefix(payload, ops, order + c.first, n - c.first, bs, ri, bpk, max_file_bytes, arena + off,
                                     c.index_offset, handles + 2 * pair, &bt, &ft);
        lv_compact_output_file f{};
        f.first_entry = c.first;
        f.entries = c.entries;
        f.file_off = off;
        f.file_bytes = c.file_bytes;
        f.data_blocks = c.data_blocks;
        f.first_handle = pair;
        f.filter_keys = bpk ? ft.filter_keys : 0;
        files[k] = f;
        if (int rc = lv_sst_open_host(arena + off, c.file_bytes, nullptr, 0, &tables[k])) return rc;
        if (blooms)
            if (int rc = lv_sst_bloom_open_host(arena + off, &tables[k], &blooms[k])) return rc;
        if (version_files) {
            if (int rc = lv_version_file_host(arena, arena_cap, off, c.file_bytes, &tables[k], first_number + k, level,
                                              bound_keys, bound_keys_cap, bound_used, &version_files[k]))
                return rc;
            version_files[k].file_off += images_off;
        }
        pair += c.data_blocks + extra;
        off = (off + c.file_bytes + 15) & ~15ull;
    }
    return 0;
}

}  // extern "C"
