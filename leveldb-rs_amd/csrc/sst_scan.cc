// The host twin of sst_scan.hip (include/lvgpu/table.h, "Scan"): a table image
// in host memory back to an op table, serial, by the core both halves compile
// (lvk/sst_scan.h).  Host only, no GPU; the check of the device path that
// tools/sst_scan_host_check.cc runs under a sanitizer and the one-core baseline
// of tools/bench_sst_scan.py.
#include <cstring>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/table.h"
#include "lvk/sst_scan.h"

namespace {

// Every block and run of the table: the counts, or false for CORRUPT.  With
// ops != NULL the entries are written as well (the counts are known to fit).
bool walk_table(const uint8_t *file, const lv_sst_table &t, const lvr::Restarts &ir, uint64_t *entries,
                uint64_t *bytes, uint64_t *runs, uint8_t *arena, lv_wb_op *ops, uint64_t base_e, uint64_t base_b) {
    uint64_t ne = 0, nb = 0, nr = 0;
    for (uint64_t b = 0; b < ir.n; ++b) {
        lvs::Block k;
        if (!lvs::block_header(file, t.file_bytes, t.index_offset, ir, b, &k)) return false;
        const uint8_t *raw = file + k.off;
        for (uint64_t r = 0; r < k.n; ++r, ++nr) {
            if (!ops) {
                uint64_t e, by;
                if (!lvs::run_count(raw, k, r, &e, &by)) return false;
                ne += e;
                nb += by;
                continue;
            }
            lvs::Walk w;
            lvs::Prev p;
            lvs::run_begin(raw, k, r, &w);
            uint64_t at = base_b + nb;
            while (!w.done()) {
                lvr::Entry e{};
                lvs::Copy jobs[3];
                lvs::step(raw, &w, &e);
                const uint64_t next = lvs::emit_entry(raw, e, w.klen, arena, at, &p, &ops[base_e + ne], jobs);
                for (const lvs::Copy &j : jobs)
                    if (j.len) std::memcpy(j.dst, j.src, j.len);
                nb += next - at;
                at = next;
                ++ne;
            }
        }
    }
    *entries = ne;
    *bytes = nb;
    *runs = nr;
    return true;
}

}  // namespace

extern "C" {

int lv_sst_scan_host(const uint8_t *file, const lv_sst_table *table, const lv_sst_scan_totals *prev, uint8_t *arena,
                     uint64_t arena_cap, lv_wb_op *ops, size_t op_cap, uint32_t *order, lv_mt_totals *mt_totals,
                     lv_sst_scan_totals *totals) {
    if (!table || !totals || prev == totals || (!file && table->file_bytes) || (!arena && arena_cap) ||
        (!ops && op_cap) || op_cap > 0xfffffffeull)
        return LV_ERR_INVALID;
    if (!order != !mt_totals || (mt_totals && prev)) return LV_ERR_INVALID;
    lv_sst_scan_totals t{};
    const uint64_t base_e = prev ? prev->entries : 0, base_b = prev ? prev->arena_bytes : 0;
    t.entries = base_e;
    t.arena_bytes = base_b;
    if (prev && prev->status) t.status |= LV_SST_SCAN_UPSTREAM;
    if (table->status) t.status |= LV_SST_SCAN_NO_TABLE;
    lvr::Restarts ir{0, 0};
    if (!t.status && table->file_bytes) {
        if (!lvs::index_header(file, table->file_bytes, table->index_offset, table->index_size, table->data_blocks,
                               &ir)) {
            t.status = LV_SST_SCAN_CORRUPT;
        } else {
            t.data_blocks = ir.n;
            if (!walk_table(file, *table, ir, &t.table_entries, &t.table_bytes, &t.runs, nullptr, nullptr, 0, 0)) {
                t.status = LV_SST_SCAN_CORRUPT;
                t.table_entries = t.table_bytes = t.runs = 0;
            }
        }
    }
    if (!t.status) {
        t.entries = base_e + t.table_entries;
        t.arena_bytes = base_b + t.table_bytes;
        if (lvs::over(base_e, t.table_entries, op_cap)) t.status |= LV_SST_SCAN_OP_OVER;
        if (lvs::over(base_b, t.table_bytes, arena_cap)) t.status |= LV_SST_SCAN_ARENA_OVER;
    }
    if (!t.status && t.table_entries) {
        uint64_t e, b, r;
        walk_table(file, *table, ir, &e, &b, &r, arena, ops, base_e, base_b);
    }
    if (mt_totals) {
        lv_mt_totals m{0, 0, LV_MT_BUILD_UPSTREAM};
        if (!t.status) {
            m = lv_mt_totals{t.table_entries, t.table_entries ? 1u : 0u, 0};
            for (uint64_t i = 0; i < t.table_entries; ++i) {
                order[i] = static_cast<uint32_t>(i);
                if (!i) continue;
                bool same;
                if (lvs::op_compare(arena, ops[i - 1], ops[i], &same) > 0) m.status = LV_SST_SCAN_MT_UNORDERED;
                m.user_keys += !same;
            }
            if (m.status) m.user_keys = 0;
        }
        *mt_totals = m;
    }
    *totals = t;
    return 0;
}

}  // extern "C"
