// The host twins of version.hip (include/lvgpu/version.h): the boundary keys of
// an opened image, the validation of a version's descriptor and Version::Get
// for one query, over host memory, serial, by the core both halves compile
// (lvk/version_read.h).  Host only, no GPU; what tools/version_host_check.cc
// runs under a sanitizer.
#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/version.h"
#include "lvk/version_read.h"

extern "C" {

int lv_version_file_host(const uint8_t *images, uint64_t images_bytes, uint64_t file_off, uint64_t file_cap,
                         const lv_sst_table *table, uint64_t number, uint32_t level, uint8_t *bound_keys,
                         uint64_t bound_keys_cap, uint64_t *bound_used, lv_version_file *out) {
    if (!table || !out || !bound_used || (!images && images_bytes) || (!bound_keys && bound_keys_cap) ||
        level >= LV_NUM_LEVELS)
        return LV_ERR_INVALID;
    lvv::file_fill(images, images_bytes, file_off, file_cap, *table, number, level, bound_keys, bound_keys_cap,
                   bound_used, out);
    return 0;
}

int lv_version_open_host(uint64_t images_bytes, const lv_version_file *files, const lv_sst_table *tables,
                         size_t n_files, const uint8_t *bound_keys, uint64_t bound_keys_bytes, lv_version_state *version) {
    if (!version || (n_files && (!files || !tables)) || (!bound_keys && bound_keys_bytes) ||
        n_files > LV_VERSION_MAX_FILES)
        return LV_ERR_INVALID;
    const lvv::View v{nullptr, images_bytes, files, tables, nullptr, n_files, bound_keys, bound_keys_bytes};
    lv_version_state V{};
    V.files = n_files;
    V.first_bad = n_files;
    for (uint64_t f = 0; f < n_files; ++f) {
        const uint32_t bits = lvv::judge(v, f);
        if (bits && V.first_bad == n_files) V.first_bad = f;
        V.status |= bits;
    }
    if (!V.status) {
        for (uint32_t l = 0; l <= LV_NUM_LEVELS; ++l) V.level_start[l] = n_files;
        for (uint64_t f = n_files; f-- > 0;) {
            uint32_t from, to;
            lvv::starts_of(v, f, &from, &to);
            for (uint32_t l = from; l < to; ++l) V.level_start[l] = f;
        }
    }
    *version = V;
    return 0;
}

int lv_version_get_host(const uint8_t *images, uint64_t images_bytes, const lv_version_file *files,
                        const lv_sst_table *tables, const lv_sst_bloom *blooms, size_t n_files,
                        const uint8_t *bound_keys, uint64_t bound_keys_bytes, const lv_version_state *version,
                        const uint8_t *qkey, size_t qkey_len, uint64_t seq, lv_version_get_result *result) {
    if (!version || !result || (n_files && (!files || !tables)) || (!images && images_bytes) ||
        (!bound_keys && bound_keys_bytes) || (!qkey && qkey_len) || qkey_len > 0xffffffffull ||
        n_files > LV_VERSION_MAX_FILES)
        return LV_ERR_INVALID;
    const lvv::View v{images, images_bytes, files, tables, blooms, n_files, bound_keys, bound_keys_bytes};
    lv_version_get_result r{};
    if (!lvv::version_ok(*version, n_files)) {
        r.status = LV_SST_GET_NO_TABLE;
    } else if (seq > LV_MT_MAX_SEQUENCE) {
        r.status = LV_SST_GET_BAD_SEQ;
    } else {
        const lvr::Target t{qkey, static_cast<uint32_t>(qkey_len), (seq << 8) | LV_WB_TYPE_VALUE};
        lvv::get(v, *version, t, &r);
    }
    *result = r;
    return 0;
}

}  // extern "C"
