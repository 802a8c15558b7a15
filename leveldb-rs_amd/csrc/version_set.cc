// lv_version_apply_host (include/lvgpu/version_set.h): the serial twin of
// version_set.hip, host only, no GPU.  It is upstream's VersionSet::Builder
// written out (db/version_set.cc): per level a set of deleted file numbers and
// a set of added files under the version's order; Apply over every record
// (compact pointers, deleted files, then new files, each new file leaving the
// deleted set); SaveTo, which keeps an added file unless its number is in the
// deleted set -- with Recover's bookkeeping of the scalars around it.  The
// device states the same result per pair (the largest deleting record, the
// lowest adding row), so the two agree only if both are right.
#include "../../include/lvgpu/version_set.h"

#include <cstring>
#include <set>
#include <unordered_set>
#include <vector>

#include "../../include/lvgpu/crc32c.h"

namespace {

constexpr uint64_t kMaxRecords = 0xfffffffeull;
constexpr uint64_t kMaxRows = 1ull << 30;

bool extent_ok(uint64_t off, uint64_t len, uint64_t bytes) { return off <= bytes && len <= bytes - off; }

// InternalKeyComparator over two internal keys of at least 8 bytes: user key
// ascending bytewise, then the tag (8 little-endian bytes) descending.
int icmp(const uint8_t *a, uint32_t alen, const uint8_t *b, uint32_t blen) {
    const uint32_t ua = alen - 8, ub = blen - 8, m = ua < ub ? ua : ub;
    const int c = m ? std::memcmp(a, b, m) : 0;
    if (c) return c < 0 ? -1 : 1;
    if (ua != ub) return ua < ub ? -1 : 1;
    uint64_t ta, tb;
    std::memcpy(&ta, a + ua, 8);
    std::memcpy(&tb, b + ub, 8);
    return ta > tb ? -1 : ta < tb ? 1 : 0;
}

// The order of a level's files (version.h): level 0 newest first; deeper
// levels by smallest key, then number (upstream's BySmallestKey).
struct FileOrder {
    const uint8_t *src;
    const lv_ve_file *files;
    bool level0;
    bool operator()(uint64_t x, uint64_t y) const {
        const lv_ve_file &a = files[x], &b = files[y];
        if (level0) return a.number > b.number;
        const int c = icmp(src + a.smallest_off, a.smallest_len, src + b.smallest_off, b.smallest_len);
        if (c) return c < 0;
        return a.number < b.number;
    }
};

struct LevelState {  // Builder::LevelState
    std::set<uint64_t> deleted_files;
    std::set<uint64_t, FileOrder> added_files;  // NewFile row indices
    explicit LevelState(const FileOrder &o) : added_files(o) {}
};

int refuse(lv_vs_totals &t, uint64_t records, uint64_t status, uint64_t kind, uint64_t row) {
    t = lv_vs_totals{};
    t.records = records;
    t.status = status;
    t.bad_kind = kind;
    t.bad_row = row;
    return 0;
}

}  // namespace

extern "C" int lv_version_apply_host(const uint8_t *src, size_t src_bytes, const lv_ve_encode_in *in, size_t records,
                                     const lv_vs_placement *dir, size_t dir_n, const lv_vs_out *out) {
    if (!in || !out || !out->d_totals) return LV_ERR_INVALID;
    if (!in->d_rec_file || !in->d_rec_deleted || !in->d_rec_pointer || (!src && src_bytes) ||
        (!in->d_files && in->file_cap) || (!in->d_deleted && in->deleted_cap) || (!in->d_pointers && in->pointer_cap) ||
        (records && !in->d_edits) || (!dir && dir_n) || (!out->d_files_out && out->files_cap) || records > kMaxRecords ||
        in->file_cap > kMaxRows || in->deleted_cap > kMaxRows || in->pointer_cap > kMaxRows || dir_n > kMaxRows ||
        out->files_cap > LV_VERSION_MAX_FILES)
        return LV_ERR_INVALID;
    lv_vs_totals &t = *out->d_totals;
    const uint64_t *pb = in->d_rec_pointer, *db = in->d_rec_deleted, *fb = in->d_rec_file;
    // the bounds, before any row is read
    for (size_t r = 0; r < records; ++r) {
        if (!(pb[r] <= pb[r + 1] && pb[r + 1] <= in->pointer_cap)) return refuse(t, records, LV_VS_BAD_BOUNDS, LV_VE_KIND_POINTER, r);
        if (!(db[r] <= db[r + 1] && db[r + 1] <= in->deleted_cap)) return refuse(t, records, LV_VS_BAD_BOUNDS, LV_VE_KIND_DELETED, r);
        if (!(fb[r] <= fb[r + 1] && fb[r + 1] <= in->file_cap)) return refuse(t, records, LV_VS_BAD_BOUNDS, LV_VE_KIND_FILE, r);
    }
    const uint64_t p0 = records ? pb[0] : 0, p1 = records ? pb[records] : 0;
    const uint64_t d0 = records ? db[0] : 0, d1 = records ? db[records] : 0;
    const uint64_t f0 = records ? fb[0] : 0, f1 = records ? fb[records] : 0;
    // every row, kind by kind, before any byte of src is read
    for (uint64_t i = p0; i < p1; ++i) {
        const lv_ve_pointer &p = in->d_pointers[i];
        if (p.level >= LV_NUM_LEVELS || p.key_len < 8 || !extent_ok(p.key_off, p.key_len, src_bytes))
            return refuse(t, records, LV_VS_BAD_ROW, LV_VE_KIND_POINTER, i);
    }
    for (uint64_t i = d0; i < d1; ++i) {
        const lv_ve_deleted &d = in->d_deleted[i];
        if (d.level >= LV_NUM_LEVELS || d.number >= LV_VS_MAX_NUMBER) return refuse(t, records, LV_VS_BAD_ROW, LV_VE_KIND_DELETED, i);
    }
    for (uint64_t i = f0; i < f1; ++i) {
        const lv_ve_file &f = in->d_files[i];
        if (f.level >= LV_NUM_LEVELS || f.number >= LV_VS_MAX_NUMBER || f.smallest_len < 8 || f.largest_len < 8 ||
            !extent_ok(f.smallest_off, f.smallest_len, src_bytes) || !extent_ok(f.largest_off, f.largest_len, src_bytes))
            return refuse(t, records, LV_VS_BAD_ROW, LV_VE_KIND_FILE, i);
    }
    {  // LevelDB never reuses a file number: a pair is added once
        std::unordered_set<uint64_t> seen;
        seen.reserve(f1 - f0);
        for (uint64_t i = f0; i < f1; ++i)
            if (!seen.insert((static_cast<uint64_t>(in->d_files[i].level) << 56) | in->d_files[i].number).second)
                return refuse(t, records, LV_VS_DUPLICATE, LV_VE_KIND_FILE, i);
    }
    for (size_t i = 1; i < dir_n; ++i)
        if (dir[i - 1].number >= dir[i].number) return refuse(t, records, LV_VS_BAD_DIRECTORY, LV_VS_KIND_DIRECTORY, i);

    t = lv_vs_totals{};
    t.records = records;
    t.bad_kind = t.bad_row = ~0ull;
    t.new_files = f1 - f0;
    t.deleted = d1 - d0;
    t.pointers = p1 - p0;
    std::vector<LevelState> levels;
    for (uint32_t l = 0; l < LV_NUM_LEVELS; ++l) levels.emplace_back(FileOrder{src, in->d_files, l == 0});
    bool have_log = false, have_prev = false;
    for (size_t r = 0; r < records; ++r) {
        // Builder::Apply
        for (uint64_t i = pb[r]; i < pb[r + 1]; ++i) t.compact_pointer[in->d_pointers[i].level] = i + 1;
        for (uint64_t i = db[r]; i < db[r + 1]; ++i) levels[in->d_deleted[i].level].deleted_files.insert(in->d_deleted[i].number);
        for (uint64_t i = fb[r]; i < fb[r + 1]; ++i) {
            LevelState &L = levels[in->d_files[i].level];
            L.deleted_files.erase(in->d_files[i].number);
            L.added_files.insert(i);
        }
        // Recover's loop over the edit's scalars
        const lv_ve_edit &e = in->d_edits[r];
        if (e.has & LV_VE_HAS_COMPARATOR) {
            t.comparator_off = e.comparator_off;
            t.comparator_len = e.comparator_len;
        }
        if (e.has & LV_VE_HAS_LOG_NUMBER) {
            t.log_number = e.log_number;
            have_log = true;
        }
        if (e.has & LV_VE_HAS_PREV_LOG_NUMBER) {
            t.prev_log_number = e.prev_log_number;
            have_prev = true;
        }
        if (e.has & LV_VE_HAS_NEXT_FILE) t.next_file_number = e.next_file_number;
        if (e.has & LV_VE_HAS_LAST_SEQUENCE) t.last_sequence = e.last_sequence;
        t.has |= e.has & LV_VE_HAS_ALL;
    }
    // MarkFileNumberUsed(log_number), then (prev_log_number)
    if (have_log && t.next_file_number <= t.log_number) t.next_file_number = t.log_number + 1;
    if (have_prev && t.next_file_number <= t.prev_log_number) t.next_file_number = t.prev_log_number + 1;
    // Builder::SaveTo over an empty base: MaybeAddFile drops a file whose number was deleted after it was added
    std::vector<uint64_t> rows;
    for (uint32_t l = 0; l < LV_NUM_LEVELS; ++l)
        for (uint64_t i : levels[l].added_files) {
            const lv_ve_file &f = in->d_files[i];
            if (levels[l].deleted_files.count(f.number)) continue;
            rows.push_back(i);
            ++t.level_files[l];
            t.level_bytes[l] += f.file_size;
            if (f.number > t.max_file_number) t.max_file_number = f.number;
        }
    t.live = rows.size();
    // the placements
    std::vector<uint32_t> at(rows.size(), LV_VS_NO_DIR_INDEX);
    for (size_t j = 0; j < rows.size() && dir_n; ++j) {
        const lv_ve_file &f = in->d_files[rows[j]];
        size_t lo = 0, hi = dir_n;
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (dir[mid].number < f.number)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo < dir_n && dir[lo].number == f.number && dir[lo].file_cap >= f.file_size)
            at[j] = static_cast<uint32_t>(lo);
        else
            ++t.unplaced;
    }
    if (t.live > out->files_cap) {
        t.status = LV_VS_FILE_OVER;
        return 0;
    }
    for (size_t j = 0; j < rows.size(); ++j) {
        const lv_ve_file &f = in->d_files[rows[j]];
        lv_version_file o{};
        o.number = f.number;
        if (at[j] != LV_VS_NO_DIR_INDEX) {
            o.file_off = dir[at[j]].file_off;
            o.file_cap = dir[at[j]].file_cap;
        } else if (!dir_n) {
            o.file_cap = f.file_size;
        } else {
            o.status = LV_VERSION_FILE_UNPLACED;
        }
        o.smallest_off = f.smallest_off;
        o.largest_off = f.largest_off;
        o.smallest_len = f.smallest_len;
        o.largest_len = f.largest_len;
        o.level = f.level;
        o.reserved = rows[j];
        out->d_files_out[j] = o;
        if (out->d_dir_index) out->d_dir_index[j] = at[j];
    }
    return 0;
}
