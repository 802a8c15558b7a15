// The serial core of a version's point lookup (include/lvgpu/version.h):
// lv_version_file's boundary keys, lv_version_open's judgement of one file and
// of the pair in front of it, and Version::Get for one target over the levels.
// One text for both halves, over lvk/sst_read.h: version.cc compiles it for the
// host twins, version.hip for the kernels, so the bounds logic the host check
// program (tools/version_host_check.cc) runs under a sanitizer is the logic a
// lane runs.  Everything here reads images[0, images_bytes), bounds[0,
// bounds_bytes) and the n_files entries of the three arrays only, whatever the
// descriptors say: every extent taken from memory is compared against its
// limit, in u64, before a byte behind it is touched.
//
// No key is materialised by the lookup.  A boundary key is compared in place:
// its user bytes against the query's by common prefix, then the tags.
#pragma once
#include <stdint.h>

#include "../../../include/lvgpu/version.h"
#include "sst_read.h"

namespace lvv {
namespace {

// [off, off + len) lies inside [0, total): u64, no wrap
LVR_FN bool extent(uint64_t off, uint64_t len, uint64_t total) { return off <= total && len <= total - off; }

LVR_FN uint64_t le64(const uint8_t *p) {
    return static_cast<uint64_t>(lvr::le32(p)) | static_cast<uint64_t>(lvr::le32(p + 4)) << 32;
}

// a[0, an) against b[0, bn) bytewise, a proper prefix first: -1, 0, +1
LVR_FN int cmp_bytes(const uint8_t *a, uint32_t an, const uint8_t *b, uint32_t bn) {
    const uint32_t m = an < bn ? an : bn, i = lvr::lcp(a, b, m);
    if (i < m) return a[i] < b[i] ? -1 : 1;
    return an < bn ? -1 : an > bn ? 1 : 0;
}

// InternalKeyComparator of the internal key k[0, kn), kn >= 8, against
// (user key, tag): user key ascending, then tag descending.
LVR_FN int icmp(const uint8_t *k, uint32_t kn, const uint8_t *u, uint32_t un, uint64_t tag) {
    if (const int c = cmp_bytes(k, kn - 8, u, un)) return c;
    const uint64_t kt = le64(k + kn - 8);
    return kt > tag ? -1 : kt < tag ? 1 : 0;
}

// What a lookup is told about a version.  Nothing in it is trusted.
struct View {
    const uint8_t *images;
    uint64_t images_bytes;
    const lv_version_file *files;
    const lv_sst_table *tables;
    const lv_sst_bloom *blooms;  // may be null
    uint64_t n_files;
    const uint8_t *bounds;
    uint64_t bounds_bytes;
};

// a boundary key {off, len} lies inside the bounds and holds a tag
LVR_FN bool bound_ok(uint64_t off, uint32_t len, uint64_t bounds_bytes) {
    return len >= 8 && extent(off, len, bounds_bytes);
}

// ---- lv_version_file: the boundary keys of one opened image ----

// The data block index restart i names: false for anything that does not decode.
LVR_FN bool boundary_block(const uint8_t *file, uint64_t fb, const uint8_t *idx, const lvr::Restarts &r, uint64_t i,
                           uint64_t *off, uint64_t *size) {
    lvr::Entry e;
    if (!lvr::decode(idx, lvr::le32(idx + r.arr + 4 * i), r.arr, &e) || e.shared != 0 || e.non_shared < 8) return false;
    if (!lvr::handle(idx, e.value_at(), e.end(), off, size) || !lvr::in_range(*off, *size, fb)) return false;
    return file[*off + *size] == LV_SST_NO_COMPRESSION;
}

// The last entry's key of the run raw[at, arr): its length in *klen; with dst
// its first `keep` bytes are stored at dst (every key of the run is cut to
// `keep` bytes, which leaves the first `keep` bytes of its successors intact).
// -1 corrupt, 0 no entry, 1 found.
LVR_FN int last_key(const uint8_t *raw, uint64_t at, uint64_t arr, uint64_t *klen, uint8_t *dst, uint64_t keep) {
    uint64_t len = 0, count = 0;
    while (at < arr) {  // every entry is at least 3 bytes: at most arr / 3 rounds
        lvr::Entry e;
        if (!lvr::decode(raw, at, arr, &e) || e.shared > len) return -1;
        len = static_cast<uint64_t>(e.shared) + e.non_shared;
        if (len < 8) return -1;
        if (dst)
            for (uint64_t p = e.shared; p < len && p < keep; ++p) dst[p] = raw[e.key_at + (p - e.shared)];
        ++count;
        at = e.end();
    }
    *klen = len;
    return count ? 1 : 0;
}

// Every field of *out.  *used is read, and advanced when the status is 0.
LVR_FN void file_fill(const uint8_t *images, uint64_t images_bytes, uint64_t file_off, uint64_t file_cap,
                      const lv_sst_table &t, uint64_t number, uint32_t level, uint8_t *bounds, uint64_t bounds_cap,
                      uint64_t *used, lv_version_file *out) {
    lv_version_file f{};
    f.number = number;
    f.file_off = file_off;
    f.file_cap = file_cap;
    f.level = level;
    f.status = [&]() -> uint32_t {
        const uint64_t fb = t.file_bytes;
        if (t.status || fb > file_cap) return LV_VERSION_FILE_NO_TABLE;
        if (!extent(file_off, file_cap, images_bytes)) return LV_VERSION_FILE_BAD_EXTENT;
        if (!fb) return LV_VERSION_FILE_EMPTY;
        const uint8_t *file = images + file_off;
        if (!lvr::in_range(t.index_offset, t.index_size, fb)) return LV_VERSION_FILE_CORRUPT;
        const uint8_t *idx = file + t.index_offset;
        lvr::Restarts r, b;
        if (!lvr::restarts(idx, t.index_size, &r) || r.n < 1) return LV_VERSION_FILE_CORRUPT;
        // smallest: the entry at offset 0 of the first block
        uint64_t so, ss, lo, ls;
        if (!boundary_block(file, fb, idx, r, 0, &so, &ss) || !lvr::restarts(file + so, ss, &b))
            return LV_VERSION_FILE_CORRUPT;
        if (!b.n || !b.arr) return LV_VERSION_FILE_EMPTY;
        lvr::Entry first;
        if (!lvr::decode(file + so, 0, b.arr, &first) || first.shared != 0 || first.non_shared < 8)
            return LV_VERSION_FILE_CORRUPT;
        // largest: the last entry of the last block, from its last restart
        if (!boundary_block(file, fb, idx, r, r.n - 1, &lo, &ls) || !lvr::restarts(file + lo, ls, &b))
            return LV_VERSION_FILE_CORRUPT;
        if (!b.n) return LV_VERSION_FILE_EMPTY;
        const uint64_t from = lvr::le32(file + lo + b.arr + 4 * (b.n - 1));
        uint64_t llen = 0;
        const int got = last_key(file + lo, from, b.arr, &llen, nullptr, 0);
        if (got < 0) return LV_VERSION_FILE_CORRUPT;
        if (!got) return LV_VERSION_FILE_EMPTY;
        const uint64_t need = first.non_shared + llen, at = *used;  // both below 2^32
        if (at > bounds_cap || need > bounds_cap - at) {
            f.reserved = need;
            return LV_VERSION_FILE_BOUND_OVER;
        }
        for (uint32_t i = 0; i < first.non_shared; ++i) bounds[at + i] = file[so + first.key_at + i];
        last_key(file + lo, from, b.arr, &llen, bounds + at + first.non_shared, llen);
        f.smallest_off = at;
        f.smallest_len = first.non_shared;
        f.largest_off = at + first.non_shared;
        f.largest_len = static_cast<uint32_t>(llen);
        *used = at + need;
        return 0u;
    }();
    *out = f;
}

// ---- lv_version_open: file f, and the pair (f - 1, f) ----

LVR_FN bool bounds_ok(const lv_version_file &F, uint64_t bounds_bytes) {
    return bound_ok(F.smallest_off, F.smallest_len, bounds_bytes) && bound_ok(F.largest_off, F.largest_len, bounds_bytes);
}

LVR_FN uint32_t judge(const View &v, uint64_t f) {
    const lv_version_file F = v.files[f];
    const lv_sst_table &T = v.tables[f];
    uint32_t bits = 0;
    if (F.status || F.level >= LV_NUM_LEVELS || !extent(F.file_off, F.file_cap, v.images_bytes) || !T.file_bytes ||
        T.file_bytes > F.file_cap)
        bits |= LV_VERSION_OPEN_BAD_FILE;
    if (T.status) bits |= LV_VERSION_OPEN_BAD_TABLE;
    const bool ok = bounds_ok(F, v.bounds_bytes);
    if (!ok) {
        bits |= LV_VERSION_OPEN_BAD_BOUND;
    } else {
        const uint8_t *l = v.bounds + F.largest_off;
        if (icmp(v.bounds + F.smallest_off, F.smallest_len, l, F.largest_len - 8, le64(l + F.largest_len - 8)) > 0)
            bits |= LV_VERSION_OPEN_BAD_BOUND;
    }
    if (f) {
        const lv_version_file P = v.files[f - 1];
        if (P.level > F.level) {
            bits |= LV_VERSION_OPEN_UNSORTED;
        } else if (P.level == F.level) {
            if (F.level == 0) {
                if (P.number <= F.number) bits |= LV_VERSION_OPEN_UNSORTED;
            } else if (ok && bounds_ok(P, v.bounds_bytes)) {  // (a bad bound is its own lane's BAD_BOUND)
                const uint8_t *s = v.bounds + F.smallest_off;
                if (icmp(v.bounds + P.largest_off, P.largest_len, s, F.smallest_len - 8, le64(s + F.smallest_len - 8)) >= 0)
                    bits |= LV_VERSION_OPEN_UNSORTED;
            }
        }
    }
    return bits;
}

// the levels l whose level_start is f in a version that is in order: those in
// [*from, *to), none when from >= to (levels above that of f - 1, up to f's)
LVR_FN void starts_of(const View &v, uint64_t f, uint32_t *from, uint32_t *to) {
    const uint32_t lf = v.files[f].level, lp = f ? v.files[f - 1].level : 0u;
    *to = lf < LV_NUM_LEVELS ? lf + 1 : 0u;
    *from = f ? (lp < LV_NUM_LEVELS ? lp + 1 : LV_NUM_LEVELS) : 0u;
}

// ---- lv_version_get ----

// *V is sound enough to search by: its level_start are in order inside
// [0, n_files] and it speaks of n_files files.
LVR_FN bool version_ok(const lv_version_state &V, uint64_t n_files) {
    if (V.status || V.files != n_files || V.level_start[0] != 0 || V.level_start[LV_NUM_LEVELS] != n_files) return false;
    for (uint32_t l = 0; l < LV_NUM_LEVELS; ++l)
        if (V.level_start[l] > V.level_start[l + 1]) return false;
    return true;
}

// Version::Get for one target: every field of *res.  The caller has decided
// NO_TABLE (version_ok), BAD_SEQ and BAD_QUERY.
LVR_FN void get(const View &v, const lv_version_state &V, const lvr::Target &t, lv_version_get_result *res) {
    lv_version_get_result out{};
    const lv_version_get_result no_table{0, 0, 0, 0, LV_SST_GET_NO_TABLE, 0, 0, 0, 0, 0};
    uint64_t last = ~0ull;
    uint64_t i = 0;        // level 0: the next file to look at
    uint32_t level = 0;
    for (;;) {
        uint64_t f = ~0ull;  // the next file to visit
        if (level == 0) {
            const uint64_t end = V.level_start[1];
            while (i < end && f == ~0ull) {
                const lv_version_file *F = v.files + i;
                const uint64_t so = F->smallest_off, lo = F->largest_off;
                const uint32_t sl = F->smallest_len, ll = F->largest_len;
                if (!bound_ok(so, sl, v.bounds_bytes) || !bound_ok(lo, ll, v.bounds_bytes)) {
                    *res = no_table;
                    return;
                }
                if (cmp_bytes(t.q, t.ql, v.bounds + so, sl - 8) >= 0 && cmp_bytes(t.q, t.ql, v.bounds + lo, ll - 8) <= 0)
                    f = i;
                ++i;
            }
            if (f == ~0ull) {
                level = 1;
                continue;
            }
        } else if (level >= LV_NUM_LEVELS) {
            break;
        } else {
            const uint64_t first = V.level_start[level], n = V.level_start[level + 1] - first;
            ++level;
            uint64_t lo = 0, hi = n;  // FindFile: the first file whose largest is not less than the target
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                const lv_version_file *F = v.files + first + mid;
                const uint64_t o = F->largest_off;
                const uint32_t l = F->largest_len;
                if (!bound_ok(o, l, v.bounds_bytes)) {
                    *res = no_table;
                    return;
                }
                if (icmp(v.bounds + o, l, t.q, t.ql, t.tag) < 0)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo >= n) continue;
            const lv_version_file *F = v.files + first + lo;
            const uint64_t o = F->smallest_off;
            const uint32_t l = F->smallest_len;
            if (!bound_ok(o, l, v.bounds_bytes)) {
                *res = no_table;
                return;
            }
            if (cmp_bytes(t.q, t.ql, v.bounds + o, l - 8) < 0) continue;
            f = first + lo;
        }
        // visit(f)
        const uint64_t file_off = v.files[f].file_off, file_cap = v.files[f].file_cap;
        const lv_sst_table *T = v.tables + f;
        const uint64_t fb = T->file_bytes;
        if (!extent(file_off, file_cap, v.images_bytes) || T->status || fb > file_cap) {
            *res = no_table;
            return;
        }
        if (last != ~0ull && out.seek_file == 0) out.seek_file = static_cast<uint32_t>(last) + 1;
        last = f;
        ++out.files_read;
        lv_sst_get_result r{};
        // (the filter is read where it lies: lvr::may_match checks every field of it again)
        const lv_sst_bloom *bp = v.blooms && v.blooms[f].present == 1 ? v.blooms + f : nullptr;
        const uint32_t st = lvr::get(v.images + file_off, fb, T->index_offset, T->index_size, t, &r, bp);
        if (r.reserved == LV_SST_GET_FILTERED) ++out.filtered;
        if (st == LV_SST_GET_ABSENT) continue;
        out.status = st;
        out.file = static_cast<uint32_t>(f);
        out.level = v.files[f].level;
        if (st != LV_SST_GET_CORRUPT) {
            out.tag = r.tag;
            out.block = r.block;
        }
        if (st == LV_SST_GET_FOUND) {
            out.val_off = file_off + r.val_off;
            out.val_len = r.val_len;
        }
        break;
    }
    *res = out;
}

}  // namespace
}  // namespace lvv
