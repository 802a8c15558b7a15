// lv_version_edit_decode_host: VersionEdit::decode_from (version_edit.rs:236-319)
// over one record, and lv_version_edit_encode_host: encode_to (:192-234) over a
// batch of edits.  The scalar twins of version_edit.hip; host only, no GPU.
#include "../../include/lvgpu/version_edit.h"

#include <cstring>

#include "../../include/lvgpu/crc32c.h"

namespace {

// coding.rs:186-204 over the remaining input [*pos, n).
bool get_varint32(const uint8_t *rec, size_t n, size_t *pos, uint32_t *v) {
    uint32_t result = 0;
    size_t p = *pos;
    for (uint32_t shift = 0; shift <= 28 && p < n; shift += 7) {
        const uint8_t byte = rec[p++];
        result |= static_cast<uint32_t>(byte & 0x7f) << shift;  // bits above 31 of the fifth byte fall off
        if (!(byte & 0x80)) {
            *pos = p;
            *v = result;
            return true;
        }
    }
    return false;
}

// coding.rs:223-241.
bool get_varint64(const uint8_t *rec, size_t n, size_t *pos, uint64_t *v) {
    uint64_t result = 0;
    size_t p = *pos;
    for (uint32_t shift = 0; shift <= 63 && p < n; shift += 7) {
        const uint8_t byte = rec[p++];
        result |= static_cast<uint64_t>(byte & 0x7f) << shift;  // bits above 63 of the tenth byte fall off
        if (!(byte & 0x80)) {
            *pos = p;
            *v = result;
            return true;
        }
    }
    return false;
}

// coding.rs:294-305: the body is skipped, not read.
uint32_t get_varstring(const uint8_t *rec, size_t n, size_t *pos, uint64_t *off, uint32_t *len) {
    uint32_t l;
    if (!get_varint32(rec, n, pos, &l)) return LV_VE_BAD_VARINT32;
    if (n - *pos < l) return LV_VE_BAD_LENGTH;
    *off = *pos;
    *len = l;
    *pos += l;
    return LV_VE_OK;
}

// get_level (version_edit.rs:361-369): the comparison is the i32's.
uint32_t get_level(const uint8_t *rec, size_t n, size_t *pos, uint32_t *level, uint32_t *flags) {
    if (!get_varint32(rec, n, pos, level)) return LV_VE_BAD_VARINT32;
    if (*level & 0x80000000u)
        *flags |= LV_VE_FLAG_NEG_LEVEL;
    else if (*level >= LV_VE_NUM_LEVELS)
        return LV_VE_BAD_LEVEL;
    return LV_VE_OK;
}

}  // namespace

extern "C" uint32_t lv_version_edit_decode_host(const uint8_t *rec, size_t n, lv_ve_edit *edit, lv_ve_file *files,
                                                size_t file_cap, lv_ve_deleted *deleted, size_t deleted_cap,
                                                lv_ve_pointer *pointers, size_t pointer_cap, size_t *counts) {
    lv_ve_edit e{};
    size_t nf = 0, nd = 0, np = 0, pos = 0;
    uint32_t st = LV_VE_OK;
    while (st == LV_VE_OK) {
        uint32_t tag;
        if (!get_varint32(rec, n, &pos, &tag)) {
            if (pos < n) st = LV_VE_INVALID_TAG;
            break;
        }
        uint64_t *scalar = nullptr;
        uint32_t bit = 0;
        switch (tag & 0xffu) {
        case 1:
            if ((st = get_varstring(rec, n, &pos, &e.comparator_off, &e.comparator_len)) == LV_VE_OK)
                e.has |= LV_VE_HAS_COMPARATOR;
            break;
        case 2: scalar = &e.log_number, bit = LV_VE_HAS_LOG_NUMBER; break;
        case 9: scalar = &e.prev_log_number, bit = LV_VE_HAS_PREV_LOG_NUMBER; break;
        case 3: scalar = &e.next_file_number, bit = LV_VE_HAS_NEXT_FILE; break;
        case 4: scalar = &e.last_sequence, bit = LV_VE_HAS_LAST_SEQUENCE; break;
        case 5: {
            lv_ve_pointer p{};
            if ((st = get_level(rec, n, &pos, &p.level, &e.flags)) != LV_VE_OK) break;
            if ((st = get_varstring(rec, n, &pos, &p.key_off, &p.key_len)) != LV_VE_OK) break;
            if (p.key_len < 8) e.flags |= LV_VE_FLAG_SHORT_KEY;
            if (pointers && np < pointer_cap) pointers[np] = p;
            ++np;
            break;
        }
        case 6: {
            lv_ve_deleted d{};
            if ((st = get_level(rec, n, &pos, &d.level, &e.flags)) != LV_VE_OK) break;
            if (!get_varint64(rec, n, &pos, &d.number)) {
                st = LV_VE_BAD_VARINT64;
                break;
            }
            if (deleted && nd < deleted_cap) deleted[nd] = d;
            ++nd;
            break;
        }
        case 7: {
            lv_ve_file f{};
            if ((st = get_level(rec, n, &pos, &f.level, &e.flags)) != LV_VE_OK) break;
            if (!get_varint64(rec, n, &pos, &f.number) || !get_varint64(rec, n, &pos, &f.file_size)) {
                st = LV_VE_BAD_VARINT64;
                break;
            }
            if ((st = get_varstring(rec, n, &pos, &f.smallest_off, &f.smallest_len)) != LV_VE_OK) break;
            if ((st = get_varstring(rec, n, &pos, &f.largest_off, &f.largest_len)) != LV_VE_OK) break;
            if (f.smallest_len < 8 || f.largest_len < 8) e.flags |= LV_VE_FLAG_SHORT_KEY;
            if (files && nf < file_cap) files[nf] = f;
            ++nf;
            break;
        }
        default: st = LV_VE_UNKNOWN_TAG; break;
        }
        if (scalar) {
            if (get_varint64(rec, n, &pos, scalar))
                e.has |= bit;
            else
                st = LV_VE_BAD_VARINT64;
        }
    }
    if (st != LV_VE_OK) {  // the reference returns Err: nothing of the object is a result
        e = lv_ve_edit{};
        nf = nd = np = 0;
    }
    e.status = st;
    if (edit) *edit = e;
    if (counts) {
        counts[0] = nf;
        counts[1] = nd;
        counts[2] = np;
    }
    return st;
}

namespace {

constexpr uint64_t kMaxRecords = 0xfffffffeull;
constexpr uint64_t kMaxRows = 1ull << 30;

bool extent_ok(uint64_t off, uint64_t len, uint64_t bytes) { return off <= bytes && len <= bytes - off; }

// coding.rs' varint at out + at (out may be null: sizing); returns the bytes.
uint32_t put_varint(uint8_t *out, uint64_t at, uint64_t v) {
    uint32_t n = 0;
    for (; v >= 128; v >>= 7, ++n)
        if (out) out[at + n] = static_cast<uint8_t>(v | 0x80);
    if (out) out[at + n] = static_cast<uint8_t>(v);
    return n + 1;
}

uint64_t put_string(uint8_t *out, uint64_t at, const uint8_t *src, uint64_t off, uint32_t len) {
    const uint32_t h = put_varint(out, at, len);
    if (out && len) std::memcpy(out + at + h, src + off, len);
    return static_cast<uint64_t>(h) + len;
}

struct Bad {
    lv_ve_encode_totals *t;
    int operator()(uint64_t status, uint64_t rec, uint64_t kind, uint64_t row) const {
        t->status = status;
        t->bad_record = rec;
        t->bad_kind = kind;
        t->bad_row = row;
        return 0;
    }
};

}  // namespace

extern "C" int lv_version_edit_encode_host(const uint8_t *src, size_t src_bytes, const lv_ve_encode_in *in,
                                           size_t records, const lv_ve_encode_out *out) {
    if (!in || !out || !out->d_totals) return LV_ERR_INVALID;
    uint8_t *dst = out->d_out;
    const bool sizing = !dst && !out->out_cap;  // src is then never read and may be null
    if (!in->d_rec_file || !in->d_rec_deleted || !in->d_rec_pointer || (!src && src_bytes && !sizing) ||
        (!in->d_files && in->file_cap) || (!in->d_deleted && in->deleted_cap) || (!in->d_pointers && in->pointer_cap) ||
        (!dst && out->out_cap) || (records && (!in->d_edits || !out->d_rec_off || !out->d_rec_len)) ||
        records > kMaxRecords || in->file_cap > kMaxRows || in->deleted_cap > kMaxRows || in->pointer_cap > kMaxRows)
        return LV_ERR_INVALID;
    lv_ve_encode_totals &t = *out->d_totals;
    t = lv_ve_encode_totals{};
    t.records = records;
    t.bad_record = t.bad_kind = t.bad_row = ~0ull;
    const Bad bad{&t};
    const uint64_t *pb = in->d_rec_pointer, *db = in->d_rec_deleted, *fb = in->d_rec_file;
    // the bounds, before any row is read
    for (size_t r = 0; r < records; ++r) {
        if (!(pb[r] <= pb[r + 1] && pb[r + 1] <= in->pointer_cap)) return bad(LV_VE_ENCODE_BAD_BOUNDS, r, LV_VE_KIND_POINTER, ~0ull);
        if (!(db[r] <= db[r + 1] && db[r + 1] <= in->deleted_cap)) return bad(LV_VE_ENCODE_BAD_BOUNDS, r, LV_VE_KIND_DELETED, ~0ull);
        if (!(fb[r] <= fb[r + 1] && fb[r + 1] <= in->file_cap)) return bad(LV_VE_ENCODE_BAD_BOUNDS, r, LV_VE_KIND_FILE, ~0ull);
    }
    // every item, kind by kind, before any byte of src is read
    uint64_t kb = 0;
    for (size_t r = 0; r < records; ++r) {
        const lv_ve_edit &e = in->d_edits[r];
        if ((e.has & ~LV_VE_HAS_ALL) ||
            ((e.has & LV_VE_HAS_COMPARATOR) && !extent_ok(e.comparator_off, e.comparator_len, src_bytes)))
            return bad(LV_VE_ENCODE_BAD_ROW, r, LV_VE_KIND_EDIT, r);
        if (e.has & LV_VE_HAS_COMPARATOR) kb += e.comparator_len;
    }
    for (size_t r = 0; r < records; ++r)
        for (uint64_t i = pb[r]; i < pb[r + 1]; ++i) {
            const lv_ve_pointer &p = in->d_pointers[i];
            if (p.level >= LV_VE_NUM_LEVELS || !extent_ok(p.key_off, p.key_len, src_bytes))
                return bad(LV_VE_ENCODE_BAD_ROW, r, LV_VE_KIND_POINTER, i);
            kb += p.key_len;
        }
    for (size_t r = 0; r < records; ++r)
        for (uint64_t i = db[r]; i < db[r + 1]; ++i) {
            const lv_ve_deleted &d = in->d_deleted[i];
            bool ok = d.level < LV_VE_NUM_LEVELS;
            if (ok && i > db[r]) {
                const lv_ve_deleted &q = in->d_deleted[i - 1];
                ok = q.level < d.level || (q.level == d.level && q.number < d.number);
            }
            if (!ok) return bad(LV_VE_ENCODE_BAD_ROW, r, LV_VE_KIND_DELETED, i);
        }
    for (size_t r = 0; r < records; ++r)
        for (uint64_t i = fb[r]; i < fb[r + 1]; ++i) {
            const lv_ve_file &f = in->d_files[i];
            if (f.level >= LV_VE_NUM_LEVELS || !extent_ok(f.smallest_off, f.smallest_len, src_bytes) ||
                !extent_ok(f.largest_off, f.largest_len, src_bytes))
                return bad(LV_VE_ENCODE_BAD_ROW, r, LV_VE_KIND_FILE, i);
            kb += static_cast<uint64_t>(f.smallest_len) + f.largest_len;
        }
    // one loop sizes (w == null) and writes
    for (int pass = sizing ? 1 : 0; pass < 2; ++pass) {
        uint8_t *w = pass && !sizing ? dst : nullptr;
        uint64_t at = 0;
        for (size_t r = 0; r < records; ++r) {
            const uint64_t begin = at;
            const lv_ve_edit &e = in->d_edits[r];
            if (e.has & LV_VE_HAS_COMPARATOR) {
                at += put_varint(w, at, 1);
                at += put_string(w, at, src, e.comparator_off, e.comparator_len);
            }
            const struct { uint32_t bit, tag; uint64_t v; } sc[4] = {{LV_VE_HAS_LOG_NUMBER, 2, e.log_number},
                                                                     {LV_VE_HAS_PREV_LOG_NUMBER, 9, e.prev_log_number},
                                                                     {LV_VE_HAS_NEXT_FILE, 3, e.next_file_number},
                                                                     {LV_VE_HAS_LAST_SEQUENCE, 4, e.last_sequence}};
            for (const auto &s : sc)
                if (e.has & s.bit) {
                    at += put_varint(w, at, s.tag);
                    at += put_varint(w, at, s.v);
                }
            for (uint64_t i = pb[r]; i < pb[r + 1]; ++i) {
                const lv_ve_pointer &p = in->d_pointers[i];
                at += put_varint(w, at, 5);
                at += put_varint(w, at, p.level);
                at += put_string(w, at, src, p.key_off, p.key_len);
            }
            for (uint64_t i = db[r]; i < db[r + 1]; ++i) {
                const lv_ve_deleted &d = in->d_deleted[i];
                at += put_varint(w, at, 6);
                at += put_varint(w, at, d.level);
                at += put_varint(w, at, d.number);
            }
            for (uint64_t i = fb[r]; i < fb[r + 1]; ++i) {
                const lv_ve_file &f = in->d_files[i];
                at += put_varint(w, at, 7);
                at += put_varint(w, at, f.level);
                at += put_varint(w, at, f.number);
                at += put_varint(w, at, f.file_size);
                at += put_string(w, at, src, f.smallest_off, f.smallest_len);
                at += put_string(w, at, src, f.largest_off, f.largest_len);
            }
            if (pass) {
                out->d_rec_off[r] = begin;
                out->d_rec_len[r] = at - begin;
            }
        }
        if (!pass) {  // sized: judge the capacity before any byte is written
            t.out_bytes = at;
            if (at > out->out_cap) {
                t.status = LV_VE_ENCODE_OUT_OVER;
                break;
            }
        }
        t.out_bytes = at;
    }
    t.files = records ? fb[records] - fb[0] : 0;
    t.deleted = records ? db[records] - db[0] : 0;
    t.pointers = records ? pb[records] - pb[0] : 0;
    t.key_bytes = kb;
    return 0;
}
