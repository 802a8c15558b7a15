// The host twin of sst_build.hip (include/lvgpu/table.h): the sorted memtable
// to an SSTable image, as a serial restatement of upstream LevelDB's
// BlockBuilder / TableBuilder (the header spells the format out).  Host only,
// no GPU; the model-independent check of the device path and the baseline of
// tools/bench_sst_build.py.  Two runs of one serial walk: the first sizes the
// table and decides the status, the second writes (the index block's place in
// the file is known only after the first).
#include <cstring>
#include <optional>
#include <vector>

#include "../../include/lvgpu/crc32c.h"
#include "../../include/lvgpu/table.h"
#include "lvk/sst_read.h"
#include "sst_build_host.h"

namespace {

constexpr uint64_t kMaxOps = 0xfffffffeull;
constexpr uint64_t kLargeBlock = 0xffffffffull;  // raw sizes from here on: sst_in_range refuses them
const uint8_t kMaxTag[8] = {0x01, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff};

struct IKey {  // an internal key: ulen user bytes at k, then the 8 tag bytes
    const uint8_t *k;
    uint64_t ulen;
    uint8_t tag[8];
    uint64_t len() const { return ulen + 8; }
    uint8_t at(uint64_t i) const { return i < ulen ? k[i] : tag[i - ulen]; }
};

void put_tag(uint8_t *dst, uint64_t tag) {
    for (int i = 0; i < 8; ++i) dst[i] = static_cast<uint8_t>(tag >> (8 * i));
}

uint64_t varint_len(uint64_t v) {
    uint64_t n = 1;
    while (v >= 128) {
        v >>= 7;
        ++n;
    }
    return n;
}

// where the bytes go: nowhere (sizing) or into the file
struct Sink {
    uint8_t *file;  // NULL: sizing
    void bytes(uint64_t at, const uint8_t *src, uint64_t n) const {
        if (file && n) std::memcpy(file + at, src, n);
    }
    uint64_t varint(uint64_t at, uint64_t v) const {
        const uint64_t n = varint_len(v);
        if (file) {
            uint8_t *p = file + at;
            while (v >= 128) {
                *p++ = static_cast<uint8_t>(v | 0x80);
                v >>= 7;
            }
            *p = static_cast<uint8_t>(v);
        }
        return n;
    }
    void fixed32(uint64_t at, uint64_t v) const {
        if (file)
            for (int i = 0; i < 4; ++i) file[at + i] = static_cast<uint8_t>(v >> (8 * i));
    }
    void trailer(uint64_t off, uint64_t size) const {
        if (!file) return;
        const uint8_t type = LV_SST_NO_COMPRESSION;
        const uint32_t crc = lv_crc32c_mask(lv_crc32c_extend(lv_crc32c_extend(0, file + off, size), &type, 1));
        file[off + size] = type;
        fixed32(off + size + 1, crc);
    }
};

// A BlockBuilder writing at file offset `base`.
struct Block {
    const Sink &out;
    uint64_t base, interval;
    uint64_t buffer = 0, counter = 0;
    std::vector<uint64_t> restarts{0};
    bool has_last = false;
    IKey last{};
    Block(const Sink &o, uint64_t b, uint64_t ri) : out(o), base(b), interval(ri) {}
    bool empty() const { return buffer == 0; }
    uint64_t estimate() const { return buffer + 4 * restarts.size() + 4; }
    void add(const IKey &key, const uint8_t *value, uint64_t vlen) {
        uint64_t shared = 0;
        if (counter < interval) {
            if (has_last) {
                const uint64_t m = last.len() < key.len() ? last.len() : key.len();
                while (shared < m && last.at(shared) == key.at(shared)) ++shared;
            }
        } else {
            restarts.push_back(buffer);
            counter = 0;
        }
        uint64_t at = base + buffer;
        at += out.varint(at, shared);
        at += out.varint(at, key.len() - shared);
        at += out.varint(at, vlen);
        if (shared < key.ulen) {
            out.bytes(at, key.k + shared, key.ulen - shared);
            at += key.ulen - shared;
            out.bytes(at, key.tag, 8);
            at += 8;
        } else {
            out.bytes(at, key.tag + (shared - key.ulen), key.len() - shared);
            at += key.len() - shared;
        }
        out.bytes(at, value, vlen);
        at += vlen;
        buffer = at - base;
        last = key;
        has_last = true;
        ++counter;
    }
    // The only entry of a block whose key is a plain byte string, not an
    // internal key (the metaindex block's): shared = 0.
    void add_only(const uint8_t *key, uint64_t klen, const uint8_t *value, uint64_t vlen) {
        uint64_t at = base;
        at += out.varint(at, 0);
        at += out.varint(at, klen);
        at += out.varint(at, vlen);
        out.bytes(at, key, klen);
        out.bytes(at + klen, value, vlen);
        buffer = at + klen + vlen - base;
        ++counter;
    }
    uint64_t finish() {  // the raw size
        uint64_t at = base + buffer;
        for (uint64_t r : restarts) {
            out.fixed32(at, r);
            at += 4;
        }
        out.fixed32(at, restarts.size());
        return at + 4 - base;
    }
};

// shortest_separator(a, b) / short_successor(a) as the key's parts: `copy`
// bytes of u(a), then (bump) the byte u(a)[copy] + 1 and MAXTAG, or a's tag.
struct Sep {
    uint64_t copy;
    bool bump;
};
Sep shortest_separator(const IKey &a, const IKey &b) {
    const uint64_t m = a.ulen < b.ulen ? a.ulen : b.ulen;
    uint64_t d = 0;
    while (d < m && a.k[d] == b.k[d]) ++d;
    if (d >= m) return {a.ulen, false};
    const unsigned c = a.k[d];
    if (c < 0xff && c + 1 < b.k[d]) return {d, true};
    return {a.ulen, false};
}
Sep short_successor(const IKey &a) {
    uint64_t i = 0;
    while (i < a.ulen && a.k[i] == 0xff) ++i;
    if (i >= a.ulen || i + 1 >= a.ulen) return {a.ulen, false};
    return {i, true};
}

// BloomFilterPolicy::CreateFilter over n key hashes into dst[0, bytes + 1).
uint32_t bloom_k(uint32_t bpk) {
    const uint32_t k = bpk * 69 / 100;
    return k < 1 ? 1 : k > 30 ? 30 : k;
}
uint64_t bloom_bytes(uint64_t n, uint32_t bpk) {  // without the k byte
    const unsigned __int128 want = static_cast<unsigned __int128>(n) * bpk;
    const unsigned __int128 bits = want < 64 ? 64 : want;
    const unsigned __int128 bytes = (bits + 7) / 8;
    return bytes > (1ull << 62) ? 1ull << 62 : static_cast<uint64_t>(bytes);  // (no table comes near)
}
void bloom_fill(uint8_t *dst, uint64_t bytes, uint32_t bpk, const uint32_t *hashes, uint64_t n) {
    const uint64_t bits = bytes * 8;
    const uint32_t k = bloom_k(bpk);
    std::memset(dst, 0, bytes);
    dst[bytes] = static_cast<uint8_t>(k);
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t h = hashes[i];
        const uint32_t delta = (h >> 17) | (h << 15);
        for (uint32_t j = 0; j < k; ++j) {
            const uint64_t pos = h % bits;
            dst[pos / 8] |= static_cast<uint8_t>(1u << (pos % 8));
            h += delta;
        }
    }
}

// FilterBlockBuilder (base lg 11), keys held as their Bloom hashes.
struct FilterBlock {
    uint32_t bpk;
    std::vector<uint32_t> pending;
    std::vector<uint8_t> result;
    std::vector<uint64_t> offsets;
    uint64_t keys = 0;
    void add(const uint8_t *k, uint64_t n) {
        pending.push_back(lvr::hash(k, n, lvr::kBloomSeed));
        ++keys;
    }
    void generate() {
        offsets.push_back(result.size());
        if (pending.empty()) return;
        const uint64_t bytes = bloom_bytes(pending.size(), bpk), at = result.size();
        result.resize(at + bytes + 1);
        bloom_fill(result.data() + at, bytes, bpk, pending.data(), pending.size());
        pending.clear();
    }
    void start_block(uint64_t offset) {
        while ((offset >> LV_SST_FILTER_BASE_LG) > offsets.size()) generate();
    }
    uint64_t finish_size() {  // the block's size; the array follows the filters
        if (!pending.empty()) generate();
        return result.size() + 4 * offsets.size() + 5;
    }
};

struct Run {
    const uint8_t *payload;
    const lv_wb_op *ops;
    const uint32_t *order;
    uint64_t n, block_size, interval;
    uint32_t bpk;  // 0: no filter policy
    // one output file of a compaction (compact_output.cc): the walk ends with the
    // add after which the flushed bytes reach max_file (0: no limit)
    uint64_t max_file = 0;
};

IKey ikey(const Run &R, uint64_t i) {
    const lv_wb_op &o = R.ops[R.order[i]];
    IKey k;
    k.k = R.payload + o.key_off;
    k.ulen = o.key_len;
    put_tag(k.tag, o.tag);
    return k;
}

// One walk.  index_at: where the index block goes (the write pass knows it
// from the sizing pass).  handles is NULL in a sizing pass; a write pass runs
// only with data_blocks <= block_cap, so it has room for data_blocks + 2 pairs
// (+ 3 with a filter policy: the filter block's comes before the metaindex's).
// Returns the entries added: R.n unless R.max_file ended the walk.
uint64_t walk(const Run &R, const Sink &out, uint64_t index_at, uint64_t *handles, lv_sst_build_totals *t,
              lv_sst_bloom_totals *bt) {
    uint64_t offset = 0, blocks = 0;
    bool large = false;
    Block index(out, index_at, 1);
    std::vector<uint8_t> scratch;  // a separator's bytes: the index block keeps pointers into it
    bool pending = false;
    uint64_t pend_off = 0, pend_size = 0;
    IKey last{};
    FilterBlock filter{R.bpk};
    uint64_t added = 0;
    auto add_index = [&](const Sep &s) {
        IKey k;
        k.k = last.k;
        k.ulen = s.copy;
        std::memcpy(k.tag, last.tag, 8);
        if (s.bump) {  // u(a)[:copy] + byte + MAXTAG: the bumped byte leads the "tag" part
            scratch.resize(s.copy + 1);
            if (s.copy) std::memcpy(scratch.data(), last.k, s.copy);
            scratch[s.copy] = static_cast<uint8_t>(last.k[s.copy] + 1);
            k.k = scratch.data();
            k.ulen = s.copy + 1;
            std::memcpy(k.tag, kMaxTag, 8);
        }
        uint8_t h[LV_SST_BLOCK_HANDLE_MAX];
        const size_t hn = lv_sst_block_handle_encode(pend_off, pend_size, h);
        index.add(k, h, hn);
        pending = false;
    };
    auto write_block = [&](Block &b) {
        const uint64_t size = b.finish();
        if (size >= kLargeBlock) large = true;
        out.trailer(offset, size);
        if (handles) {
            handles[2 * blocks] = offset;
            handles[2 * blocks + 1] = size;
        }
        pend_off = offset;
        pend_size = size;
        offset += size + LV_SST_TRAILER_SIZE;
        if (R.bpk) filter.start_block(offset);
    };
    if (R.n) {
        std::optional<Block> data;
        data.emplace(out, 0, R.interval);
        for (uint64_t i = 0; i < R.n; ++i) {
            const lv_wb_op &o = R.ops[R.order[i]];
            const IKey key = ikey(R, i);
            if (pending) add_index(shortest_separator(last, key));
            last = key;
            if (R.bpk) filter.add(key.k, key.ulen);
            data->add(key, R.payload + o.val_off, o.val_len);
            if (data->estimate() >= R.block_size) {
                write_block(*data);
                ++blocks;
                pending = true;
                data.emplace(out, offset, R.interval);
                if (R.max_file && offset >= R.max_file) {  // DoCompactionWork closes the file here
                    added = i + 1;
                    break;
                }
            }
            added = i + 1;
        }
        if (!data->empty()) {
            write_block(*data);
            ++blocks;
            pending = true;
        }
    }
    t->data_blocks = blocks;
    if (!R.n) return 0;  // no file
    uint64_t nh = blocks;  // the next handle pair
    uint8_t fh[LV_SST_BLOCK_HANDLE_MAX];
    size_t fhn = 0;
    if (R.bpk) {  // the filter block: the filters, their offsets, array_offset, the base
        const uint64_t size = filter.finish_size(), array = filter.result.size();
        if (size >= kLargeBlock) large = true;
        if (out.file) {
            out.bytes(offset, filter.result.data(), array);
            uint64_t at = offset + array;
            for (uint64_t o : filter.offsets) {
                out.fixed32(at, o);
                at += 4;
            }
            out.fixed32(at, array);
            out.file[at + 4] = LV_SST_FILTER_BASE_LG;
        }
        out.trailer(offset, size);
        if (handles) {
            handles[2 * nh] = offset;
            handles[2 * nh + 1] = size;
        }
        ++nh;
        bt->filter_offset = offset;
        bt->filter_size = size;
        bt->filters = filter.offsets.size();
        bt->filter_keys = filter.keys;
        fhn = lv_sst_block_handle_encode(offset, size, fh);
        offset += size + LV_SST_TRAILER_SIZE;
    }
    // the metaindex block: an empty BlockBuilder, or one with the filter's entry
    Block meta(out, offset, R.interval);
    if (R.bpk) {
        static const uint8_t name[] = LV_SST_BLOOM_NAME;
        meta.add_only(name, sizeof(name) - 1, fh, fhn);
    }
    t->metaindex_offset = offset;
    t->metaindex_size = meta.finish();
    out.trailer(offset, t->metaindex_size);
    if (handles) {
        handles[2 * nh] = offset;
        handles[2 * nh + 1] = t->metaindex_size;
    }
    ++nh;
    offset += t->metaindex_size + LV_SST_TRAILER_SIZE;
    if (pending) add_index(short_successor(last));
    t->index_offset = offset;
    t->index_size = index.finish();
    if (t->index_size >= kLargeBlock) large = true;
    out.trailer(offset, t->index_size);
    if (handles) {
        handles[2 * nh] = offset;
        handles[2 * nh + 1] = t->index_size;
    }
    offset += t->index_size + LV_SST_TRAILER_SIZE;
    if (out.file)
        lv_sst_footer_encode(t->metaindex_offset, t->metaindex_size, t->index_offset, t->index_size, out.file + offset);
    t->file_bytes = offset + LV_SST_FOOTER_SIZE;
    if (large) t->status |= LV_SST_BUILD_BLOCK_LARGE;
    return added;
}

bool extent_ok(uint64_t off, uint64_t len, uint64_t bytes) { return off <= bytes && len <= bytes - off; }

bool options_ok(const lv_sst_build_options *opt, uint64_t *bs, uint64_t *ri) {
    *bs = opt ? opt->block_size : LV_SST_DEFAULT_BLOCK_SIZE;
    *ri = opt ? opt->restart_interval : LV_SST_DEFAULT_RESTART_INTERVAL;
    return *bs >= 1 && *bs <= LV_SST_MAX_BLOCK_SIZE && *ri >= 1 && *ri <= LV_SST_MAX_RESTART_INTERVAL;
}

}  // namespace

uint64_t lvgpu_host::sst_build_prefix(const uint8_t *payload, const lv_wb_op *ops, const uint32_t *order, uint64_t n,
                                      uint64_t block_size, uint64_t restart_interval, uint32_t bpk,
                                      uint64_t max_file_bytes, uint8_t *file, uint64_t index_offset,
                                      uint64_t *handles, lv_sst_build_totals *totals,
                                      lv_sst_bloom_totals *bloom_totals) {
    Run R{payload, ops, order, n, block_size, restart_interval, bpk};
    R.max_file = max_file_bytes;
    lv_sst_build_totals t{};
    lv_sst_bloom_totals bt{};
    const uint64_t added = walk(R, Sink{file}, file ? index_offset : 0, file ? handles : nullptr, &t, &bt);
    t.entries = added;
    *totals = t;
    *bloom_totals = bt;
    return added;
}

extern "C" {

uint64_t lv_sst_build_file_bound(uint64_t payload_bytes, uint64_t op_cap, const lv_sst_build_options *opt) {
    (void)opt;  // the bound holds for every block_size and restart_interval (table.h)
    if (!op_cap) return 0;
    const unsigned __int128 b = static_cast<unsigned __int128>(payload_bytes) * 2 +
                                static_cast<unsigned __int128>(op_cap) * 75 + 70;
    return b > ~0ull ? ~0ull : static_cast<uint64_t>(b);
}

}  // extern "C"

namespace {

// lv_sst_build_host (bpk == 0, bloom_totals == NULL) and lv_sst_build_bloom_host.
int build_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops, const uint32_t *order,
               const lv_mt_totals *mt_totals, const lv_sst_build_options *opt, uint32_t bpk, uint8_t *file,
               uint64_t file_cap, uint64_t *handles, size_t block_cap, lv_sst_build_totals *totals,
               lv_sst_bloom_totals *bloom_totals) {
    uint64_t bs, ri;
    lv_sst_bloom_totals bt{}, unused{};
    if (bloom_totals) *bloom_totals = bt;
    if (!totals || !mt_totals || !options_ok(opt, &bs, &ri)) return LV_ERR_INVALID;
    if ((!payload && payload_bytes) || (!file && file_cap) || (!handles && block_cap)) return LV_ERR_INVALID;
    const bool sizing = !file && !file_cap;
    lv_sst_build_totals t{};
    uint64_t n = mt_totals->entries;
    if (mt_totals->status) {
        t.status = LV_SST_BUILD_NO_TABLE;
        n = 0;
    }
    if (n > kMaxOps || (n && (!ops || !order))) return LV_ERR_INVALID;
    for (uint64_t i = 0; i < n && !t.status; ++i) {  // not the memtable build's arguments: no table
        const lv_wb_op &o = ops[order[i]];
        if (!extent_ok(o.key_off, o.key_len, payload_bytes) || !extent_ok(o.val_off, o.val_len, payload_bytes))
            t.status = LV_SST_BUILD_NO_TABLE;
    }
    if (t.status) {
        *totals = t;
        return 0;
    }
    t.entries = n;
    const Run R{payload, ops, order, n, bs, ri, bpk};
    walk(R, Sink{nullptr}, 0, nullptr, &t, &bt);
    if (t.data_blocks > block_cap && !(sizing && !handles)) t.status |= LV_SST_BUILD_HANDLE_OVER;
    if (t.file_bytes > file_cap && !sizing) t.status |= LV_SST_BUILD_FILE_OVER;
    if (!t.status && file && n) {
        lv_sst_build_totals again{};
        walk(R, Sink{file}, t.index_offset, handles, &again, &unused);
    }
    *totals = t;
    if (bloom_totals && !t.status) *bloom_totals = bt;
    return 0;
}

}  // namespace

extern "C" {

int lv_sst_build_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops, const uint32_t *order,
                      const lv_mt_totals *mt_totals, const lv_sst_build_options *opt, uint8_t *file, uint64_t file_cap,
                      uint64_t *handles, size_t block_cap, lv_sst_build_totals *totals) {
    return build_host(payload, payload_bytes, ops, order, mt_totals, opt, 0, file, file_cap, handles, block_cap, totals,
                      nullptr);
}

int lv_sst_build_bloom_host(const uint8_t *payload, size_t payload_bytes, const lv_wb_op *ops, const uint32_t *order,
                            const lv_mt_totals *mt_totals, const lv_sst_build_options *opt,
                            const lv_sst_bloom_options *bloom, uint8_t *file, uint64_t file_cap, uint64_t *handles,
                            size_t block_cap, lv_sst_build_totals *totals, lv_sst_bloom_totals *bloom_totals) {
    if (!bloom || !bloom_totals || bloom->bits_per_key < 1 || bloom->bits_per_key > 64 || bloom->reserved)
        return LV_ERR_INVALID;
    return build_host(payload, payload_bytes, ops, order, mt_totals, opt, bloom->bits_per_key, file, file_cap, handles,
                      block_cap, totals, bloom_totals);
}

uint64_t lv_sst_build_bloom_file_bound(uint64_t payload_bytes, uint64_t op_cap, const lv_sst_build_options *opt,
                                       const lv_sst_bloom_options *bloom) {
    (void)opt;
    if (!op_cap || !bloom || bloom->bits_per_key < 1 || bloom->bits_per_key > 64 || bloom->reserved) return 0;
    const unsigned __int128 n = op_cap, p = payload_bytes;
    const unsigned __int128 b = p * 2 + n * 75 + 70 + n * bloom->bits_per_key / 8 + n * 9 + (p + n * 36) / 512 + 72;
    return b > ~0ull ? ~0ull : static_cast<uint64_t>(b);
}

size_t lv_bloom_filter_bytes(size_t n, uint32_t bits_per_key) {
    return bits_per_key ? static_cast<size_t>(bloom_bytes(n, bits_per_key) + 1) : 0;
}

int lv_bloom_create_filter(const uint8_t *keys, const uint64_t *off, const uint32_t *len, size_t n,
                           uint32_t bits_per_key, uint8_t *dst) {
    if (!dst || !bits_per_key || (n && (!off || !len))) return LV_ERR_INVALID;
    std::vector<uint32_t> hashes(n);
    for (size_t i = 0; i < n; ++i) {
        if (!keys && len[i]) return LV_ERR_INVALID;
        hashes[i] = lvr::hash(keys ? keys + off[i] : nullptr, len[i], lvr::kBloomSeed);
    }
    bloom_fill(dst, bloom_bytes(n, bits_per_key), bits_per_key, hashes.data(), n);
    return 0;
}

}  // extern "C"
