"""Bloom filter blocks in Python, written straight from the "Bloom filter
blocks" section of include/lvgpu/table.h: the hash, BloomFilterPolicy,
FilterBlockBuilder in its serial StartBlock / GenerateFilter form layered on
sst_build_cases' block model, a TableBuilder that writes the filter block and
the metaindex entry, and a model READER (ReadMeta, KeyMayMatch, the filtered
get); the case tables, the damaged images and the device helpers shared by
test_sst_bloom.py, test_gpu_sst_bloom_device.py and
test_gpu_sst_bloom_stress.py, and a `dump FILE` mode for
tools/sst_bloom_host_check.cc.

The filter count of the product comes from a closed form; the model's comes
from the serial form, so the closed form is what the comparison tests."""
import numpy as np

import memtable_cases as M
import sst_build_cases as S
import sst_get_cases as G
from memtable_cases import MAX_SEQUENCE, make_table, tag
from write_batch_cases import CANARY, GUARD, M64, tail_is_canary, varint

NAME = b"filter.leveldb.BuiltinBloomFilter2"
BASE_LG = 11
SEED = 0xBC9F1D34
BLOOM_TOTALS = ("filter_offset", "filter_size", "filters", "filter_keys")
BLOOM_FIELDS = ("filter_offset", "filter_size", "array_offset", "num", "base_lg", "present", "why", "reserved")
WHY_TABLE, WHY_EMPTY, WHY_BAD_METAINDEX, WHY_NO_ENTRY, WHY_BAD_HANDLE, WHY_BAD_TYPE, WHY_SHORT, WHY_BAD_ARRAY = range(1, 9)
FILTERED = 1
M32 = 0xFFFFFFFF


# ---- the hash and the filter policy ----
def leveldb_hash(data, seed):
    """util/hash.rs (upstream's Hash)."""
    m = 0xC6A4A793
    n = len(data)
    h = (seed ^ (m * n)) & M32
    i = 0
    while i + 4 <= n:
        h = (h + int.from_bytes(data[i:i + 4], "little")) & M32
        h = (h * m) & M32
        h ^= h >> 16
        i += 4
    rest = n - i
    if rest >= 3:
        h = (h + (data[i + 2] << 16)) & M32
    if rest >= 2:
        h = (h + (data[i + 1] << 8)) & M32
    if rest >= 1:
        h = (h + data[i]) & M32
        h = (h * m) & M32
        h ^= h >> 24
    return h


def bloom_hash(key):
    return leveldb_hash(bytes(key), SEED)


def bloom_k(bpk):
    return min(30, max(1, bpk * 69 // 100))


def probes(key, bits, k):
    h = bloom_hash(key)
    delta = ((h >> 17) | (h << 15)) & M32
    for _ in range(k):
        yield h % bits
        h = (h + delta) & M32


def create_filter(keys, bpk):
    bits = max(64, len(keys) * bpk)
    nbytes = (bits + 7) // 8
    bits = nbytes * 8
    f = bytearray(nbytes)
    k = bloom_k(bpk)
    for key in keys:
        for pos in probes(key, bits, k):
            f[pos // 8] |= 1 << (pos % 8)
    return bytes(f) + bytes([k])


def key_may_match(key, f):
    if len(f) < 2:
        return False
    k = f[-1]
    if k > 30:
        return True
    return all(f[pos // 8] & (1 << (pos % 8)) for pos in probes(key, (len(f) - 1) * 8, k))


# ---- the builders ----
class FilterBlockBuilder:
    def __init__(self, bpk):
        self.bpk = bpk
        self.keys = []
        self.result = bytearray()
        self.offsets = []
        self.added = 0

    def start_block(self, block_offset):
        index = block_offset // (1 << BASE_LG)
        while index > len(self.offsets):
            self.generate_filter()

    def add_key(self, key):
        self.keys.append(bytes(key))
        self.added += 1

    def generate_filter(self):
        self.offsets.append(len(self.result))
        if not self.keys:
            return
        self.result += create_filter(self.keys, self.bpk)
        self.keys = []

    def finish(self):
        if self.keys:
            self.generate_filter()
        array_offset = len(self.result)
        return (bytes(self.result) + b"".join(S.fixed32(o) for o in self.offsets) + S.fixed32(array_offset) +
                bytes([BASE_LG]))


class BloomTableBuilder(S.TableBuilder):
    def __init__(self, bpk, block_size=S.BLOCK_SIZE, restart_interval=S.RESTART_INTERVAL):
        super().__init__(block_size, restart_interval)
        self.filter = FilterBlockBuilder(bpk)
        self.filter.start_block(0)

    def add(self, key, value):
        # (TableBuilder::Add adds the key to the filter before the data block; the filter sees the user key)
        self.filter.add_key(S.user(key))
        super().add(key, value)

    def flush(self):
        super().flush()
        self.filter.start_block(len(self.file))

    def finish(self):
        if not self.data.empty():
            self.flush()
        filt = self.write_block(self.filter.finish())
        mb = S.BlockBuilder(self.restart_interval)
        mb.add(NAME, S.handle_encoding(*filt))
        meta = self.write_block(mb.finish())
        if self.pending is not None:
            self.index.add(S.short_successor(self.last_key), S.handle_encoding(*self.pending))
            self.pending = None
        index = self.write_block(self.index.finish())
        footer = S.handle_encoding(*meta) + S.handle_encoding(*index)
        self.file += footer + bytes(40 - len(footer)) + S.MAGIC.to_bytes(8, "little")
        return filt, meta, index


def model_build(payload, ops, bpk=10, block_size=S.BLOCK_SIZE, restart_interval=S.RESTART_INTERVAL, order=None):
    """(file, handles of data blocks + filter + metaindex + index, totals dict,
    bloom totals dict) of the flush with NewBloomFilterPolicy(bpk)."""
    ents = S.entries_of(payload, ops, order)
    if not ents:
        return b"", [], dict(zip(S.TOTALS, [0] * 8)), dict(zip(BLOOM_TOTALS, [0] * 4))
    tb = BloomTableBuilder(bpk, block_size, restart_interval)
    for k, v in ents:
        tb.add(k, v)
    filt, meta, index = tb.finish()
    tot = dict(entries=len(ents), data_blocks=len(tb.handles), file_bytes=len(tb.file), metaindex_offset=meta[0],
               metaindex_size=meta[1], index_offset=index[0], index_size=index[1], status=0)
    btot = dict(filter_offset=filt[0], filter_size=filt[1], filters=len(tb.filter.offsets), filter_keys=tb.filter.added)
    return bytes(tb.file), tb.handles + [filt, meta, index], tot, btot


# ---- the reader ----
def model_bloom_open(file, table, file_cap=None):
    """The lv_sst_bloom dict of ReadMeta / ReadFilter over the image and the
    table dict of the open."""
    b = dict.fromkeys(BLOOM_FIELDS, 0)

    def no(why):
        b["why"] = why
        return b
    fb = table["file_bytes"]
    if table["status"] or (file_cap is not None and fb > file_cap):
        return no(WHY_TABLE)
    if fb == 0:
        return no(WHY_EMPTY)
    mo, ms = table["metaindex_offset"], table["metaindex_size"]
    if not G.in_range(mo, ms, fb) or file[mo + ms] != 0:
        return no(WHY_BAD_METAINDEX)
    raw = file[mo:mo + ms]
    r = G.restarts(raw)
    if r is None:
        return no(WHY_BAD_METAINDEX)
    n, arr = r
    at, key, hit = 0, b"", None
    while n and at < arr:
        e = G.decode(raw, at, arr)
        if e is None or e[0] > len(key):
            return no(WHY_BAD_METAINDEX)
        shared, ns, vl, key_at = e
        key = key[:shared] + raw[key_at:key_at + ns]
        if key >= NAME:
            hit = (key, key_at + ns, vl)
            break
        at = key_at + ns + vl
    if hit is None or hit[0] != NAME:
        return no(WHY_NO_ENTRY)
    hd = G.handle_at(raw, hit[1], hit[1] + hit[2])
    if hd is None or not G.in_range(hd[0], hd[1], fb):
        return no(WHY_BAD_HANDLE)
    fo, fs = hd
    if file[fo + fs] != 0:
        return no(WHY_BAD_TYPE)
    if fs < 5:
        return no(WHY_SHORT)
    array = G.le32(file, fo + fs - 5)
    if array > fs - 5:
        return no(WHY_BAD_ARRAY)
    b.update(filter_offset=fo, filter_size=fs, array_offset=array, num=(fs - 5 - array) // 4, base_lg=file[fo + fs - 1],
             present=1)
    return b


def model_may_match(file, fb, b, block_offset, key):
    """FilterBlockReader::KeyMayMatch, with the bloom dict's offsets checked
    against the file again (a dict that does not fit means no filter)."""
    fo, fs, array = b["filter_offset"], b["filter_size"], b["array_offset"]
    if b["present"] != 1 or not G.in_range(fo, fs, fb) or fs < 5 or array > fs - 5 or b["num"] > (fs - 5 - array) // 4:
        return True
    data = file[fo:fo + fs]
    i = block_offset >> b["base_lg"] if b["base_lg"] < 64 else 0
    if i >= b["num"]:
        return True
    start, limit = G.le32(data, array + 4 * i), G.le32(data, array + 4 * i + 4)
    if start <= limit <= array:
        return key_may_match(key, data[start:limit])
    return start != limit


def model_get(file, table, bloom, key, seq, *, file_cap=None, bad_query=False):
    """The result dict of one filtered query: G.model_get's, but for a query
    whose data block the filter rules out, which is ABSENT with reserved = 1."""
    res = G.model_get(file, table, key, seq, file_cap=file_cap, bad_query=bad_query)
    if bloom["present"] != 1 or res["status"] in (G.NO_TABLE, G.BAD_SEQ, G.BAD_QUERY) or table["file_bytes"] == 0:
        return res
    # the index seek again, up to the handle: where the filter is asked
    fb = table["file_bytes"]
    io, isz = table["index_offset"], table["index_size"]
    if not G.in_range(io, isz, fb):
        return res
    idx = file[io:io + isz]
    r = G.restarts(idx)
    if r is None:
        return res
    n, arr = r
    target = (bytes(key), tag(seq, 1))
    try:
        lo, hi = 0, n
        while lo < hi:
            mid = lo + (hi - lo) // 2
            k, _ = G.probe(idx, arr, mid)
            if G.less(k, target):
                lo = mid + 1
            else:
                hi = mid
        if lo >= n:
            return res
        _, e = G.probe(idx, arr, lo)
    except G.Corrupt:
        return res
    hd = G.handle_at(idx, e[3] + e[1], e[3] + e[1] + e[2])
    if hd is None or not G.in_range(hd[0], hd[1], fb):
        return res
    if model_may_match(file, fb, bloom, hd[0], bytes(key)):
        return res
    out = dict.fromkeys(G.RESULT_FIELDS, 0)
    out["reserved"] = FILTERED
    return out


def queries_for(payload, ops, block_size, restart_interval):
    """G.queries_for around everything the table holds; the index keys are the
    plain image's (the data blocks and the index block do not depend on the
    filter policy)."""
    plain = S.model_build(payload, ops, block_size, restart_interval)[0]
    return G.queries_for(plain, payload, ops)


# ---- cases ----
def window_items(n, klen=6, vlen=3, start=0):
    return S.seq_items(n, klen, vlen, start)


def edge_items(data_end):
    """One entry whose single data block's trailer ends at data_end (>= 160):
    key "k", a value of data_end - 26 bytes (a two-byte varint)."""
    vlen = data_end - 26
    assert 128 <= vlen < 16384
    return [(b"k", tag(1), b"e" * vlen)]


def cases():
    """name -> (items, block_size, restart_interval, bits_per_key): the smallest
    shapes at which each mechanism can go wrong."""
    c = {}
    D = (S.BLOCK_SIZE, S.RESTART_INTERVAL)
    c["empty"] = ([], *D, 10)
    c["one_entry"] = ([(b"k", tag(1), b"v")], *D, 10)
    # n * bpk of 63, 64 and 65 bits; 63 / 64 / 65 keys in one window (a wave's lanes)
    for n in (63, 64, 65):
        c[f"bits_{n}"] = (window_items(n), *D, 1)
        c[f"wave_{n}"] = (window_items(n), *D, 10)
    for bpk in (1, 10, 64):
        c[f"bpk_{bpk}"] = (window_items(40), 256, 4, bpk)
    # the hash's tail and alignment: user keys of 0 .. 9 bytes
    c["key_lengths"] = ([(bytes(range(65, 65 + n)), tag(n + 1), b"v%d" % n) for n in range(10)], *D, 10)
    c["versions"] = ([(b"same", tag(s), b"v%d" % s) for s in range(1, 41)] + [(b"same", tag(7), b"v7")] * 3 +
                     [(b"dup", tag(42, 0), b"")] * 2, 128, 4, 10)
    # about eight blocks to a window
    c["block_256"] = (window_items(300, vlen=10), 256, 16, 10)
    # empty filters between used ones, blocks that straddle a window edge
    c["block_8192"] = (window_items(400, vlen=100), 8192, 16, 10)
    c["block_5000"] = (window_items(400, vlen=100), 5000, 16, 10)
    # the last block's trailer ends on a multiple of 2048 and a byte either side: both arms of F
    for end in (2047, 2048, 2049, 4095, 4096, 4097):
        c[f"data_end_{end}"] = (edge_items(end), *D, 10)
    c["big_value_then_small"] = ([(b"a", tag(1), b"B" * 9000), (b"b", tag(2), b"s"), (b"c", tag(3), b"t")], *D, 10)
    rng = np.random.default_rng(11)
    c["random_small_blocks"] = (M.random_items(rng, 300, alphabet=3, maxlen=12, seqs=6), 64, 4, 10)
    c["random_default"] = (M.random_items(rng, 500, alphabet=4, maxlen=30, seqs=50), *D, 7)
    c["corner_keys"] = (M.corner_items(), 256, 3, 10)
    return c


def large_items(n=60000):
    """One filter beyond the LDS budget: n entries with 8-byte keys and no
    value, to go under block_size 2^30 (one block, one window)."""
    return [(b"%08d" % i, tag(1), b"") for i in range(n)]


# ---- absent keys: the guard against a vacuous read test ----
ABSENT_SEED = 5


def absent_source():
    """(items, block_size, restart_interval, bpk, absent keys): a table of 600
    keys and 2,000 keys it does not hold, of which the model's filter rejects
    at least 90 % (about 99 % at 10 bits per key)."""
    rng = np.random.default_rng(ABSENT_SEED)
    keys = sorted({b"user%06d" % int(v) for v in rng.integers(0, 1000000, size=600)})
    items = [(k, tag(10 + i % 5), b"value%d" % (i % 9)) for i, k in enumerate(keys)]
    held = set(keys)
    absent = []
    while len(absent) < 2000:
        k = b"user%06d" % int(rng.integers(0, 1000000))
        if k not in held:
            absent.append(k)
    return items, 1024, 16, 10, absent


# ---- damaged images ----
def why_cases():
    """name -> (image, expected why): every reason there is no filter."""
    items, bs, ri, bpk = cases()["block_256"]
    payload, ops = make_table(items)
    image, handles, tot, btot = model_build(payload, ops, bpk, bs, ri)
    plain, _, _ = S.model_build(payload, ops, bs, ri)
    fo, fs = handles[-3]
    mo, ms = handles[-2]
    c = {}
    c["ok"] = (image, 0)
    c["empty_table"] = (b"", WHY_EMPTY)
    c["not_a_table"] = (image[:-1] + bytes([image[-1] ^ 1]), WHY_TABLE)
    c["no_filter_policy"] = (plain, WHY_NO_ENTRY)

    def with_meta(raw, typ=0):
        """The image with another metaindex block (same place; what follows moves)."""
        data = image[:mo]
        blocks = data + raw + bytes([typ]) + S.trailer(raw)[1:]
        io = len(blocks)
        idx = image[handles[-1][0]:handles[-1][0] + handles[-1][1]]
        blocks += idx + S.trailer(idx)
        foot = S.handle_encoding(mo, len(raw)) + S.handle_encoding(io, len(idx))
        return blocks + foot + bytes(40 - len(foot)) + S.MAGIC.to_bytes(8, "little")

    def meta_block(entries, interval=16):
        b = S.BlockBuilder(interval)
        for k, v in entries:
            b.add(k, v)
        return b.finish()
    good = S.handle_encoding(fo, fs)
    c["rebuilt_ok"] = (with_meta(meta_block([(NAME, good)])), 0)
    c["meta_type_1"] = (with_meta(meta_block([(NAME, good)]), typ=1), WHY_BAD_METAINDEX)
    c["meta_size_3"] = (with_meta(b"\x00\x00\x00"), WHY_BAD_METAINDEX)
    c["meta_restarts_0"] = (with_meta(S.fixed32(0)), WHY_NO_ENTRY)
    c["meta_entry_undecodable"] = (with_meta(b"\x00\x80\x80" + S.fixed32(0) + S.fixed32(1)), WHY_BAD_METAINDEX)
    c["meta_shared_beyond_key"] = (with_meta(G.raw_block([G.enc(0, b"a", b"x"), G.enc(5, b"zz", b"y")], 16)),
                                   WHY_BAD_METAINDEX)
    c["name_after_others"] = (with_meta(meta_block([(b"a.first", b"x"), (b"filter.leveldb.Builtin", b"y"), (NAME, good),
                                                    (b"zz", b"z")])), 0)
    c["name_prefix_only"] = (with_meta(meta_block([(NAME[:-1], good)])), WHY_NO_ENTRY)
    c["name_longer"] = (with_meta(meta_block([(NAME + b"x", good)])), WHY_NO_ENTRY)
    c["only_smaller_keys"] = (with_meta(meta_block([(b"a", good), (b"b", good)])), WHY_NO_ENTRY)
    c["handle_undecodable"] = (with_meta(meta_block([(NAME, b"\x80")])), WHY_BAD_HANDLE)
    c["handle_out_of_range"] = (with_meta(meta_block([(NAME, S.handle_encoding(len(image), 8))])), WHY_BAD_HANDLE)
    c["handle_wraps"] = (with_meta(meta_block([(NAME, S.handle_encoding(M64 - 2, 8))])), WHY_BAD_HANDLE)
    c["handle_trailing_bytes"] = (with_meta(meta_block([(NAME, good + b"junk")])), 0)
    c["filter_type_1"] = (image[:fo + fs] + b"\x01" + image[fo + fs + 1:], WHY_BAD_TYPE)
    # four bytes in front of a type byte 0: the type is checked before the size
    c["filter_short"] = (with_meta(meta_block([(NAME, S.handle_encoding(fo + fs - 4, 4))])), WHY_SHORT)
    c["filter_short_type"] = (with_meta(meta_block([(NAME, S.handle_encoding(fo, 4))])), WHY_BAD_TYPE)
    # the same bytes read as a filter block of another size: its array_offset is what lies at size - 5
    c["filter_bad_array"] = (image[:fo + fs - 5] + S.fixed32(fs - 4) + image[fo + fs - 1:], WHY_BAD_ARRAY)
    c["filter_array_at_limit"] = (image[:fo + fs - 5] + S.fixed32(fs - 5) + image[fo + fs - 1:], 0)  # num = 0
    c["filter_base_lg_64"] = (image[:fo + fs - 1] + b"\x40" + image[fo + fs:], 0)
    c["filter_base_lg_255"] = (image[:fo + fs - 1] + b"\xff" + image[fo + fs:], 0)
    c["filter_base_lg_0"] = (image[:fo + fs - 1] + b"\x00" + image[fo + fs:], 0)
    # offsets that decrease, equal offsets, a limit beyond the array
    arr = fo + btot["filter_size"] - 5 - 4 * btot["filters"]
    c["offsets_swapped"] = (image[:arr] + image[arr + 4:arr + 8] + image[arr:arr + 4] + image[arr + 8:], 0)
    c["offset_beyond_array"] = (image[:arr + 4] + S.fixed32(0xFFFFFF) + image[arr + 8:], 0)
    c["k_31"] = (image[:fo + G.le32(image, arr + 4) - 1] + b"\x1f" + image[fo + G.le32(image, arr + 4):], 0)
    return c, queries_for(payload, ops, bs, ri)


def flip_cases(count=300):
    """[(name, image)]: random flips inside the filter block, the metaindex
    block and the footer of block_256's image."""
    items, bs, ri, bpk = cases()["block_256"]
    payload, ops = make_table(items)
    image, handles, _, _ = model_build(payload, ops, bpk, bs, ri)
    fo, fs = handles[-3]
    mo, ms = handles[-2]
    rng = np.random.default_rng(91)
    spans = [(fo, fo + fs + 5), (mo, mo + ms + 5), (len(image) - 48, len(image))]
    out = []
    for i in range(count):
        lo, hi = spans[i % 3]
        out.append((f"flip/{i}", next(G.flips(image, rng, 1, lo, hi, multi=i % 2 == 1))))
    return out


def damaged_cases(flip_count=300):
    """[(name, image, queries)] of why_cases and flip_cases."""
    wc, queries = why_cases()
    queries = queries[::5]
    out = [("why/" + n, img, queries) for n, (img, _) in wc.items()]
    out += [(n, img, queries[i % 4::4]) for i, (n, img) in enumerate(flip_cases(flip_count))]
    return out


def model_answers(image, queries, file_cap=None):
    """(table dict, bloom dict, [result dict]) of the model for one image."""
    table = G.model_open(image, handles=False, file_cap=file_cap)[0]
    bloom = model_bloom_open(image, table, file_cap)
    return table, bloom, [model_get(image, table, bloom, k, s, file_cap=file_cap) for k, s in queries]


# ---- the host twins ----
def host_answers(image, queries):
    import lvgpu.table as T
    table, _ = T.open_host(image, handles=False)
    bloom = T.bloom_open_host(image, table)
    return table, bloom, [T.get_bloom_host(image, table, bloom, k, s) for k, s in queries]


# ---- one device call ----
def run_device(torch, dev, payload, ops, bpk=10, block_size=S.BLOCK_SIZE, restart_interval=S.RESTART_INTERVAL, *, shift=0,
               file_cap=None, block_cap=None, mt_status=0, op_cap=None, stream=None, want=None):
    """lv_memtable_build_device, then lv_sst_build_bloom_device over its
    outputs on a guarded payload, with canary-filled outputs and a dirty
    workspace.  Returns the lvgpu.table.BuiltBloom."""
    import lvgpu.table as T
    table, buf = M.run_build(torch, dev, payload, ops, shift=shift, op_cap=op_cap, stream=stream)
    if mt_status:
        table.totals[2] = mt_status
    want = want or model_build(payload, ops, bpk, block_size or S.BLOCK_SIZE, restart_interval or S.RESTART_INTERVAL)
    fc = len(want[0]) if file_cap is None else file_cap
    bc = max(len(want[1]) - 3, 0) if block_cap is None else block_cap
    ws = torch.full((max(T.build_bloom_workspace_bytes(table.op_cap, bc), 16),), 0x5A, dtype=torch.uint8, device=dev)
    built = T.build_bloom_device(table, bpk, block_size=block_size, restart_interval=restart_interval, file_cap=fc,
                                 block_cap=bc, workspace=ws, stream=stream, fill=CANARY, guard=GUARD)
    built._buf = buf
    return built


def compare_device(built, want, tag_=""):
    """The image, the handles and both totals of a call whose status is 0
    against the model's (file, handles, totals, bloom totals), and the canaries
    behind both outputs."""
    want_file, want_handles, want_tot, want_btot = want
    t = built.sync_totals()
    assert t == want_tot, (tag_, t, want_tot)
    bt = built.sync_bloom_totals()
    assert bt == want_btot, (tag_, bt, want_btot)
    got = built.file()
    if got != want_file:
        at = next(i for i, (a, b) in enumerate(zip(got, want_file)) if a != b)
        raise AssertionError((tag_, "file differs at", at, got[at:at + 16].hex(), want_file[at:at + 16].hex(), want_handles[-3:]))
    assert built.handles() == want_handles, (tag_, built.handles()[-4:], want_handles[-4:])
    assert tail_is_canary(built.file_t, len(want_file)), (tag_, "d_file written at or beyond file_bytes")
    assert tail_is_canary(built.handles_t, 16 * len(want_handles)), (tag_, "d_handles written beyond its count")


def check_device(torch, dev, items, block_size=S.BLOCK_SIZE, restart_interval=S.RESTART_INTERVAL, bpk=10, *, shift=0,
                 gaps=None, tag_="", **kw):
    payload, ops = make_table(items, gaps)
    want = model_build(payload, ops, bpk, block_size, restart_interval)
    built = run_device(torch, dev, payload, ops, bpk, block_size, restart_interval, shift=shift, want=want, **kw)
    compare_device(built, want, tag_)
    return built, payload, ops, want


def open_both(torch, dev, image, *, shift=0, file_cap=None):
    """lv_sst_open_device (no handles) and lv_sst_bloom_open_device over the
    image in a guarded tensor: (Opened, bloom tensor, owner)."""
    import lvgpu.table as T
    owner, file_t = G.place(torch, dev, image, shift)
    op = G.run_open(torch, dev, file_t, len(image), handles=False, file_cap=file_cap)
    return op, T.bloom_open_device(op), owner


def run_get(torch, dev, opened, bloom_t, qk, off, ln, sq, stream=None):
    """lv_sst_get_bloom_device with canaries behind the results."""
    import lvgpu.table as T
    nq = len(off)
    g = T.get_bloom_device(opened, bloom_t, *G.dev_queries(torch, dev, qk, off, ln, sq), nq=nq, stream=stream,
                           fill=CANARY, guard=GUARD)
    out = g.sync()
    assert tail_is_canary(g.res, nq * 32), "d_results written past nq"
    return out


def result_dicts(arr):
    return [{k: int(r[k]) for k in G.RESULT_FIELDS} for r in arr]


# ---- the file tools/sst_bloom_host_check.cc replays ----
def dump(path):
    """The damaged cases with the model's expected outputs (little-endian u64
    fields; see the program's replay())."""
    u64 = lambda v: int(v).to_bytes(8, "little")
    cases_ = damaged_cases()
    out = bytearray(u64(len(cases_)))
    for _, image, queries in cases_:
        table, bloom, results = model_answers(image, queries)
        out += u64(len(image)) + image + b"".join(u64(bloom[f]) for f in BLOOM_FIELDS) + u64(len(queries))
        for (key, seq), r in zip(queries, results):
            out += u64(len(key)) + key + u64(seq) + np.array([tuple(r[f] for f in G.RESULT_FIELDS)], dtype=G_DTYPE).tobytes()
    with open(path, "wb") as f:
        f.write(out)
    return len(cases_)


G_DTYPE = np.dtype([("val_off", "<u8"), ("tag", "<u8"), ("val_len", "<u4"), ("block", "<u4"), ("status", "<u4"),
                    ("reserved", "<u4")])


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "leveldb-rs_amd"))
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        print("wrote", dump(sys.argv[2]), "cases")
    else:
        raise SystemExit("usage: python tests/sst_bloom_cases.py dump FILE")
