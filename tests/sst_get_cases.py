"""The SSTable reader in Python, written straight from the "Open" and "Get"
sections of include/lvgpu/table.h over bytes: the open's checks, the serial
get with its exact probe order and corruption rules (keys materialised, unlike
the product), the query generator, builders of damaged images and the device
helpers shared by test_sst_get.py, test_gpu_sst_get_device.py and
test_gpu_sst_get_stress.py.

model_open / model_get are the model every output of lv_sst_open_* and
lv_sst_get_* is compared with.  On well-formed images sst_build_cases.index_seek
is the independent cross-check: the two must agree there."""
import numpy as np

import memtable_cases as M
import sst_build_cases as S
from memtable_cases import MAX_SEQUENCE, make_table, tag
from write_batch_cases import CANARY, GUARD, M64, guarded_payload, tail_is_canary, varint

UPSTREAM, NOT_A_TABLE, BAD_FOOTER, BAD_INDEX, INDEX_SHAPE, HANDLE_OVER = 1, 2, 4, 8, 16, 32
ABSENT, FOUND, DELETED, BAD_SEQ, NO_TABLE, BAD_QUERY, CORRUPT = range(7)
TABLE_FIELDS = ("file_bytes", "metaindex_offset", "metaindex_size", "index_offset", "index_size", "data_blocks",
                "reserved", "status")
RESULT_FIELDS = ("val_off", "tag", "val_len", "block", "status", "reserved")
HANDLE_CANARY = 0xA5A5A5A5A5A5A5A5


# ---- the decoders ----
def varint64(b, at, limit):
    """decode_varint_64_limit: (value, next) or None; at most 10 bytes."""
    r, shift = 0, 0
    while shift <= 63 and at < limit:
        c = b[at]
        at += 1
        r |= ((c & 0x7F) << shift) & M64
        if not c & 0x80:
            return r, at
        shift += 7
    return None


def varint32(b, at, limit):
    """GetVarint32Ptr: (value, next) or None; at most 5 bytes."""
    r, shift = 0, 0
    while shift <= 28 and at < limit:
        c = b[at]
        at += 1
        r |= ((c & 0x7F) << shift) & 0xFFFFFFFF
        if not c & 0x80:
            return r, at
        shift += 7
    return None


def handle_at(b, at, limit):
    o = varint64(b, at, limit)
    if o is None:
        return None
    s = varint64(b, o[1], limit)
    if s is None:
        return None
    return o[0], s[0]


def in_range(off, size, fb):
    return size < 0xFFFFFFFF and off + size + 5 <= fb


def decode(raw, p, limit):
    """(shared, non_shared, value_len, key_at) or None."""
    if p > limit or limit - p < 3:
        return None
    out = []
    for _ in range(3):
        v = varint32(raw, p, limit)
        if v is None:
            return None
        out.append(v[0])
        p = v[1]
    if limit - p < out[1] + out[2]:
        return None
    return out[0], out[1], out[2], p


def le32(b, at):
    return int.from_bytes(b[at:at + 4], "little")


def restarts(raw):
    """(n, arr) or None."""
    if len(raw) < 4:
        return None
    n = le32(raw, len(raw) - 4)
    if n > (len(raw) - 4) // 4:
        return None
    return n, len(raw) - 4 - 4 * n


def less(key, target):
    """InternalKeyComparator: internal key bytes against (user key, tag)."""
    uk, t = target
    if key[:-8] != uk:
        return key[:-8] < uk
    return int.from_bytes(key[-8:], "little") > t


# ---- Table::Open ----
def model_open(file, *, block_cap=None, handles=True, file_cap=None, upstream=0):
    """(table dict, handles [(offset, size)] or None when none are written)."""
    t = dict.fromkeys(TABLE_FIELDS, 0)
    if upstream:
        t["status"] = UPSTREAM
        return t, None
    fb = len(file)
    if fb == 0:
        return t, []
    t["file_bytes"] = fb
    if fb < 48 or (file_cap is not None and fb > file_cap) or int.from_bytes(file[-8:], "little") != S.MAGIC:
        t["status"] = NOT_A_TABLE
        return t, None
    foot, at, h = file[-48:], 0, []
    for _ in range(4):
        v = varint64(foot, at, 48)
        if v is None:
            t["status"] = BAD_FOOTER
            return t, None
        h.append(v[0])
        at = v[1]
    if not in_range(h[0], h[1], fb) or not in_range(h[2], h[3], fb):
        t["status"] = BAD_FOOTER
        return t, None
    t["metaindex_offset"], t["metaindex_size"], t["index_offset"], t["index_size"] = h
    idx = file[h[2]:h[2] + h[3]]
    r = restarts(idx)
    if file[h[2] + h[3]] != 0 or r is None or r[0] < 1:
        t["status"] = BAD_INDEX
        return t, None
    n, arr = r
    t["data_blocks"] = n
    out, status = [], 0
    for i in range(n):
        at = le32(idx, arr + 4 * i)
        end = le32(idx, arr + 4 * (i + 1)) if i + 1 < n else arr
        if end > arr or at >= end:
            status |= BAD_INDEX
            continue
        klen, count, bad = 0, 0, False
        while at < end:
            e = decode(idx, at, end)
            if e is None or e[0] > klen:
                bad = True
                break
            shared, ns, vl, key_at = e
            klen = shared + ns
            hd = handle_at(idx, key_at + ns, key_at + ns + vl)
            if klen < 8 or hd is None or not in_range(hd[0], hd[1], fb):
                bad = True
                break
            if count == 0:
                out.append(hd)
            count += 1
            at = key_at + ns + vl
        if bad:
            status |= BAD_INDEX
        elif count > 1:
            status |= INDEX_SHAPE
    if handles and n > (n if block_cap is None else block_cap):
        status |= HANDLE_OVER
    t["status"] = status
    if status:
        return t, None
    return t, out + [(h[0], h[1]), (h[2], h[3])]


# ---- Table::InternalGet + SaveValue ----
class Corrupt(Exception):
    pass


def probe(raw, arr, i):
    """The contiguous key of the entry at restart i, and the entry."""
    e = decode(raw, le32(raw, arr + 4 * i), arr)
    if e is None or e[0] != 0 or e[1] < 8:
        raise Corrupt
    return raw[e[3]:e[3] + e[1]], e


def block_seek(raw, target):
    """(key, value offset in raw, value length) of the first entry not less
    than target, or None; Corrupt."""
    r = restarts(raw)
    if r is None:
        raise Corrupt
    n, arr = r
    if n == 0:
        return None
    left, right = 0, n - 1
    while left < right:
        mid = (left + right + 1) // 2
        key, _ = probe(raw, arr, mid)
        if less(key, target):
            left = mid
        else:
            right = mid - 1
    at, key = le32(raw, arr + 4 * left), b""
    while True:
        if at >= arr:
            return None
        e = decode(raw, at, arr)
        if e is None or e[0] > len(key) or e[0] + e[1] < 8:
            raise Corrupt
        shared, ns, vl, key_at = e
        key = key[:shared] + raw[key_at:key_at + ns]
        if not less(key, target):
            return key, key_at + ns, vl
        at = key_at + ns + vl


def model_get(file, table, key, seq, *, file_cap=None, bad_query=False):
    """The result dict of one query over the image and the table dict."""
    res = dict.fromkeys(RESULT_FIELDS, 0)

    def done(status):
        res["status"] = status
        return res
    fb = table["file_bytes"]
    if table["status"] or (file_cap is not None and fb > file_cap):
        return done(NO_TABLE)
    if seq > MAX_SEQUENCE:
        return done(BAD_SEQ)
    if bad_query:
        return done(BAD_QUERY)
    if fb == 0:
        return done(ABSENT)
    target = (bytes(key), tag(seq, 1))
    io, isz = table["index_offset"], table["index_size"]
    if not in_range(io, isz, fb):
        return done(CORRUPT)
    idx = file[io:io + isz]
    r = restarts(idx)
    if r is None:
        return done(CORRUPT)
    n, arr = r
    try:
        lo, hi = 0, n
        while lo < hi:
            mid = lo + (hi - lo) // 2
            k, _ = probe(idx, arr, mid)
            if less(k, target):
                lo = mid + 1
            else:
                hi = mid
        if lo >= n:
            return done(ABSENT)
        _, e = probe(idx, arr, lo)
        hd = handle_at(idx, e[3] + e[1], e[3] + e[1] + e[2])
        if hd is None or not in_range(hd[0], hd[1], fb) or file[hd[0] + hd[1]] != 0:
            return done(CORRUPT)
        hit = block_seek(file[hd[0]:hd[0] + hd[1]], target)
    except Corrupt:
        return done(CORRUPT)
    if hit is None or hit[0][:-8] != target[0]:
        return done(ABSENT)
    k, vat, vl = hit
    if k[-8] > 1:
        return done(CORRUPT)
    res["tag"], res["block"] = int.from_bytes(k[-8:], "little"), lo
    if k[-8] == 0:
        return done(DELETED)
    res["val_off"], res["val_len"] = hd[0] + vat, vl
    return done(FOUND)


# ---- queries ----
def bump(key, d):
    return key[:-1] + bytes([(key[-1] + d) & 0xFF])


def queries_for(file, payload, ops):
    """[(key, seq)] around everything the table holds (see the issue's list):
    every version at snapshots around its own, 0 and the maximum; every key
    with its last byte +-1, cut by a byte, extended by a zero; the user key of
    every index entry; the empty key; 0xff runs; keys beyond both ends; one
    snapshot above the maximum."""
    qs = []
    for o in ops:
        key, seq = M.key_of(payload, o), int(o["tag"]) >> 8
        for s in (seq - 1, seq, seq + 1, 0, MAX_SEQUENCE):
            if 0 <= s <= MAX_SEQUENCE:
                qs.append((key, s))
    keys = sorted({M.key_of(payload, o) for o in ops})
    for k in keys:
        if k:
            qs += [(bump(k, 1), MAX_SEQUENCE), (bump(k, -1), MAX_SEQUENCE), (k[:-1], MAX_SEQUENCE)]
        qs.append((k + b"\x00", MAX_SEQUENCE))
    if file:
        for ik, _ in S.read_table(file)[1]:
            qs += [(ik[:-8], MAX_SEQUENCE), (ik[:-8], 0)]
    qs.append((b"", MAX_SEQUENCE))
    qs += [(b"\xff" * i, MAX_SEQUENCE) for i in range(1, 5)]
    if keys:
        qs += [(keys[-1] + b"\x01", MAX_SEQUENCE), (keys[0][:-1] if keys[0] else b"", 5)]
    qs.append((keys[0] if keys else b"k", MAX_SEQUENCE + 1))  # BAD_SEQ
    return qs


def pack_queries(queries, bad_query=True):
    """M.pack_queries with gaps, plus (bad_query) one more query whose extent
    ends one byte beyond qkeys: (qkeys, q_off, q_len, q_seq, flags of BAD_QUERY)."""
    qk, off, ln, sq = M.pack_queries(queries, gaps=[i % 5 for i in range(len(queries))])
    bad = [False] * len(queries)
    if bad_query:
        off = np.append(off, np.uint64(max(len(qk) - 1, 0)))
        ln = np.append(ln, np.uint32(3))
        sq = np.append(sq, np.uint64(1))
        bad.append(True)
    return qk, off, ln, sq, bad


# ---- assembling images by hand ----
def parts_of(image):
    """(data block raws, index [(key, (offset, size))]) of a well-formed image."""
    _, index, _ = S.read_table(image)
    return [image[o:o + s] for _, (o, s) in index], index


def index_block(entries, interval=1):
    """BlockBuilder over [(key, value bytes)]."""
    b = S.BlockBuilder(interval)
    for k, v in entries:
        b.add(k, v)
    return b.finish()


def assemble(blocks, keys, *, index=None, interval=1, types=None):
    """An image of the given data block raws with one index entry (keys[i], the
    handle of block i) each, or with `index` as the index block's raw bytes:
    (file, handles)."""
    f, hs = bytearray(), []

    def put(raw, typ=0):
        hs.append((len(f), len(raw)))
        f.extend(raw + bytes([typ]) + S.trailer(raw)[1:])
    for i, raw in enumerate(blocks):
        put(raw, types[i] if types else 0)
    put(S.BlockBuilder(16).finish())
    if index is None:
        index = index_block([(k, S.handle_encoding(*hs[i])) for i, k in enumerate(keys)], interval)
    put(index)
    foot = S.handle_encoding(*hs[-2]) + S.handle_encoding(*hs[-1])
    f.extend(foot + bytes(40 - len(foot)) + S.MAGIC.to_bytes(8, "little"))
    return bytes(f), hs


def with_index(image, raw):
    blocks, index = parts_of(image)
    return assemble(blocks, [k for k, _ in index], index=raw)[0]


def with_footer(image, foot40):
    return image[:-48] + foot40 + bytes(40 - len(foot40)) + image[-8:]


def enc(shared, suffix, value, *, sv=None, nv=None, vv=None):
    """One block entry; sv / nv / vv replace a varint's bytes."""
    return ((varint(shared) if sv is None else sv) + (varint(len(suffix)) if nv is None else nv) +
            (varint(len(value)) if vv is None else vv) + suffix + value)


def raw_block(parts, interval, *, restarts_=None, count=None):
    """A block of encoded entries with a restart at every interval-th one (or
    the given restart offsets / restart count)."""
    buf, rs = bytearray(), []
    for i, p in enumerate(parts):
        if i % interval == 0:
            rs.append(len(buf))
        buf += p
    rs = rs if restarts_ is None else restarts_(rs, len(buf))
    return bytes(buf) + b"".join(S.fixed32(r) for r in rs) + S.fixed32(len(rs) if count is None else count)


BASE_ITEMS = S.seq_items(40, klen=4, vlen=2)  # with (64, 4): several blocks of several restarts
BASE_OPT = (64, 4)


def base_image():
    payload, ops = make_table(BASE_ITEMS)
    image, handles, _ = S.model_build(payload, ops, *BASE_OPT)
    return payload, ops, image, handles


def open_cases():
    """name -> (image, model_open keywords, expected status): every open status."""
    _, _, image, handles = base_image()
    blocks, index = parts_of(image)
    n, fb = len(index), len(image)
    ents = [(k, S.handle_encoding(o, s)) for k, (o, s) in index]
    good = index_block(ents)
    arr = len(good) - 4 - 4 * n
    r1 = le32(good, arr + 4)
    c = {}
    c["ok"] = (image, {}, 0)
    c["ok_no_handles"] = (image, dict(handles=False), 0)
    c["empty_file"] = (b"", {}, 0)
    c["bytes_47"] = (image[-47:], {}, NOT_A_TABLE)
    c["wrong_magic"] = (image[:-1] + bytes([image[-1] ^ 1]), {}, NOT_A_TABLE)
    c["footer_handle_out_of_range"] = (with_footer(image, S.handle_encoding(*handles[-2]) +
                                                   S.handle_encoding(handles[-1][0], handles[-1][1] + 49)), {}, BAD_FOOTER)
    c["footer_size_large"] = (with_footer(image, S.handle_encoding(*handles[-2]) +
                                          S.handle_encoding(0, 0xFFFFFFFF)), {}, BAD_FOOTER)
    c["footer_offset_wraps"] = (with_footer(image, S.handle_encoding(*handles[-2]) +
                                            S.handle_encoding(M64 - 2, 8)), {}, BAD_FOOTER)
    c["footer_varint_truncated"] = (with_footer(image, S.handle_encoding(*handles[-2]) + b"\x80" * 30), {}, BAD_FOOTER)
    io, isz = handles[-1]
    c["index_type_1"] = (image[:io + isz] + b"\x01" + image[io + isz + 1:], {}, BAD_INDEX)
    c["index_n_0"] = (with_index(image, good[:arr] + S.fixed32(0)), {}, BAD_INDEX)
    c["index_n_large"] = (with_index(image, good[:-4] + S.fixed32(n + 1 + arr // 4)), {}, BAD_INDEX)
    c["index_size_3"] = (with_index(image, b"\x00\x00\x00"), {}, BAD_INDEX)
    c["index_entry_overruns_restart"] = (with_index(image, good[:arr + 4] + S.fixed32(r1 - 1) + good[arr + 8:]), {},
                                         BAD_INDEX)
    c["index_restart_beyond_arr"] = (with_index(image, good[:-8] + S.fixed32(arr + 1) + good[-4:]), {}, BAD_INDEX)
    c["index_empty_run"] = (with_index(image, good[:arr + 4] + S.fixed32(0) + good[arr + 8:]), {},
                            BAD_INDEX | INDEX_SHAPE)  # run 0 is empty, run 1 holds two entries
    c["index_shared_1"] = (with_index(image, good[:r1] + b"\x01" + good[r1 + 1:]), {}, BAD_INDEX)
    short = [(k[:7] if i == 1 else k, v) for i, (k, v) in enumerate(ents)]
    c["index_key_7"] = (with_index(image, index_block(short)), {}, BAD_INDEX)
    c["index_handle_undecodable"] = (with_index(image, index_block(ents[:2] + [(ents[2][0], b"\x80")] + ents[3:])), {},
                                     BAD_INDEX)
    c["index_handle_out_of_range"] = (with_index(image, index_block(ents[:-1] + [(ents[-1][0], S.handle_encoding(fb, 10))])),
                                      {}, BAD_INDEX)
    c["index_handle_trailing_bytes"] = (with_index(image, index_block([(k, v + b"junk") for k, v in ents])), {}, 0)
    c["index_interval_2"] = (with_index(image, index_block(ents, 2)), {}, INDEX_SHAPE)
    c["index_interval_2_and_bad"] = (with_index(image, index_block(short, 2)), {}, BAD_INDEX | INDEX_SHAPE)
    c["handle_over"] = (image, dict(block_cap=n - 1), HANDLE_OVER)
    c["handle_over_and_shape"] = (with_index(image, index_block(ents, 2)), dict(block_cap=0), INDEX_SHAPE | HANDLE_OVER)
    return c


# a hand-made data block: 12 keys, restart interval 4
HAND_KEYS = [b"key%02d" % i for i in range(12)]


def hand_parts(patch=None):
    """The encoded entries of the hand-made block; patch[i] = keywords of enc
    (or a whole replacement entry as bytes) for entry i."""
    parts, last, patch = [], b"", dict(patch or {})
    for i, k in enumerate(HAND_KEYS):
        ik = S.ikey(k, tag(50 + i))
        shared = 0 if i % 4 == 0 else S.common_prefix(last, ik)
        p = patch.get(i, {})
        parts.append(p if isinstance(p, bytes) else enc(p.pop("shared", shared), p.pop("suffix", ik[shared:]),
                                                         p.pop("value", b"val%d" % i), **p))
        last = ik
    return parts


def get_corruption_cases():
    """name -> (image, queries, whether some query must be CORRUPT): a table of
    three blocks whose middle one is the hand-made block, damaged."""
    lo_items = [(b"a%02d" % i, tag(10 + i), b"lo") for i in range(5)]
    hi_items = [(b"z%02d" % i, tag(10 + i), b"hi") for i in range(5)]

    def side(items):
        b = S.BlockBuilder(2)
        for k, t, v in items:
            b.add(S.ikey(k, t), v)
        return b.finish()
    keys = [S.ikey(b"a99", tag(1)), S.ikey(b"key99", tag(1)), S.ikey(b"z99", tag(1))]
    queries = [(k, s) for k in HAND_KEYS + [b"key", b"key055", b"a02", b"z04", b"zzz"] for s in (0, 49, 55, 61, MAX_SEQUENCE)]

    def table(mid, **kw):
        return assemble([side(lo_items), mid, side(hi_items)], keys, **kw)[0]
    c = {}
    good = raw_block(hand_parts(), 4)
    c["good"] = (table(good), False)
    c["type_byte_1"] = (table(good, types=[0, 1, 0]), True)
    c["n_0"] = (table(raw_block(hand_parts(), 4, count=0, restarts_=lambda rs, end: [])), False)
    c["n_large"] = (table(raw_block(hand_parts(), 4, count=1 << 30)), True)
    c["size_3"] = (table(b"\x01\x00\x00"), True)
    c["restart_at_arr"] = (table(raw_block(hand_parts(), 4, restarts_=lambda rs, end: [rs[0], end, rs[2]])), True)
    c["restart_beyond_arr"] = (table(raw_block(hand_parts(), 4, restarts_=lambda rs, end: [rs[0], rs[1], end + 9])), True)
    # restart 0 is never probed: a scan from it finds no entry
    c["restart_huge"] = (table(raw_block(hand_parts(), 4, restarts_=lambda rs, end: [0xFFFFFFFF, rs[1], rs[2]])), False)
    c["shared_on_probed_restart"] = (table(raw_block(hand_parts({4: dict(shared=1)}), 4)), True)
    c["shared_beyond_previous_key"] = (table(raw_block(hand_parts({5: dict(shared=100)}), 4)), True)
    c["value_len_overruns"] = (table(raw_block(hand_parts({11: dict(vv=b"\x7f")}), 4)), True)
    c["non_shared_overruns"] = (table(raw_block(hand_parts({9: dict(nv=b"\xff\xff\xff\xff\x0f")}), 4)), True)
    c["varint_5_bytes_high_bits"] = (table(raw_block(hand_parts({4: dict(sv=b"\x80\x80\x80\x80\x70")}), 4)), False)
    c["varint_6_bytes"] = (table(raw_block(hand_parts({4: dict(sv=b"\x80\x80\x80\x80\x80\x00")}), 4)), True)
    c["varint_runs_into_limit"] = (table(raw_block(hand_parts({11: b"\x00\x80\x80"}), 4)), True)
    c["key_shorter_than_8"] = (table(raw_block(hand_parts({8: dict(suffix=b"key08\x01\x00")}), 4)), True)
    c["scanned_key_shorter_than_8"] = (table(raw_block(hand_parts({1: dict(shared=2, suffix=b"x")}), 4)), True)
    type_2 = dict(suffix=b"6" + tag(56, 2).to_bytes(8, "little"))
    c["entry_type_2"] = (table(raw_block(hand_parts({6: type_2}), 4)), True)
    # an index entry whose handle points at a block that is in range but is no block
    bad_handle = index_block([(keys[0], S.handle_encoding(0, 7)), (keys[1], S.handle_encoding(1 << 40, 8)),
                              (keys[2], b"\x80\x80")])
    c["index_handles"] = (table(good, index=bad_handle), True)
    return {k: (img, queries, must) for k, (img, must) in c.items()}


def flips(image, rng, count, lo=0, hi=None, multi=False):
    """`count` images with one random byte (multi: one to four) of image[lo, hi)
    replaced."""
    hi = len(image) if hi is None else hi
    for _ in range(count):
        b = bytearray(image)
        for _ in range(int(rng.integers(1, 5)) if multi else 1):
            b[int(rng.integers(lo, hi))] = int(rng.integers(0, 256))
        yield bytes(b)


# ---- the device ----
def place(torch, dev, image, shift=0):
    """The image in a canary-filled tensor at `shift` bytes past a 16-B
    boundary: (owner, the image's slice)."""
    return guarded_payload(torch, dev, image, shift)


def run_open(torch, dev, file_t, nbytes, *, upstream=None, block_cap=None, handles=True, file_cap=None, stream=None):
    """lv_sst_open_device with a canary-filled handle array: the Opened."""
    import lvgpu.table as T
    d_fb = M.dev_i64(torch, dev, [nbytes])
    d_up = None if upstream is None else M.dev_i64(torch, dev, [upstream])
    return T.open_device(file_t, d_fb, d_up, file_cap=file_cap, block_cap=block_cap or 0, handles=handles,
                         stream=stream, fill=CANARY, guard=GUARD)


def check_open(torch, dev, image, *, shift=0, tag_="", upstream=None, file_cap=None, **kw):
    """The table and the handles of one device open against the model, and the
    canaries of d_handles: (Opened, owner, model table)."""
    want_t, want_h = model_open(image, upstream=upstream or 0, file_cap=file_cap, **kw)
    bc = kw.get("block_cap")
    if not kw.get("handles", True):
        bc = 0  # a NULL d_handles goes with block_cap 0
    elif bc is None:
        bc = model_open(image)[0]["data_blocks"]
    owner, file_t = place(torch, dev, image, shift)
    op = run_open(torch, dev, file_t, len(image), upstream=upstream, block_cap=bc, handles=kw.get("handles", True),
                  file_cap=file_cap)
    got = op.sync(check=False)
    assert got == want_t, (tag_, got, want_t)
    if op.handles_t is not None:
        if want_h is None:
            assert tail_is_canary(op.handles_t, 0), (tag_, "d_handles written on a status")
        else:
            assert op.handles() == want_h, (tag_, op.handles()[:4], want_h[:4])
            assert tail_is_canary(op.handles_t, 16 * len(want_h)), (tag_, "d_handles written beyond its count")
    return op, owner, want_t


def dev_queries(torch, dev, qk, off, ln, sq):
    d_qk = M.dev_bytes(torch, dev, qk)[: len(qk)] if len(qk) else torch.zeros(0, dtype=torch.uint8, device=dev)
    l32 = np.ascontiguousarray(ln, dtype=np.uint32)
    d_len = (torch.from_numpy(l32.view(np.int32).copy()).to(dev) if l32.size
             else torch.zeros(1, dtype=torch.int32, device=dev))
    return d_qk, M.dev_i64(torch, dev, off), d_len, M.dev_i64(torch, dev, sq)


def run_get(torch, dev, opened, qk, off, ln, sq, stream=None):
    """lv_sst_get_device with canaries behind the results: a structured array."""
    import lvgpu.table as T
    nq = len(off)
    g = T.get_device(opened, *dev_queries(torch, dev, qk, off, ln, sq), nq=nq, stream=stream, fill=CANARY, guard=GUARD)
    out = g.sync()
    assert tail_is_canary(g.res, nq * 32), "d_results written past nq"
    return out


def model_results(image, table, queries, bad, file_cap=None):
    """The model's result dicts for packed queries (bad: pack_queries' flags)."""
    qs = list(queries) + [(b"", 1)] * (len(bad) - len(queries))
    return [model_get(image, table, k, s, bad_query=b, file_cap=file_cap) for (k, s), b in zip(qs, bad)]


def compare_results(got, wants, tag_=""):
    """Device results against the model's, query by query; the statuses seen."""
    assert len(got) == len(wants)
    for i, want in enumerate(wants):
        g = {k: int(got[i][k]) for k in RESULT_FIELDS}
        assert g == want, (tag_, i, g, want)
    return {w["status"] for w in wants}


class Packed:
    """Queries packed once, with the model's answers for one image and table."""

    def __init__(self, image, table, queries, file_cap=None):
        self.arrays = pack_queries(queries)
        self.wants = model_results(image, table, queries, self.arrays[4], file_cap)

    def check(self, torch, dev, opened, tag_="", stream=None):
        return compare_results(run_get(torch, dev, opened, *self.arrays[:4], stream=stream), self.wants, tag_)


def check_image(torch, dev, image, queries, *, shifts=(0,), tag_="", **kw):
    """Open and get of one image on the device against the model, the image at
    each of `shifts`: the statuses seen."""
    packed = Packed(image, model_open(image, **kw)[0], queries)
    seen = set()
    for shift in shifts:
        op, owner, _ = check_open(torch, dev, image, shift=shift, tag_=f"{tag_} shift {shift}", **kw)
        seen |= packed.check(torch, dev, op, f"{tag_} shift {shift}")
        host = owner.cpu().numpy()
        base = (-owner.data_ptr()) % 16 + shift + GUARD
        assert host[base:base + len(image)].tobytes() == image and (host[:base] == CANARY).all() and \
            (host[base + len(image):] == CANARY).all(), (tag_, "the image or its guards changed")
    return seen


def set_table(torch, opened, table):
    """Overwrites an Opened's device table with a table dict (a table the open
    did not write)."""
    vals = np.array([table[f] for f in TABLE_FIELDS], dtype=np.uint64)
    opened.table.copy_(torch.from_numpy(vals.view(np.int64).copy()))


# ---- the damaged images the host check program and the GPU suite share ----
def get_table(name, image):
    """The table dict the gets of a get-corruption case go by: the open's, or
    for the image the open refuses a table it did not write (status 0 with
    this image's size and index handle)."""
    t = model_open(image)[0]
    if name == "index_handles":
        assert t["status"] == BAD_INDEX
        t = dict(t, status=0, data_blocks=3)
    return t


def flip_source():
    items, bs, ri = S.cases()["random_small_blocks"]
    payload, ops = make_table(items)
    image, handles, _ = S.model_build(payload, ops, bs, ri)
    return image, handles[-3][0] + handles[-3][1] + 5, queries_for(image, payload, ops)[::7]


def damaged_cases(flip_count=200):
    """[(name, image, model_open keywords, table dict for the gets, queries)]:
    every open status, every deterministic get corruption and flip_count random
    flips inside the data blocks of random_small_blocks."""
    payload, ops, base, _ = base_image()
    base_q = queries_for(base, payload, ops)[:60]
    out = []
    for name, (image, kw, _) in open_cases().items():
        out.append(("open/" + name, image, kw, model_open(image, **kw)[0], base_q))
    for name, (image, queries, _) in get_corruption_cases().items():
        out.append(("get/" + name, image, {}, get_table(name, image), queries))
    image, data_end, queries = flip_source()
    rng = np.random.default_rng(78)
    for i, bad in enumerate(flips(image, rng, flip_count, 0, data_end)):
        out.append((f"flip/{i}", bad, {}, model_open(bad)[0], queries[i % 3::3]))
    return out


def dump(path):
    """The damaged cases with the model's expected outputs, for
    tools/sst_get_host_check.cc to replay under a sanitizer (little-endian
    u64 fields; see its replay())."""
    u64 = lambda v: int(v).to_bytes(8, "little")
    table_bytes = lambda t: b"".join(u64(t[f]) for f in TABLE_FIELDS)
    cases = damaged_cases()
    out = bytearray(u64(len(cases)))
    for _, image, kw, use, queries in cases:
        want_t, want_h = model_open(image, **kw)
        with_handles = kw.get("handles", True)
        cap = kw.get("block_cap")
        cap = model_open(image)[0]["data_blocks"] if cap is None else cap
        out += u64(len(image)) + image + u64(with_handles) + u64(cap if with_handles else 0) + table_bytes(want_t)
        if want_h is None or not with_handles:
            out += u64(M64)
        else:
            out += u64(len(want_h)) + b"".join(u64(o) + u64(s) for o, s in want_h)
        out += table_bytes(use) + u64(len(queries))
        for key, seq in queries:
            r = model_get(image, use, key, seq)
            out += u64(len(key)) + key + u64(seq) + np.array(
                [tuple(r[f] for f in RESULT_FIELDS)],
                dtype=[("val_off", "<u8"), ("tag", "<u8"), ("val_len", "<u4"), ("block", "<u4"), ("status", "<u4"),
                       ("reserved", "<u4")]).tobytes()
    with open(path, "wb") as f:
        f.write(out)
    return len(cases)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "leveldb-rs_amd"))
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        print("wrote", dump(sys.argv[2]), "cases")
    else:
        raise SystemExit("usage: python tests/sst_get_cases.py dump FILE")
