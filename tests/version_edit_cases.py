"""A serial Python model of VersionEdit::encode_to / decode_from, written from
src/version_edit.rs:192-319 and :357-369 and src/util/coding.rs:186-305 of the
reference (not from the C code), the cases the CPU and GPU tests share, and the
dump tools/version_edit_hostcheck.cc replays.

An edit in the model is a dict: comparator (bytes or None), log_number,
prev_log_number, next_file_number, last_sequence (int or None), pointers
[(level, key)], deleted [(level, number)], files [(level, number, file_size,
smallest, largest)].  decode() returns the C structs' view of it instead:
offsets into the record, has bits, flags.
"""
import copy
import hashlib
import json
import os
import random
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "version_edit_example.json")

OK, UNKNOWN_TAG, INVALID_TAG, BAD_VARINT32, BAD_VARINT64, BAD_LENGTH, BAD_LEVEL, OUT_OF_RANGE = range(8)
HAS = {"comparator": 1, "log_number": 2, "prev_log_number": 4, "next_file_number": 8, "last_sequence": 16}
FLAG_NEG_LEVEL, FLAG_SHORT_KEY = 1, 2
NUM_LEVELS = 7  # config.rs:18
M64 = (1 << 64) - 1


# ---- coding.rs ------------------------------------------------------------------
def varint(v):
    """encode_varint_32 / encode_varint_64: the same bytes for a value both hold."""
    out = bytearray()
    while v >= 128:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _decode_varint(data, pos, last_shift, mask):
    """decode_varint_{32,64}_limit over data[pos:]: (value, new pos) or None.
    `while shift <= last_shift && idx < limit`; bits beyond the type fall off."""
    shift, result = 0, 0
    while shift <= last_shift and pos < len(data):
        byte = data[pos]
        pos += 1
        result |= ((byte & 0x7F) << shift) & mask
        shift += 7
        if byte & 0x80 == 0:
            return result, pos
    return None


def decode_varint32(data, pos):
    return _decode_varint(data, pos, 28, 0xFFFFFFFF)


def decode_varint64(data, pos):
    return _decode_varint(data, pos, 63, M64)


def internal_key(user_key, seq, vtype):
    """InternalKey::new: the user key, then (seq << 8 | type) as fixed64."""
    return bytes(user_key) + struct.pack("<Q", (seq << 8) | vtype)


# ---- version_edit.rs --------------------------------------------------------------
def new_edit(**kw):
    e = dict(comparator=None, log_number=None, prev_log_number=None, next_file_number=None, last_sequence=None,
             pointers=[], deleted=[], files=[])
    e.update(kw)
    return e


def _i32(level):
    return level - (1 << 32) if level & 0x80000000 else level


def encode_to(e):
    """VersionEdit::encode_to (:192-234).  deleted_files is a BTreeSet<(i32,
    u64)>: iterated in that order, without duplicates."""
    out = bytearray()
    if e["comparator"] is not None:
        out += varint(1) + varint(len(e["comparator"])) + e["comparator"]
    for tag, name in ((2, "log_number"), (9, "prev_log_number"), (3, "next_file_number"), (4, "last_sequence")):
        if e[name] is not None:
            out += varint(tag) + varint(e[name])
    for level, key in e["pointers"]:
        out += varint(5) + varint(level & 0xFFFFFFFF) + varint(len(key)) + key
    for level, number in sorted(set((_i32(l), n) for l, n in e["deleted"])):
        out += varint(6) + varint(level & 0xFFFFFFFF) + varint(number)
    for level, number, size, smallest, largest in e["files"]:
        out += (varint(7) + varint(level & 0xFFFFFFFF) + varint(number) + varint(size) + varint(len(smallest)) + smallest +
                varint(len(largest)) + largest)
    return bytes(out)


class _Err(Exception):
    pass


def decode(rec, base=0):
    """VersionEdit::decode_from (:236-319) on VersionEdit::new(), as the C
    structs report it: dict(status, has, flags, scalars, comparator (off, len),
    files [(number, size, s_off, s_len, l_off, l_len, level)], deleted
    [(number, level)], pointers [(key_off, key_len, level)]), offsets + base."""
    rec = bytes(rec)
    st = dict(status=OK, has=0, flags=0, log_number=0, prev_log_number=0, next_file_number=0, last_sequence=0,
              comparator=(0, 0), files=[], deleted=[], pointers=[])
    pos = 0

    def v32():
        nonlocal pos
        r = decode_varint32(rec, pos)
        if r is None:
            raise _Err(BAD_VARINT32)
        pos = r[1]
        return r[0]

    def v64():
        nonlocal pos
        r = decode_varint64(rec, pos)
        if r is None:
            raise _Err(BAD_VARINT64)
        pos = r[1]
        return r[0]

    def string():  # decode_length_prefixed_slice
        nonlocal pos
        n = v32()
        if len(rec) - pos < n:
            raise _Err(BAD_LENGTH)
        at = pos
        pos += n
        return at + base, n

    def level():  # get_level: (v as i32) < NUM_LEVELS
        v = v32()
        if _i32(v) >= NUM_LEVELS:
            raise _Err(BAD_LEVEL)
        if v & 0x80000000:
            st["flags"] |= FLAG_NEG_LEVEL
        return v

    def key():
        at, n = string()
        if n < 8:
            st["flags"] |= FLAG_SHORT_KEY
        return at, n

    try:
        while True:
            r = decode_varint32(rec, pos)
            if r is None:  # "No more input"
                if pos < len(rec):
                    raise _Err(INVALID_TAG)
                break
            pos = r[1]
            tag = r[0] & 0xFF  # tag_num.unwrap() as u8
            if tag == 1:
                st["comparator"] = string()
                st["has"] |= 1
            elif tag in (2, 9, 3, 4):
                name = {2: "log_number", 9: "prev_log_number", 3: "next_file_number", 4: "last_sequence"}[tag]
                st[name] = v64()
                st["has"] |= HAS[name]
            elif tag == 5:
                lv = level()
                at, n = key()
                st["pointers"].append((at, n, lv))
            elif tag == 6:
                lv = level()
                st["deleted"].append((v64(), lv))
            elif tag == 7:
                lv = level()
                number, size = v64(), v64()
                s, l = key(), key()
                st["files"].append((number, size, s[0], s[1], l[0], l[1], lv))
            else:
                raise _Err(UNKNOWN_TAG)
    except _Err as err:  # Err: what the object holds is not a result
        st = dict(status=err.args[0], has=0, flags=0, log_number=0, prev_log_number=0, next_file_number=0,
                  last_sequence=0, comparator=(0, 0), files=[], deleted=[], pointers=[])
    return st


def to_edit(d, rec, base=0):
    """The model's edit dict of a decode() result (for re-encoding)."""
    rec = bytes(rec)
    cut = lambda off, n: rec[off - base:off - base + n]
    e = new_edit()
    if d["has"] & 1:
        e["comparator"] = cut(*d["comparator"])
    for name, bit in HAS.items():
        if name != "comparator" and d["has"] & bit:
            e[name] = d[name]
    e["pointers"] = [(lv, cut(off, n)) for off, n, lv in d["pointers"]]
    e["deleted"] = [(lv, num) for num, lv in d["deleted"]]
    e["files"] = [(lv, num, size, cut(so, sn), cut(lo, ln)) for num, size, so, sn, lo, ln, lv in d["files"]]
    return e


# ---- the C tables of a batch ---------------------------------------------------------
def _dtypes():
    import lvgpu.version_edit as VE
    return VE.EDIT_DTYPE, VE.FILE_DTYPE, VE.DELETED_DTYPE, VE.POINTER_DTYPE


def decode_batch(payload, rec_off, rec_len):
    """What lv_version_edit_decode_device writes for these records: (edits,
    files, deleted, pointers, bounds (3 arrays), totals dict)."""
    ED, FD, DD, PD = _dtypes()
    payload = bytes(payload)
    n = len(rec_off)
    edits = np.zeros(n, dtype=ED)
    files, deleted, pointers = [], [], []
    bf, bd, bp = [0], [0], [0]
    bad, first_bad = 0, n
    last_has = [0] * 5
    for r, (o, l) in enumerate(zip(rec_off, rec_len)):
        o, l = int(o), int(l)
        if o > len(payload) or l > len(payload) - o:
            d = dict(decode(b""), status=OUT_OF_RANGE)
        else:
            d = decode(payload[o:o + l], base=o)
        e = edits[r]
        for name in ("log_number", "prev_log_number", "next_file_number", "last_sequence", "has", "flags", "status"):
            e[name] = d[name]
        e["comparator_off"], e["comparator_len"] = d["comparator"]
        if d["status"] != OK:
            bad += 1
            first_bad = min(first_bad, r)
        elif first_bad == n:
            for b in range(5):
                if d["has"] >> b & 1:
                    last_has[b] = r + 1
        files += [(num, size, so, lo, sn, ln, lv, 0) for num, size, so, sn, lo, ln, lv in d["files"]]
        deleted += [(num, lv, 0) for num, lv in d["deleted"]]
        pointers += d["pointers"]
        bf.append(len(files))
        bd.append(len(deleted))
        bp.append(len(pointers))
    tot = dict(records=n, files=len(files), deleted=len(deleted), pointers=len(pointers), bad_records=bad,
               first_bad=first_bad, status=0)
    tot.update({f"last_has{b}": last_has[b] for b in range(5)})
    return (edits, np.array(files, dtype=FD), np.array(deleted, dtype=DD), np.array(pointers, dtype=PD),
            tuple(np.array(b, dtype=np.uint64) for b in (bf, bd, bp)), tot)


def tables_of(edits, lead=(0, 0, 0)):
    """The encode's inputs for model edits: (src, edits, files, rec_file,
    deleted, rec_deleted, pointers, rec_pointer).  Every comparator and key
    gets its own extent of src, behind one byte that is nobody's; lead = rows
    of 0xEE bytes in front of each table that no record covers (level 0xEEEEEEEE:
    any check that looked at them would refuse)."""
    ED, FD, DD, PD = _dtypes()
    src = bytearray(b"\xa5")

    def put(b):
        at = len(src)
        src.extend(b)
        return at, len(b)

    E = np.zeros(len(edits), dtype=ED)
    files = [tuple([0xEEEEEEEEEEEEEEEE] * 4 + [0xEEEEEEEE] * 4)] * lead[0]
    deleted = [(0xEEEEEEEEEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEE)] * lead[1]
    pointers = [(0xEEEEEEEEEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEE)] * lead[2]
    bf, bd, bp = [len(files)], [len(deleted)], [len(pointers)]
    for r, e in enumerate(edits):
        if e["comparator"] is not None:
            E[r]["comparator_off"], E[r]["comparator_len"] = put(e["comparator"])
            E[r]["has"] |= 1
        for name, bit in HAS.items():
            if name != "comparator" and e[name] is not None:
                E[r][name] = e[name]
                E[r]["has"] |= bit
        for lv, key in e["pointers"]:
            pointers.append(put(key) + (lv,))
        for lv, num in e["deleted"]:
            deleted.append((num, lv, 0))
        for lv, num, size, s, l in e["files"]:
            so, sn = put(s)
            lo, ln = put(l)
            files.append((num, size, so, lo, sn, ln, lv, 0))
        bf.append(len(files))
        bd.append(len(deleted))
        bp.append(len(pointers))
    u = lambda b: np.array(b, dtype=np.uint64)
    return (bytes(src), E, np.array(files, dtype=FD), u(bf), np.array(deleted, dtype=DD), u(bd),
            np.array(pointers, dtype=PD), u(bp))


def encode_batch(src_bytes, E, F, bf, D, bd, P, bp, records=None, caps=None, src=None, out_cap=None):
    """lv_version_edit_encode_*'s judgement and output per version_edit.h: (out
    bytes or None, rec_off, rec_len, totals dict).  records: the caller's count."""
    n = len(E) if records is None else records
    caps = (len(F), len(D), len(P)) if caps is None else caps
    none = M64
    tot = dict(records=n, files=0, deleted=0, pointers=0, key_bytes=0, out_bytes=0, status=0, bad_record=none,
               bad_kind=none, bad_row=none)
    bf, bd, bp = ([int(x) for x in b] for b in (bf, bd, bp))
    for r in range(n):
        for kind, b, cap in ((1, bp, caps[2]), (2, bd, caps[1]), (3, bf, caps[0])):
            if not (b[r] <= b[r + 1] <= cap):
                tot.update(status=4, bad_record=r, bad_kind=kind)
                return None, [], [], tot
    inside = lambda off, ln: int(off) <= src_bytes and int(ln) <= src_bytes - int(off)

    def bad(kind, row, r):
        tot.update(status=8, bad_record=r, bad_kind=kind, bad_row=row)
        return None, [], [], tot
    for r in range(n):
        e = E[r]
        if int(e["has"]) & ~31 or (int(e["has"]) & 1 and not inside(e["comparator_off"], e["comparator_len"])):
            return bad(0, r, r)
    for r in range(n):
        for i in range(bp[r], bp[r + 1]):
            if int(P[i]["level"]) >= NUM_LEVELS or not inside(P[i]["key_off"], P[i]["key_len"]):
                return bad(1, i, r)
    for r in range(n):
        for i in range(bd[r], bd[r + 1]):
            if int(D[i]["level"]) >= NUM_LEVELS or (i > bd[r] and not (
                    (int(D[i - 1]["level"]), int(D[i - 1]["number"])) < (int(D[i]["level"]), int(D[i]["number"])))):
                return bad(2, i, r)
    for r in range(n):
        for i in range(bf[r], bf[r + 1]):
            f = F[i]
            if (int(f["level"]) >= NUM_LEVELS or not inside(f["smallest_off"], f["smallest_len"]) or
                    not inside(f["largest_off"], f["largest_len"])):
                return bad(3, i, r)
    cut = (lambda off, ln: src[int(off):int(off) + int(ln)]) if src is not None else (lambda off, ln: bytes(int(ln)))
    out, rec_off, rec_len, kb = bytearray(), [], [], 0
    for r in range(n):
        e = new_edit()
        if int(E[r]["has"]) & 1:
            e["comparator"] = cut(E[r]["comparator_off"], E[r]["comparator_len"])
            kb += len(e["comparator"])
        for name, bit in HAS.items():
            if name != "comparator" and int(E[r]["has"]) & bit:
                e[name] = int(E[r][name])
        e["pointers"] = [(int(P[i]["level"]), cut(P[i]["key_off"], P[i]["key_len"])) for i in range(bp[r], bp[r + 1])]
        e["deleted"] = [(int(D[i]["level"]), int(D[i]["number"])) for i in range(bd[r], bd[r + 1])]
        e["files"] = [(int(F[i]["level"]), int(F[i]["number"]), int(F[i]["file_size"]),
                       cut(F[i]["smallest_off"], F[i]["smallest_len"]), cut(F[i]["largest_off"], F[i]["largest_len"]))
                      for i in range(bf[r], bf[r + 1])]
        kb += sum(len(k) for _, k in e["pointers"]) + sum(len(s) + len(l) for *_, s, l in e["files"])
        b = encode_to(e)
        rec_off.append(len(out))
        rec_len.append(len(b))
        out += b
    tot.update(files=bf[n] - bf[0] if n else 0, deleted=bd[n] - bd[0] if n else 0, pointers=bp[n] - bp[0] if n else 0,
               key_bytes=kb, out_bytes=len(out))
    if out_cap is not None and len(out) > out_cap:
        tot["status"] = 16
        return None, [], [], tot
    return (bytes(out) if src is not None else None), rec_off, rec_len, tot


# ---- known answers ------------------------------------------------------------------
def example_edit():
    return new_edit(comparator=b"foo", log_number=300, prev_log_number=0, next_file_number=7, last_sequence=128,
                    pointers=[(1, internal_key(b"x", 5, 1))], deleted=[(2, 9)],
                    files=[(3, 10, 1000, internal_key(b"a", 1, 1), internal_key(b"b", 2, 0))])


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def reference_test_edits():
    """version_edit.rs:391-417: the edit before each of the four rounds, then
    with the four scalars."""
    BIG = 1 << 50
    e = new_edit()
    out = []
    for i in range(4):
        out.append(copy.deepcopy(e))
        e["files"].append((3, BIG + 300 + i, BIG + 400 + i, internal_key(b"foo", BIG + 500 + i, 1),
                           internal_key(b"zoo", BIG + 600 + i, 0)))
        e["deleted"].append((4, BIG + 700 + i))
        e["pointers"].append((i, internal_key(b"x", BIG + 900 + i, 1)))
    e.update(comparator=b"foo", log_number=BIG + 100, next_file_number=BIG + 200, last_sequence=BIG + 1000)
    out.append(e)
    return out


def _jsonable(e):
    return dict(e, comparator=None if e["comparator"] is None else e["comparator"].hex(),
                pointers=[(l, k.hex()) for l, k in e["pointers"]], deleted=[list(d) for d in e["deleted"]],
                files=[(l, n, s, a.hex(), b.hex()) for l, n, s, a, b in e["files"]])


def _from_jsonable(j):
    return dict(j, comparator=None if j["comparator"] is None else bytes.fromhex(j["comparator"]),
                pointers=[(l, bytes.fromhex(k)) for l, k in j["pointers"]], deleted=[tuple(d) for d in j["deleted"]],
                files=[(l, n, s, bytes.fromhex(a), bytes.fromhex(b)) for l, n, s, a, b in j["files"]])


REFERENCE_TEST_SHA256 = "9b8d210bdabf8a1c824a8786ced4a9f8599209bdb1b78e9f40f437caf6465a46"
REFERENCE_TEST_BYTES = 288

# one-record quirks: (hex, status, what else holds)
QUIRKS = [
    ("", OK, {}),
    ("81020141", OK, {"comparator": (3, 1), "has": 1}),
    ("08", UNKNOWN_TAG, {}),
    ("00", UNKNOWN_TAG, {}),
    ("80", INVALID_TAG, {}),
    ("818080808000", INVALID_TAG, {}),
    ("020180", INVALID_TAG, {}),
    ("060701", BAD_LEVEL, {}),
    ("06808080800801", OK, {"deleted": [(1, 1 << 31)], "flags": FLAG_NEG_LEVEL}),
    ("06808080801001", OK, {"deleted": [(1, 0)], "flags": 0}),
    ("02" + "ff" * 9 + "7f", OK, {"log_number": M64, "has": 2}),
    ("02" + "ff" * 10 + "00", BAD_VARINT64, {}),
    ("02", BAD_VARINT64, {}),
    ("010541", BAD_LENGTH, {}),
    ("02010205", OK, {"log_number": 5, "has": 2}),
]

# one record for every status a record can have (OUT_OF_RANGE is the device's, by extent)
STATUS_RECORDS = {OK: "0203", UNKNOWN_TAG: "0a", INVALID_TAG: "020180", BAD_VARINT32: "018080808080",
                  BAD_VARINT64: "04", BAD_LENGTH: "0503037878", BAD_LEVEL: "050700"}


# ---- generators ----------------------------------------------------------------------
def random_edit(rng, max_rows=4, max_key=24, big=False):
    num = lambda: rng.choice([rng.randrange(0, 200), rng.getrandbits(rng.randrange(1, 65))])
    key = lambda: bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 3, 8, 9, rng.randrange(0, max_key + 1)])))
    e = new_edit()
    if rng.random() < 0.5:
        e["comparator"] = bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 200 if big else 30)))
    for name in ("log_number", "prev_log_number", "next_file_number", "last_sequence"):
        if rng.random() < 0.5:
            e[name] = num()
    e["pointers"] = [(rng.randrange(7), key()) for _ in range(rng.randrange(max_rows + 1))]
    e["deleted"] = sorted(set((rng.randrange(7), num()) for _ in range(rng.randrange(max_rows + 1))))
    e["files"] = [(rng.randrange(7), num(), num(), key(), key()) for _ in range(rng.randrange(max_rows + 1))]
    return e


def random_edits(seed, n, **kw):
    rng = random.Random(seed)
    return [random_edit(rng, **kw) for _ in range(n)]


def lay_out(records, rng=None, gap=0, lead=0):
    """Records end to end (gap bytes of 0xCC between them, lead in front):
    (payload, rec_off, rec_len)."""
    payload = bytearray(b"\xcc" * lead)
    off, ln = [], []
    for r in records:
        off.append(len(payload))
        ln.append(len(r))
        payload += r
        payload += b"\xcc" * (gap if rng is None else rng.randrange(gap + 1))
    return bytes(payload), off, ln


def damaged_records():
    """The example's 55 prefixes, every single-byte flip of it (bit 0x80 and
    bit 0x01 and all bits), and the quirks."""
    ex = encode_to(example_edit())
    out = [(f"prefix_{k}", ex[:k]) for k in range(len(ex))]
    for i in range(len(ex)):
        for m in (0x80, 0x01, 0xFF, 0x07):
            b = bytearray(ex)
            b[i] ^= m
            out.append((f"flip_{i}_{m:02x}", bytes(b)))
    out += [(f"quirk_{k}", bytes.fromhex(h)) for k, (h, _, _) in enumerate(QUIRKS)]
    out += [(f"status_{s}", bytes.fromhex(h)) for s, h in STATUS_RECORDS.items()]
    return out


# ---- the dump the host check replays ----------------------------------------------------
def _blob(b):
    b = bytes(b)
    return struct.pack("<Q", len(b)) + b + bytes(-len(b) % 8)


def _decode_case(name, rec):
    ED, FD, DD, PD = _dtypes()
    edits, F, D, P, _, tot = decode_batch(rec, [0], [len(rec)])
    return (_blob(name.encode()) + struct.pack("<Q", 0) + _blob(rec) + struct.pack("<Q", int(edits[0]["status"])) +
            _blob(edits.tobytes()) + _blob(F.tobytes()) + _blob(D.tobytes()) + _blob(P.tobytes()))


def _encode_case(name, src, E, F, bf, D, bd, P, bp, records=None, caps=None):
    records = len(E) if records is None else records
    caps = (len(F), len(D), len(P)) if caps is None else caps
    out, ro, rl, tot = encode_batch(len(src), E, F, bf, D, bd, P, bp, records=records, caps=caps, src=src)
    import lvgpu.version_edit as VE
    u = lambda a: np.array(a, dtype=np.uint64).tobytes()
    return (_blob(name.encode()) + struct.pack("<Q", 1) + _blob(src) + struct.pack("<Q", records) + _blob(E.tobytes()) +
            _blob(F.tobytes()) + struct.pack("<Q", caps[0]) + _blob(u(bf)) + _blob(D.tobytes()) +
            struct.pack("<Q", caps[1]) + _blob(u(bd)) + _blob(P.tobytes()) + struct.pack("<Q", caps[2]) + _blob(u(bp)) +
            _blob(u([tot[k] for k in VE.ENCODE_TOTALS])) + _blob(out or b"") + _blob(u(ro)) + _blob(u(rl)))


def damaged_encode_inputs():
    """(name, tables, records, caps): bounds out of order or beyond the capacity,
    extents outside the source, bad levels and has bits, deleted rows out of
    order -- each with the verdict the header gives."""
    out = []
    for k, seed in enumerate((11, 12, 13)):
        edits = [e for e in random_edits(seed, 6) ]
        edits[2]["pointers"].append((1, b"pointerkey"))
        edits[3]["deleted"] = [(1, 5), (2, 3)]
        edits[4]["files"].append((2, 7, 70, b"smallestkey", b"largestkey"))
        edits[1]["comparator"] = b"cmp"
        base = tables_of(edits, lead=(1, 2, 1))
        for which, idx in (("file", 3), ("deleted", 5), ("pointer", 7)):
            t = [np.array(x) if not isinstance(x, bytes) else x for x in base]
            t[idx][3], t[idx][4] = t[idx][4] + 1, t[idx][3]  # out of order (or equal + 1)
            out.append((f"damaged_bounds_order_{which}_{k}", t, None, None))
            t = [np.array(x) if not isinstance(x, bytes) else x for x in base]
            t[idx][-1] += 1  # beyond the capacity
            out.append((f"damaged_bounds_over_{which}_{k}", t, None, None))
        t = [np.array(x) if not isinstance(x, bytes) else x for x in base]
        t[6][int(t[7][2])]["key_off"] = len(base[0]) - 3  # the key runs past the source's end
        t[6][int(t[7][2])]["key_len"] = 4
        out.append((f"damaged_pointer_extent_{k}", t, None, None))
        t = [np.array(x) if not isinstance(x, bytes) else x for x in base]
        t[2][int(t[3][5]) - 1]["largest_off"] = M64
        out.append((f"damaged_file_extent_{k}", t, None, None))
        t = [np.array(x) if not isinstance(x, bytes) else x for x in base]
        t[1][1]["comparator_len"] = 0xFFFFFFFF
        out.append((f"damaged_comparator_extent_{k}", t, None, None))
        t = [np.array(x) if not isinstance(x, bytes) else x for x in base]
        t[1][5]["has"] |= 32
        out.append((f"damaged_has_{k}", t, None, None))
        t = [np.array(x) if not isinstance(x, bytes) else x for x in base]
        t[2][int(t[3][4])]["level"] = 7
        out.append((f"damaged_file_level_{k}", t, None, None))
        t = [np.array(x) if not isinstance(x, bytes) else x for x in base]
        lo = int(t[5][3])
        t[4][lo + 1] = t[4][lo]  # a duplicate: not strictly ascending
        out.append((f"damaged_deleted_order_{k}", t, None, None))
    return out


def dump_cases():
    """[(name, bytes of the case)]."""
    cases = [(n, _decode_case(n, rec)) for n, rec in damaged_records()]
    for k, e in enumerate(reference_test_edits() + [example_edit()] + random_edits(5, 40) + random_edits(6, 6, max_rows=40, big=True)):
        cases.append((f"decode_model_{k}", _decode_case(f"decode_model_{k}", encode_to(e))))
    for k, seed in enumerate((1, 2, 3, 4)):
        edits = random_edits(seed, (1, 5, 20, 60)[k], max_rows=(2, 4, 8, 3)[k])
        cases.append((f"encode_model_{k}", _encode_case(f"encode_model_{k}", *tables_of(edits, lead=(k, 1, 2)))))
    cases.append(("encode_example", _encode_case("encode_example", *tables_of([example_edit()]))))
    cases.append(("encode_empty", _encode_case("encode_empty", *tables_of([]))))
    for name, t, records, caps in damaged_encode_inputs():
        cases.append((name, _encode_case(name, *t, records=records, caps=caps)))
    return cases


def dump(path):
    cases = dump_cases()
    with open(path, "wb") as f:
        f.write(b"VEDUMP01" + struct.pack("<Q", len(cases)))
        for _, c in cases:
            f.write(c)
    return len(cases)


def sha256(b):
    return hashlib.sha256(b).hexdigest()
