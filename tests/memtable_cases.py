"""The memtable order in Python, key generators and the comparison helpers
shared by the memtable tests (test_memtable.py, test_gpu_memtable_device.py,
test_gpu_memtable_stress.py).

model_order / model_get are the model every output of lv_memtable_build_* and
lv_memtable_get_* is compared with: InternalKeyComparator::compare
(dbformat.rs:153-170) over internal keys, with a later exact duplicate in front
(SkipList::insert, skiplist.rs:85-107).  reference_memtable_print restates what
the reference's own MemTable does instead -- the same comparator over whole
encoded entries (memtable.rs:75-103) -- to pin where the two differ."""
import numpy as np

from write_batch_cases import CANARY, GUARD, M64, VALUE, guarded_payload, iterate, tail_is_canary, varint

UPSTREAM, OP_OVER, BAD_OP = 1, 2, 4
ABSENT, FOUND, DELETED, BAD_SEQ, NO_TABLE, BAD_QUERY = range(6)
MAX_SEQUENCE = (1 << 56) - 1


def op_dtype():
    from lvgpu.write_batch import OP_DTYPE
    return OP_DTYPE


def make_table(items, gaps=None):
    """(payload, ops) of items = [(key, tag, value)] in log order: each key and
    value laid into the payload one after the other, gaps[i] bytes of 0xEE
    before item i.  tag is the full u64 ((seq << 8) | type)."""
    payload, ops = bytearray(), []
    for i, (key, tag, value) in enumerate(items):
        if gaps is not None:
            payload += b"\xEE" * int(gaps[i])
        ko = len(payload)
        payload += key
        vo = len(payload)
        payload += value
        ops.append((tag & M64, ko, vo, len(key), len(value)))
    arr = np.array(ops, dtype=op_dtype()) if ops else np.zeros(0, dtype=op_dtype())
    return bytes(payload), arr


def tag(seq, typ=VALUE):
    return ((seq << 8) | typ) & M64


def key_of(payload, op):
    return payload[int(op["key_off"]):int(op["key_off"]) + int(op["key_len"])]


def _keys_tags(payload, ops):
    ko, kl = ops["key_off"].tolist(), ops["key_len"].tolist()
    return [payload[o:o + n] for o, n in zip(ko, kl)], ops["tag"].tolist()


def model_order(payload, ops):
    """Op indices in memtable order: user key ascending (bytes compare as
    unsigned, a proper prefix first), tag descending, op index descending."""
    keys, tags = _keys_tags(payload, ops)
    return sorted(range(len(ops)), key=lambda i: (keys[i], -tags[i], -i))


def model_totals(payload, ops):
    order = model_order(payload, ops)
    return order, dict(entries=len(ops), user_keys=len(set(_keys_tags(payload, ops)[0])), status=0)


def model_get(payload, ops, order, key, seq):
    """MemTable::get (memtable.rs:105-143) over the table in `order`: the first
    entry not less than (key, (seq << 8) | 1), if its user key is the query's."""
    if seq > MAX_SEQUENCE:
        return dict(val_off=0, val_len=0, op=0, status=BAD_SEQ, reserved=0)
    q = (bytes(key), -tag(seq, VALUE))
    for i in order:  # linear on purpose: no second binary search to get wrong
        o = ops[i]
        if (key_of(payload, o), -int(o["tag"])) >= q:
            if key_of(payload, o) != bytes(key):
                break
            if int(o["tag"]) & 0xFF == VALUE:
                return dict(val_off=int(o["val_off"]), val_len=int(o["val_len"]), op=i, status=FOUND, reserved=0)
            return dict(val_off=0, val_len=0, op=i, status=DELETED, reserved=0)
    return dict(val_off=0, val_len=0, op=0, status=ABSENT, reserved=0)


def model_get_fast(payload, ops, order):
    """model_get for many queries: a closure over the sorted (key, -tag) list."""
    import bisect
    keys, tags = _keys_tags(payload, ops)
    ents = [(keys[i], -tags[i]) for i in order]

    def get(key, seq):
        if seq > MAX_SEQUENCE:
            return dict(val_off=0, val_len=0, op=0, status=BAD_SEQ, reserved=0)
        at = bisect.bisect_left(ents, (bytes(key), -tag(seq, VALUE)))
        if at < len(ents) and ents[at][0] == bytes(key):
            i = order[at]
            o = ops[i]
            if int(o["tag"]) & 0xFF == VALUE:
                return dict(val_off=int(o["val_off"]), val_len=int(o["val_len"]), op=i, status=FOUND, reserved=0)
            return dict(val_off=0, val_len=0, op=i, status=DELETED, reserved=0)
        return dict(val_off=0, val_len=0, op=0, status=ABSENT, reserved=0)
    return get


# ---- printing a batch in some order (the reference's print_contents) ----
def _print(status, ops, order):
    out = ""
    for i in order:
        t, key, value = ops[i]
        if t & 0xFF == VALUE:
            out += f"Put({key.decode()}, {value.decode()})"
        else:
            out += f"Delete({key.decode()})"
        out += f"@{t >> 8}"
    if status != 0:  # iterate returned an Err ("WriteBatch has wrong count" included)
        out += "ParseError()"
    return out


def _entry(t, key, value):
    """MemTable::add's encoded entry (memtable.rs:75-103)."""
    return varint(len(key) + 8) + key + t.to_bytes(8, "little") + varint(len(value)) + value


def _entry_less(a, b):
    """InternalKeyComparator::compare(a, b) == Less over two whole entries: the
    "user key" is the entry minus its last 8 bytes, the "tag" those 8 bytes as
    a little-endian u64; a tie is Greater, never Equal."""
    ua, ub = a[:-8], b[:-8]
    if ua != ub:
        return ua < ub
    return int.from_bytes(a[-8:], "little") > int.from_bytes(b[-8:], "little")


def reference_memtable_print(rep):
    """write_batch.rs:200-238 as the reference runs it: every op handed to
    MemTable::add, whose skiplist orders whole encoded entries, a new one going
    in front of the first node that is not less than it; then the walk."""
    status, ops = iterate(rep)
    nodes = []  # (entry, op index), in skiplist order
    for i, (t, key, value) in enumerate(ops):
        e = _entry(t, key, value)
        at = 0
        while at < len(nodes) and _entry_less(nodes[at][0], e):
            at += 1
        nodes.insert(at, (e, i))
    return _print(status, ops, [i for _, i in nodes])


def product_print(rep, order_of=None):
    """The same print in the product's order (model_order, or order_of(payload,
    ops) -> op indices, e.g. the host twin)."""
    status, ops = iterate(rep)
    payload, arr = make_table(ops_items(ops))
    order = model_order(payload, arr) if order_of is None else [int(i) for i in order_of(payload, arr)]
    return _print(status, ops, order)


def ops_items(ops):
    return [(key, t, value) for t, key, value in ops]


# ---- key generators ----
def corner_groups():
    """Named groups of keys that each catch one mistake of a comparator."""
    p40 = b"common-prefix-of-exactly-40-bytes-long!!"
    assert len(p40) == 40
    big = bytes(range(256)) * 20
    big = big[:4999]
    return {
        "empty": [b"", b"\x00", b"a"],
        "len_7_8_9": [b"prefix_", b"prefix_8", b"prefix_89", b"prefix_"[:6]],
        "zero_padding": [b"a", b"a\x00", b"a\x00\x00", b"a\x00\x00\x00\x00\x00\x00\x00", b"a" + bytes(8), b"a" + bytes(9),
                         b"a" + bytes(14), b"a" + bytes(15), b"a" + bytes(16)],
        "signed_first": [b"\x7fx", b"\x80x", b"\xffx", b"\x00x"],
        "signed_ninth": [b"12345678\x7f", b"12345678\x80", b"12345678\xff", b"12345678\x00", b"12345678"],
        "signed_17th": [b"1234567812345678\x7f", b"1234567812345678\x80", b"1234567812345678\xff",
                        b"1234567812345678\x00", b"1234567812345678", b"123456781234567"],
        "byte_order": [b"ab", b"ba", b"abcdefgh" + b"ab", b"abcdefgh" + b"ba"],
        "prefix_40": [p40 + b"a", p40 + b"b", p40, p40 + b"\xff"],
        "across_edge": [b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefghij", b"abcdef", b"abcdefghijklmnop",
                        b"abcdefghijklmnopq", b"abcdefghijklmnopqrstuvwx", b"abcdefghijklmnopqrstuvwxy"],
        "long_5000": [big + b"\x01", big + b"\x02", big],
    }


def corner_items():
    """All corner keys in one table, shuffled, each at a sequence of its own."""
    keys = [k for g in corner_groups().values() for k in g]
    rng = np.random.default_rng(17)
    perm = rng.permutation(len(keys))
    return [(keys[j], tag(100 + int(i)), b"v%d" % int(i)) for i, j in enumerate(perm)]


def tag_items():
    """One user key at several sequences, VALUE and DELETION at one sequence,
    sequences >= 2^56, exact duplicates."""
    items = []
    for seq in (5, 900, 1, 77, 900):  # 900 twice: an exact duplicate below
        items.append((b"versions", tag(seq), b"v%d" % seq))
    items.append((b"versions", tag(77, 0), b""))  # DELETION at 77: after the VALUE at 77
    for seq in (1 << 56, (1 << 56) - 1, (1 << 63) >> 8, (M64 >> 8), 3):  # the tag's top bits
        items.append((b"top", tag(seq), b"t"))
        items.append((b"top", tag(seq, 0), b""))
    for _ in range(3):
        items.append((b"dup", tag(42), b"same"))  # exact duplicates: the later op first
    items.append((b"dup", tag(42, 0), b""))
    items.append((b"dup", tag(42, 0), b""))
    return items


def random_items(rng, n, alphabet=4, maxlen=24, shared=0.6, seqs=50, prefixes=None):
    """n items whose keys draw from a small alphabet, a heavy share of them
    behind one of a few shared prefixes (9-30 bytes, so ties go past the 8-byte
    prefix), with repeated sequences."""
    if prefixes is None:
        prefixes = [bytes(rng.integers(97, 97 + alphabet, size=int(rng.integers(9, 31)), dtype=np.uint8))
                    for _ in range(4)]
    items = []
    for i in range(n):
        body = bytes(rng.integers(97, 97 + alphabet, size=int(rng.integers(0, maxlen)), dtype=np.uint8))
        key = (prefixes[int(rng.integers(len(prefixes)))] if rng.random() < shared else b"") + body
        typ = 0 if rng.random() < 0.25 else 1
        items.append((key, tag(int(rng.integers(1, seqs)), typ), b"" if typ == 0 else b"val%d" % (i % 7)))
    return items


# ---- one device call ----
def dev_bytes(torch, dev, b):
    """Host bytes (or a numpy array's bytes) as a uint8 tensor on dev, at least
    16 bytes long (16-B aligned: allocations are)."""
    raw = bytearray(b.tobytes() if isinstance(b, np.ndarray) else bytes(b))
    t = torch.zeros(max(len(raw), 16), dtype=torch.uint8, device=dev)
    if raw:
        t[: len(raw)].copy_(torch.frombuffer(raw, dtype=torch.uint8))
    return t


def dev_i64(torch, dev, vals):
    a = np.ascontiguousarray(vals, dtype=np.uint64)
    if a.size == 0:
        return torch.zeros(1, dtype=torch.int64, device=dev)
    return torch.from_numpy(a.view(np.int64).copy()).to(dev)


def run_build(torch, dev, payload, ops, *, shift=0, op_cap=None, n_ops=None, upstream=None, stream=None):
    """One lv_memtable_build_device call over a guarded payload (shifted by
    `shift` bytes: every key's alignment moves with it) with a canary-filled
    d_order and a dirty workspace: (Table, payload buffer)."""
    import lvgpu.memtable as MT
    buf, d_pay = guarded_payload(torch, dev, payload, shift)
    n = len(ops)
    cap = max(n, 1) if op_cap is None else op_cap
    d_ops = dev_bytes(torch, dev, np.concatenate([ops, np.zeros(max(cap - n, 0), dtype=ops.dtype)]))
    d_n = dev_i64(torch, dev, [n if n_ops is None else n_ops])
    d_up = None if upstream is None else dev_i64(torch, dev, [upstream])
    ws = torch.full((max(MT.build_workspace_bytes(cap), 16),), 0x5A, dtype=torch.uint8, device=dev)
    table = MT.build_device(d_pay, d_ops, d_n, d_up, op_cap=cap, workspace=ws, stream=stream, fill=CANARY,
                            guard=GUARD)
    return table, buf


def compare_build(table, payload, ops, tag_=""):
    """d_order and the totals of a call whose status is 0 against the model,
    and the canaries behind d_order."""
    want_order, want_tot = model_totals(payload, ops)
    t = table.sync_totals()
    assert t == want_tot, (tag_, t, want_tot)
    got = table.order()
    want = np.array(want_order, dtype=np.uint32)
    assert got.shape == want.shape, (tag_, got.shape, want.shape)
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, (tag_, "order differs at", int(diff[0]), got[diff[0]:diff[0] + 4], want[diff[0]:diff[0] + 4])
    assert tail_is_canary(table.order_t, len(ops) * 4), (tag_, "d_order written past the entries")
    return want_order


def check(torch, dev, payload, ops, *, shift=0, op_cap=None, tag_=""):
    """Runs the build and compares d_order, the totals and the canaries around
    d_order and the payload with the model; returns (Table, model order)."""
    payload = bytes(payload)
    table, buf = run_build(torch, dev, payload, ops, shift=shift, op_cap=op_cap)
    order = compare_build(table, payload, ops, tag_)
    host = buf.cpu().numpy()
    base = (-buf.data_ptr()) % 16 + shift + GUARD
    assert (host[:base] == CANARY).all() and (host[base + len(payload):] == CANARY).all(), (tag_, "payload guards")
    assert host[base:base + len(payload)].tobytes() == payload, (tag_, "payload changed")
    table._buf = buf  # the payload view must outlive a later get
    return table, order


def untouched(table):
    return tail_is_canary(table.order_t, 0)


def pack_queries(queries, gaps=None):
    """(qkeys bytes, q_off, q_len, q_seq) of queries = [(key, seq)]."""
    qk, off = bytearray(), []
    for i, (key, _) in enumerate(queries):
        if gaps is not None:
            qk += b"\xDD" * int(gaps[i])
        off.append(len(qk))
        qk += key
    return (bytes(qk), np.array(off, dtype=np.uint64), np.array([len(k) for k, _ in queries], dtype=np.uint32),
            np.array([s for _, s in queries], dtype=np.uint64))


def run_get(torch, dev, table, qkeys, q_off, q_len, q_seq, stream=None):
    """lv_memtable_get_device with canaries behind the results: the results as
    a structured array."""
    import lvgpu.memtable as MT
    nq = len(q_off)
    d_qk = dev_bytes(torch, dev, qkeys)[: len(qkeys)] if len(qkeys) else torch.zeros(0, dtype=torch.uint8, device=dev)
    d_off = dev_i64(torch, dev, q_off)
    d_seq = dev_i64(torch, dev, q_seq)
    ln = np.ascontiguousarray(q_len, dtype=np.uint32)
    d_len = (torch.from_numpy(ln.view(np.int32).copy()).to(dev) if ln.size
             else torch.zeros(1, dtype=torch.int32, device=dev))
    res = MT.get_device(table, d_qk, d_off, d_len, d_seq, nq=nq, stream=stream, fill=CANARY, guard=GUARD)
    torch.cuda.synchronize()
    assert tail_is_canary(res, nq * 24), "d_results written past nq"
    return MT.results(res, nq)


def check_get(torch, dev, table, payload, ops, order, queries, tag_=""):
    got = run_get(torch, dev, table, *pack_queries(queries, gaps=[i % 5 for i in range(len(queries))]))
    get = model_get_fast(payload, ops, order)
    for i, (key, seq) in enumerate(queries):
        want = get(key, seq)
        g = {k: int(got[i][k]) for k in want}
        assert g == want, (tag_, i, key[:40], seq, g, want)
    return got


def queries_for(payload, ops, rng=None, extra=()):
    """For every stored version: snapshots below, at and above it; for every
    stored key, the key extended by a byte and cut by a byte; plus `extra`."""
    qs = []
    for o in ops:
        key, seq = key_of(payload, o), int(o["tag"]) >> 8
        for s in (seq - 1, seq, seq + 1):
            if 0 <= s <= MAX_SEQUENCE:
                qs.append((key, s))
    keys = sorted({key_of(payload, o) for o in ops})
    for k in keys:
        qs.append((k + b"\x00", MAX_SEQUENCE))
        qs.append((k + b"\xff", MAX_SEQUENCE))
        if k:
            qs.append((k[:-1], MAX_SEQUENCE))
    qs += list(extra)
    return qs


# ---- stress trials ----
STRESS_TRIALS = 100


def stress_trial(seed):
    """(payload, ops) of one trial: 0-6,000 ops; key lengths 0-12, 13-64 and
    now and then up to 2,000; an alphabet of 2, 16 or 256 symbols, so ties are
    frequent; random sequences with repeats; packed or gapped."""
    import random
    rng = random.Random(9000 + seed)
    n = [0, 1, rng.randrange(2, 40), rng.randrange(40, 1500), rng.randrange(1500, 6001)][rng.randrange(5)]
    sym = [2, 16, 256][rng.randrange(3)]
    nseq = rng.choice([1, 3, 1000])
    budget = 64 << 10  # bytes of long keys in one trial
    fold = bytes(i % sym for i in range(256))
    rand = lambda ln: rng.randbytes(ln).translate(fold)
    stems = [rand(rng.randrange(0, 40)) for _ in range(3)]
    items = []
    for i in range(n):
        k = rng.randrange(20)
        if k < 10:
            ln = rng.randrange(0, 13)
        elif k < 19 or budget <= 0:
            ln = rng.randrange(13, 65)
        else:
            ln = rng.randrange(65, 2001)
            budget -= ln
        key = rand(ln)
        if rng.random() < 0.5:
            key = (stems[rng.randrange(3)] + key)[: max(ln, 1)] if rng.random() < 0.5 else stems[rng.randrange(3)] + key
        typ = 0 if rng.random() < 0.2 else 1
        seq = rng.randrange(nseq) + (rng.randrange(2) << 55)
        items.append((key, tag(seq, typ), b"" if typ == 0 else b"v" * rng.randrange(4)))
    gaps = [rng.randrange(20) for _ in items] if rng.random() < 0.5 else None
    return make_table(items, gaps)
