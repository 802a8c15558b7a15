"""The range read over a sorted memtable in Python, case generators and the
comparison helpers of the range tests (test_mt_range.py,
test_mt_range_hostcheck.py, test_gpu_memtable_range.py).

model_range is written from upstream C++ LevelDB's DBIter (db/db_iter.cc:
Seek, Next and FindNextUserEntry with `skipping` and `saved_key`), not from
the group form include/lvgpu/memtable.h states and not from the ballot form the
kernel runs, so that on sorted input it also pins their equivalence.  Its
seeks are linear scans on purpose: there is no binary search to get wrong."""
import json
import os
import struct

import numpy as np

from memtable_cases import MAX_SEQUENCE, dev_bytes, dev_i64, key_of, make_table, model_order, tag
from write_batch_cases import CANARY, GUARD, guarded_payload, tail_is_canary

HAS_HI, RESUME, SEEN = 1, 2, 4
DONE, MORE_LIMIT, MORE_SCAN, BAD_SEQ, NO_TABLE, BAD_QUERY = range(6)
M = MAX_SEQUENCE
FIELDS = ("seek_pos", "next_pos", "unparsed", "count", "status", "seen", "reserved")
CANARY32 = CANARY * 0x01010101
BIG = 1 << 40  # a limit or max_scan no case reaches
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt_range_example.json")


def table_of(items, gaps=None):
    """(payload, ops, order, totals) of items in log order: the sorted
    quadruple a memtable build writes."""
    payload, ops = make_table(items, gaps)
    order = np.array(model_order(payload, ops), dtype=np.uint32)
    keys = {key_of(payload, o) for o in ops}
    return payload, ops, order, dict(entries=len(ops), user_keys=len(keys), status=0)


def pack(queries, gaps=None):
    import lvgpu.memtable as MT
    return MT.pack_range_queries(queries, gaps)


def _status_only(status):
    return [], dict(seek_pos=0, next_pos=0, unparsed=0, count=0, status=status, seen=0, reserved=0)


def entries_of(payload, ops, order, n, broken=()):
    """[(user key, tag, op index)] by position, None at a broken position."""
    return [(key_of(payload, ops[i]), int(ops[i]["tag"]), int(i)) if at not in broken else None
            for at, i in enumerate(np.asarray(order)[:n].tolist())]


def model_range(payload, ops, order, totals, qkeys, row, limit, max_scan, op_cap=None, broken=(), ents=None):
    """One query (a RANGE_QUERY_DTYPE row over qkeys) as DBIter would answer
    it: (hits as a list of op indices, the result's fields as a dict).
    `broken`: positions whose entry is out of range (a damaged quadruple); the
    walk answers NO_TABLE when it meets one, and a query that would search
    such a table is refused here, because which entries a search probes is
    unspecified."""
    n = int(totals["entries"])
    cap = len(ops) if op_cap is None else op_cap
    flags, s, pos = int(row["flags"]), int(row["seq"]), int(row["pos"])
    if totals["status"] or n > cap:
        return _status_only(NO_TABLE)
    if s > MAX_SEQUENCE:
        return _status_only(BAD_SEQ)
    inside = lambda off, ln: off <= len(qkeys) and ln <= len(qkeys) - off
    lo_off, lo_len, hi_off, hi_len = (int(row[f]) for f in ("lo_off", "lo_len", "hi_off", "hi_len"))
    if flags & ~7 or (flags & SEEN and not flags & RESUME) or (not flags & RESUME and not inside(lo_off, lo_len)) or \
            (flags & HAS_HI and not inside(hi_off, hi_len)) or (flags & RESUME and pos > n):
        return _status_only(BAD_QUERY)
    assert not broken or (flags & RESUME and not flags & HAS_HI), "a search over a damaged table is unspecified"
    if ents is None:
        ents = entries_of(payload, ops, order, n, broken)
    # DBIter::Seek: the first entry at or behind (lo, s, kValueTypeForSeek)
    if flags & RESUME:
        start = pos
    else:
        target = (qkeys[lo_off:lo_off + lo_len], -tag(s, 1))
        start = next((i for i, e in enumerate(ents) if (e[0], -e[1]) >= target), n)
    end = n
    if flags & HAS_HI:
        hi = qkeys[hi_off:hi_off + hi_len]
        end = next((i for i, e in enumerate(ents) if e[0] >= hi), n)
    # the state Next() leaves: skipping entries at or below saved_key
    skipping, saved_key = False, None
    if flags & SEEN and start > 0 and start < end:
        if ents[start - 1] is None:
            return _status_only(NO_TABLE)
        skipping, saved_key = True, ents[start - 1][0]
    p, count, examined, unparsed, hits = start, 0, 0, 0, []
    while True:
        if count == limit:
            status = MORE_LIMIT
            break
        if p >= end:
            status = DONE
            break
        if examined == max_scan:
            status = MORE_SCAN
            break
        if ents[p] is None or (p == start and p > 0 and ents[p - 1] is None):
            return _status_only(NO_TABLE)
        key, t, idx = ents[p]
        p += 1
        examined += 1
        if t & 0xFF > 1:      # ParseKey fails: the entry is skipped
            unparsed += 1
            continue
        if t >> 8 > s:        # ikey.sequence > sequence_
            continue
        if t & 0xFF == 0:     # kTypeDeletion: hide the older entries of this key
            skipping, saved_key = True, key
        elif skipping and key <= saved_key:
            pass              # hidden
        else:                 # valid_ = true; the caller's Next() saves the key and skips
            hits.append(idx)
            count += 1
            skipping, saved_key = True, key
    if examined == 0:
        seen = bool(flags & SEEN)
    else:  # whether an entry of the last examined key would be skipped
        seen = skipping and ents[p - 1][0] <= saved_key
    return hits, dict(seek_pos=start, next_pos=p, unparsed=unparsed, count=count, status=status, seen=int(seen),
                      reserved=0)


def model_all(payload, ops, order, totals, qkeys, rows, limit, max_scan, **kw):
    """model_range for every row (the entries are listed once)."""
    n, cap = int(totals["entries"]), kw.get("op_cap")
    if not totals["status"] and n <= (len(ops) if cap is None else cap):
        kw["ents"] = entries_of(payload, ops, order, n, kw.get("broken", ()))
    return [model_range(payload, ops, order, totals, qkeys, r, limit, max_scan, **kw) for r in rows]


# ---- the worked example of include/lvgpu/memtable.h ----
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_table(g):
    items = []
    for key, seq, what in g["entries"]:
        typ = 0 if what == "DEL" else int(what[5:]) if what.startswith("type ") else 1
        items.append((key.encode(), tag(seq, typ), b"" if typ != 1 else what.encode()))
    return items


def golden_query(q):
    seq = M if q["seq"] == "M" else q["seq"]
    hi = q["hi"].encode() if q.get("hi") is not None else None
    if q.get("resume"):
        return ("resume", q["pos"], q["seen_in"], hi, seq)
    return (q["lo"].encode(), hi, seq)


# ---- generators ----
def random_items(rng, n, nkeys=6, type2=True):
    """n items over few user keys, so groups are long: an empty key, keys that
    are prefixes of each other, deletions, type-2 tags (unless type2 is
    False), exact duplicates."""
    pool = [b"", b"a", b"ab", b"abc", b"ab\x00", b"b", b"k" * 9, b"k" * 9 + b"x", b"k" * 17, b"\xff", b"\xff\xff"]
    keys = [pool[int(i)] for i in rng.permutation(len(pool))[:nkeys]]
    items = []
    for i in range(n):
        r = rng.random()
        typ = 2 if r < 0.08 and type2 else 0 if r < 0.3 else 1
        it = (keys[int(rng.integers(len(keys)))], tag(int(rng.integers(1, 40)), typ), b"v%d" % i if typ == 1 else b"")
        items.append(it)
        if rng.random() < 0.1 and len(items) < n:
            items.append(it)  # an exact duplicate
    return items[:n]


def queries_over(items, snapshots, rng=None, some=None):
    """Seeks to every user key, the key extended and cut by a byte and the
    empty key, open and bounded by every other such key, at each snapshot."""
    keys = sorted({k for k, _, _ in items})
    points = sorted(set(keys) | {k + b"\x00" for k in keys} | {k[:-1] for k in keys if k} | {b"", b"\xff\xff\xff"})
    qs = []
    for s in snapshots:
        for lo in points:
            qs.append((lo, None, s))
            for hi in points:
                qs.append((lo, hi, s))
    if some is not None and len(qs) > some:
        pick = rng.permutation(len(qs))[:some]
        qs = [qs[int(i)] for i in sorted(pick)]
    return qs


def snapshots_of(items):
    seqs = sorted({t >> 8 for _, t, _ in items}) or [5]
    return [0, seqs[len(seqs) // 2], M]


def run_of(key, seqs, typ=1):
    """One user key's versions, newest first; typ a type or a function of the sequence."""
    f = typ if callable(typ) else (lambda s: typ)
    return [(key, tag(s, f(s)), b"%s@%d" % (key[:8], s) if f(s) == 1 else b"") for s in sorted(seqs, reverse=True)]


def singles(prefix, count, seq=5):
    return [(prefix + b"%04d" % i, tag(seq), b"s%d" % i) for i in range(count)]


def boundary_items(n):
    """n entries in sorted order (position == op index) with a group lying
    across every multiple of 64: groups of 7 versions start at 64 k - 3, single
    keys fill the rest.  Newest version first; every third group is led by a
    deletion, every fifth by a type-2 entry."""
    items, g = [], 0
    while len(items) < n:
        at = len(items)
        if at % 64 == 61:
            lead = 0 if g % 3 == 1 else 2 if g % 5 == 2 else 1
            items += run_of(b"g%05d" % at, range(10, 17), typ=lambda s, lead=lead: lead if s == 16 else 1)
            g += 1
        else:
            items += singles(b"g%05d-" % at, 1, seq=3 + at % 9)
    return items[:n]


def long_group_items():
    """A group of 130 versions (sequences 1..130, a deletion at 100) in
    positions 0..129: it covers two whole windows; then single keys."""
    return run_of(b"g", range(1, 131), typ=lambda s: 0 if s == 100 else 1) + singles(b"h", 40)


def special_items():
    """A type-2 entry at a group start and between a deletion and the value it
    hides; a group of type-2 entries only; a deletion above a value."""
    return [(b"k", tag(9, 2), b""), (b"k", tag(8, 0), b""), (b"k", tag(7, 2), b""), (b"k", tag(6), b"k6"),
            (b"l", tag(9, 2), b""), (b"l", tag(8, 3), b""),
            (b"m", tag(9, 2), b""), (b"m", tag(8), b"m8"), (b"m", tag(7), b"m7"),
            (b"n", tag(5, 0), b""), (b"n", tag(4), b"n4"), (b"o", tag(1), b"o1")]


def big_key_items():
    big = (bytes(range(256)) * 16)[:4095]
    return [(big + b"\x01", tag(7), b"one-7"), (big + b"\x01", tag(3), b"one-3"), (big + b"\x02", tag(5, 0), b""),
            (big + b"\x02", tag(4), b"two-4"), (big, tag(2), b"stem"), (b"z", tag(1), b"z")], big


def cpu_cases():
    """name -> (items, [(queries, limit, max_scan)]): the cases the CPU tests
    and the host program replay and the GPU test runs at every payload shift."""
    out = {}
    g = golden()
    out["example"] = (golden_table(g), [([golden_query(q)], g["limit"], q.get("max_scan", BIG)) for q in g["queries"]])
    for seed, n in ((1, 0), (2, 1), (3, 40), (4, 150), (5, 300)):
        rng = np.random.default_rng(seed)
        items = random_items(rng, n)
        qs = queries_over(items, snapshots_of(items), rng, some=120)
        out[f"random_{n}"] = (items, [(qs, BIG, BIG), (qs, 1, BIG), (qs, 3, 5), (qs, BIG, 1)])
    sp = special_items()
    out["special"] = (sp, [(queries_over(sp, [0, 5, 8, M]), lim, ms) for lim, ms in ((BIG, BIG), (1, BIG), (2, 3))])
    bk, big = big_key_items()
    qs = [(b"", None, M), (big, None, M), (big + b"\x01", big + b"\x02", M), (big + b"\x01", big + b"\x02", 4),
          (big + b"\x02", None, 4), (big + b"\x02", None, 5), (big + b"\x01\x00", None, M), (big, big + b"\x01", M)]
    out["big_keys"] = (bk, [(qs, BIG, BIG), (qs, 1, 2)])
    return out


def clamp(v):
    """A limit the host slot and the device slot can be allocated for."""
    return min(v, 512)


# ---- resume chains ----
def chain(call, row, qkeys, limit, max_scan, max_calls):
    """Runs call(row) -> (hits, result) again and again, each query the resume
    of the last result: (all hits, summed unparsed, the last result, calls)."""
    import lvgpu.memtable as MT
    hits, unparsed, calls = [], 0, 0
    first = None
    while True:
        h, r = call(row)
        calls += 1
        assert calls <= max_calls, "the chain does not end"
        first = r if first is None else first
        hits += list(h)
        unparsed += r["unparsed"]
        if r["status"] not in (MORE_LIMIT, MORE_SCAN):
            return hits, unparsed, r, first, calls
        nxt = np.zeros(1, dtype=MT.RANGE_QUERY_DTYPE)[0]
        for f in ("hi_off", "hi_len", "seq"):
            nxt[f] = row[f]
        nxt["flags"] = (int(row["flags"]) & HAS_HI) | RESUME | (SEEN if r["seen"] else 0)
        nxt["pos"] = r["next_pos"]
        row = nxt


# ---- one device call ----
def device_table(torch, dev, payload, ops, order, totals, *, shift=0, op_cap=None):
    """The quadruple in HBM as a lvgpu.memtable.Table over a guarded, shifted
    payload: (Table, payload buffer)."""
    import lvgpu.memtable as MT
    buf, d_pay = guarded_payload(torch, dev, payload, shift)
    cap = max(len(ops), 1) if op_cap is None else op_cap
    pad = np.zeros(max(cap - len(ops), 0), dtype=ops.dtype)
    d_ops = dev_bytes(torch, dev, np.concatenate([ops, pad]))
    d_order = dev_bytes(torch, dev, np.asarray(order, dtype=np.uint32)).view(torch.int32)
    d_tot = dev_i64(torch, dev, [totals["entries"], totals["user_keys"], totals["status"]])
    t = MT.Table(d_pay, d_ops, cap, d_order, d_tot, None)
    t._buf = buf
    return t, buf


def compare(got_hits, got_res, wants, limit, tag_="", met_damage=False):
    """hits (nq, limit) and results against [(hits, result)]: every field,
    hits[0, count), and the canary in [count, limit) of every slot (but, with
    met_damage, in the slot of a walk that met a damaged entry: NO_TABLE after
    hits were written)."""
    for q, (wh, wr) in enumerate(wants):
        g = {f: int(got_res[q][f]) for f in FIELDS}
        assert g == wr, (tag_, q, g, wr)
        assert got_hits[q, : wr["count"]].tolist() == wh, (tag_, q, got_hits[q, : wr["count"]].tolist()[:8], wh[:8])
        if not (met_damage and wr["status"] == NO_TABLE):
            assert (got_hits[q, wr["count"]:] == CANARY32).all(), (tag_, q, "the slot is written beyond count")


def run_device(torch, dev, table, rows, qkeys, limit, max_scan, stream=None):
    """lv_memtable_range_device with canaries in and behind d_hits and
    d_results: (hits (nq, limit), results)."""
    import lvgpu.memtable as MT
    r = MT.range_device(table, rows, qkeys, limit, max_scan, stream=stream, fill=CANARY, guard=GUARD)
    hits, res = r.sync()
    assert tail_is_canary(r.hits_t, len(rows) * limit * 4), "d_hits written past nq * limit"
    assert tail_is_canary(r.results_t, len(rows) * 40), "d_results written past nq"
    return hits, res


def check_device(torch, dev, payload, ops, order, totals, queries, limit, max_scan, *, shift=0, table=None, tag_="",
                 **model_kw):
    """One launch over `queries` (tuples, or (qkeys, rows)) against the model,
    field for field, with the canaries around d_hits, d_results and the
    payload.  Returns the model's answers."""
    qkeys, rows = queries if isinstance(queries, tuple) else pack(queries, gaps=[i % 5 for i in range(len(queries))])
    limit = clamp(limit)
    buf = None
    if table is None:
        table, buf = device_table(torch, dev, payload, ops, order, totals, shift=shift)
    hits, res = run_device(torch, dev, table, rows, qkeys, limit, max_scan)
    wants = model_all(payload, ops, order, totals, qkeys, rows, limit, max_scan, **model_kw)
    compare(hits, res, wants, limit, tag_, met_damage=bool(model_kw.get("broken")))
    if buf is not None:
        host = buf.cpu().numpy()
        base = (-buf.data_ptr()) % 16 + shift + GUARD
        assert (host[:base] == CANARY).all() and (host[base + len(payload):] == CANARY).all(), (tag_, "payload guards")
    return wants


# ---- the dump tools/mt_range_hostcheck.cc replays ----
def damaged_cases():
    """Quadruples whose parts were not written for each other: name ->
    (payload, ops, order, totals, op_cap).  The host program checks only
    containment and termination over them."""
    rng = np.random.default_rng(77)
    items = random_items(rng, 120)
    payload, ops, order, totals = table_of(items)
    out = {}
    o = order.copy()
    o[17], o[90] = len(ops), 0xFFFFFFFF
    out["damaged_order_index"] = (payload, ops, o, totals, len(ops))
    b = ops.copy()
    b[int(order[30])]["key_off"], b[int(order[75])]["key_len"] = len(payload) - 1, 0xFFFFFFFF
    b[int(order[100])]["key_off"] = (1 << 64) - 2
    out["damaged_key_extent"] = (payload, b, order, totals, len(ops))
    out["damaged_unsorted"] = (payload, ops, order[rng.permutation(len(order))], totals, len(ops))
    out["damaged_reversed"] = (payload, ops, order[::-1].copy(), totals, len(ops))
    out["damaged_entries_over"] = (payload, ops, order, dict(totals, entries=len(ops) + 5), len(ops))
    out["damaged_entries_over_cap"] = (payload, ops[:60], order, totals, 60)
    return out, items


def dump_cases():
    """[(name, payload, ops, order, totals, op_cap, qkeys, rows, limit,
    max_scan, expected | None)] for dump()."""
    cases = []
    for name, (items, settings) in cpu_cases().items():
        payload, ops, order, totals = table_of(items)
        for k, (qs, limit, max_scan) in enumerate(settings):
            qkeys, rows = pack(qs)
            limit = clamp(limit)
            want = model_all(payload, ops, order, totals, qkeys, rows, limit, max_scan)
            cases.append((f"{name}_{k}", payload, ops, order, totals, len(ops), qkeys, rows, limit, max_scan, want))
    dam, items = damaged_cases()
    qs = queries_over(items, [0, 20, M], np.random.default_rng(3), some=60)
    qs += [("resume", p, s, None, M) for p in (0, 16, 17, 18, 89, 90, 119, 120) for s in (0, 1)]
    qkeys, rows = pack(qs)
    for name, (payload, ops, order, totals, cap) in dam.items():
        for limit, max_scan in ((512, BIG), (1, 3), (5, 64)):
            cases.append((f"{name}_{limit}", payload, ops, order, totals, cap, qkeys, rows, limit, max_scan, None))
    return cases


def dump(path):
    """Writes dump_cases() for the host program: little-endian, per case the
    name, the quadruple in exact sizes, the queries and, where there is one,
    the expected result and hits of every query.  Returns the case count."""
    cases = dump_cases()
    with open(path, "wb") as f:
        f.write(b"MTRG" + struct.pack("<I", len(cases)))
        for name, payload, ops, order, totals, cap, qkeys, rows, limit, max_scan, want in cases:
            nm = name.encode()
            f.write(struct.pack("<I", len(nm)) + nm)
            f.write(struct.pack("<Q", len(payload)) + payload)
            f.write(struct.pack("<Q", len(ops)) + ops.tobytes())
            od = np.ascontiguousarray(order, dtype=np.uint32)
            f.write(struct.pack("<Q", od.size) + od.tobytes())
            f.write(struct.pack("<QQQQ", totals["entries"], totals["user_keys"], totals["status"], cap))
            f.write(struct.pack("<Q", len(qkeys)) + qkeys)
            f.write(struct.pack("<IIQI", len(rows), limit, max_scan, 0 if want is None else 1))
            f.write(np.ascontiguousarray(rows).tobytes())
            if want is not None:
                for hits, r in want:
                    f.write(struct.pack("<QQQIIII", *(r[k] for k in FIELDS)))
                    f.write(np.asarray(hits, dtype=np.uint32).tobytes())
    return len(cases)
