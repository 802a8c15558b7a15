"""lv_memtable_range_host against the worked example of
include/lvgpu/memtable.h, the independent DBIter model (tests/mt_range_cases.py)
and lv_memtable_get_host: the example byte for byte, random tables with long
groups, agreement with Get, resume chains, every status in its priority
order, every refused argument.  Needs no GPU."""
import ctypes

import numpy as np
import pytest

import lvgpu
import lvgpu.memtable as MT
import memtable_cases as MC
import mt_range_cases as C
from mt_range_cases import BAD_QUERY, BAD_SEQ, BIG, DONE, HAS_HI, M, MORE_LIMIT, MORE_SCAN, NO_TABLE, RESUME, SEEN

STATUS = {"DONE": DONE, "MORE_LIMIT": MORE_LIMIT, "MORE_SCAN": MORE_SCAN}


def host(payload, ops, order, totals, qkeys, row, limit, max_scan, **kw):
    """The twin over one query with a canary-filled slot: (hits, result), and
    the slot beyond count is untouched."""
    slot, r = MT.range_host(payload, ops, order, totals, qkeys, row, limit, max_scan, canary=C.CANARY32, **kw)
    assert (slot[r["count"]:] == C.CANARY32).all(), "the slot is written beyond count"
    return slot[: r["count"]].tolist(), r


def both(payload, ops, order, totals, queries, limit, max_scan, tag_=""):
    qkeys, rows = C.pack(queries, gaps=[i % 3 for i in range(len(queries))])
    out = []
    for i, row in enumerate(rows):
        want = C.model_range(payload, ops, order, totals, qkeys, row, limit, max_scan)
        got = host(payload, ops, order, totals, qkeys, row, limit, max_scan)
        assert got == want, (tag_, i, queries[i], got, want)
        out.append(want)
    return out


def test_worked_example():
    g = C.golden()
    items = C.golden_table(g)
    assert [(k.decode(), t >> 8) for k, t, _ in items] == [(e[0], e[1]) for e in g["entries"]] and len(items) == 10
    payload, ops, order, totals = C.table_of(items)
    assert order.tolist() == list(range(10))  # a position is its op index
    assert g["limit"] == 4 and len(g["queries"]) == 7
    for q in g["queries"]:
        want_hits = q["hits"]
        want = dict(seek_pos=q["seek_pos"], next_pos=q["next_pos"], unparsed=q["unparsed"], count=q["count"],
                    status=STATUS[q["status"]], seen=q["seen"], reserved=0)
        qkeys, rows = C.pack([C.golden_query(q)])
        ms = q.get("max_scan", BIG)
        assert host(payload, ops, order, totals, qkeys, rows[0], 4, ms) == (want_hits, want), q
        assert C.model_range(payload, ops, order, totals, qkeys, rows[0], 4, ms) == (want_hits, want), q


def test_worked_example_is_the_headers():
    """The header's table states the same rows as the golden file."""
    import os
    import re
    with open(os.path.join(os.path.dirname(C.GOLDEN), "..", "..", "include", "lvgpu", "memtable.h")) as f:
        text = f.read()
    text = text[text.index("The worked example"):text.index("One launch, one wave per query")]
    g = C.golden()
    lines = [ln.split() for ln in text.splitlines() if re.search(r"\s(DONE|MORE_LIMIT|MORE_SCAN)$", ln)]
    assert len(lines) == len(g["queries"]) == 7
    for t, q in zip(lines, g["queries"]):  # from the right: status, unparsed, seen, next, count, the hits, seek
        count = int(t[-5])
        hits = [int(x) for x in t[-5 - count:-5]] if count else []
        assert count or t[-6] == "-"
        seek = int(t[-6 - max(count, 1)])
        assert (seek, hits, count, int(t[-4]), int(t[-3]), int(t[-2]), t[-1]) == \
            (q["seek_pos"], q["hits"], q["count"], q["next_pos"], q["seen"], q["unparsed"], q["status"]), (t, q)
    ents = re.findall(r"\d \((\w),(\d+),(\"\w+\"|DEL|type 2)\)", text)
    assert [(k, int(s), w.strip('"')) for k, s, w in ents] == [tuple(e) for e in g["entries"]]


@pytest.mark.parametrize("name", list(C.cpu_cases()))
def test_twin_equals_the_model(name):
    items, settings = C.cpu_cases()[name]
    payload, ops, order, totals = C.table_of(items)
    seen = set()
    for queries, limit, max_scan in settings:
        for _, r in both(payload, ops, order, totals, queries, C.clamp(limit), max_scan, name):
            seen.add(r["status"])
    if name == "random_300":
        assert seen == {DONE, MORE_LIMIT, MORE_SCAN}


def test_random_tables_have_what_they_should():
    """The random tables are not hollow: long groups, deletions, exact
    duplicates, type-2 tags, an empty key and keys that are prefixes."""
    items = C.random_items(np.random.default_rng(5), 300)
    keys = {k for k, _, _ in items}
    assert len(items) == 300 and len(keys) <= 6
    types = [t & 0xFF for _, t, _ in items]
    assert types.count(0) > 30 and types.count(2) > 10 and len(set(items)) < len(items)
    allk = set()
    for seed in (3, 4, 5):
        allk |= {k for k, _, _ in C.random_items(np.random.default_rng(seed), 150)}
    assert b"" in allk and any(a != b and b.startswith(a) and a for a in allk for b in allk)


@pytest.mark.parametrize("seed", [11, 12])
def test_get_agreement(seed):
    """A range [k, k + "\\0") with limit 1 has count == 1 iff Get says FOUND,
    and then its hit is Get's op; DELETED and ABSENT give count == 0.  Over
    tables of VALUE and DELETION tags, the two types Get knows: it reads any
    other type as a deletion, where DBIter skips the entry as unparsable."""
    rng = np.random.default_rng(seed)
    items = C.random_items(rng, 200, type2=False)
    payload, ops, order, totals = C.table_of(items)
    keys = sorted({k for k, _, _ in items} | {b"zz", b"a\x00"})
    seqs = sorted({t >> 8 for _, t, _ in items})
    statuses = set()
    for k in keys:
        for s in [0, M] + seqs:
            g = MT.get_host(payload, ops, order, totals, k, s)
            qkeys, rows = C.pack([(k, k + b"\x00", s)])
            hits, r = host(payload, ops, order, totals, qkeys, rows[0], 1, BIG)
            statuses.add(g["status"])
            if g["status"] == MC.FOUND:
                assert r["count"] == 1 and hits == [g["op"]], (k, s, g, r)
            else:
                assert g["status"] in (MC.DELETED, MC.ABSENT) and r["count"] == 0 and hits == [], (k, s, g, r)
    assert statuses == {MC.FOUND, MC.DELETED, MC.ABSENT}


@pytest.mark.parametrize("limit,max_scan", [(1, 1), (3, 5), (2, 64), (64, 2)])
def test_resume_chains(limit, max_scan):
    """A chain of calls, each the resume of the last result, concatenates to
    the answer of one call with a large limit and max_scan."""
    rng = np.random.default_rng(limit * 100 + max_scan)
    items = C.random_items(rng, 260) + C.special_items()
    payload, ops, order, totals = C.table_of(items)
    n = len(items)
    queries = C.queries_over(items, C.snapshots_of(items), rng, some=40) + [(b"", None, M), (b"", None, 20)]
    qkeys, rows = C.pack(queries)
    longest = 0
    for i, row in enumerate(rows):
        one_hits, one = host(payload, ops, order, totals, qkeys, row, 512, BIG)
        assert one["status"] == DONE
        call = lambda r: host(payload, ops, order, totals, qkeys, r, limit, max_scan)
        hits, unparsed, last, first, calls = C.chain(call, row, qkeys, limit, max_scan, n // min(limit, max_scan) + 2)
        assert hits == one_hits and unparsed == one["unparsed"], (i, queries[i])
        assert last["next_pos"] == one["next_pos"] and last["seen"] == one["seen"] and first["seek_pos"] == one["seek_pos"]
        longest = max(longest, calls)
    assert longest > 3


def test_every_status_and_their_order():
    items = C.golden_table(C.golden())
    payload, ops, order, totals = C.table_of(items)
    qkeys = b"abXYZ"
    Q = MT.RANGE_QUERY_DTYPE

    def row(**kw):
        r = np.zeros(1, dtype=Q)[0]
        r["seq"], r["lo_len"] = 5, 1
        for k, v in kw.items():
            r[k] = v
        return r

    def status(r, tot=totals, **kw):
        hits, res = host(payload, ops, order, tot, qkeys, r, 4, BIG, **kw)
        want = C.model_range(payload, ops, order, tot, qkeys, r, 4, BIG, op_cap=kw.get("op_cap"))
        assert (hits, res) == want, (r, res, want)
        if res["status"] > MORE_SCAN:
            assert res == dict(seek_pos=0, next_pos=0, unparsed=0, count=0, status=res["status"], seen=0, reserved=0)
        return res["status"]

    assert status(row()) == DONE
    # BAD_QUERY: unknown flags, SEEN without RESUME, extents, RESUME beyond the entries
    bad_queries = [row(flags=8), row(flags=1 << 31), row(flags=SEEN), row(flags=SEEN | HAS_HI), row(lo_off=5, lo_len=1),
                   row(lo_off=6, lo_len=0), row(lo_off=(1 << 64) - 1, lo_len=2), row(lo_len=6),
                   row(flags=HAS_HI, hi_off=4, hi_len=2), row(flags=HAS_HI, hi_off=(1 << 64) - 1, hi_len=0xFFFFFFFF),
                   row(flags=RESUME, pos=11), row(flags=RESUME | SEEN, pos=1 << 63),
                   row(flags=RESUME | HAS_HI, pos=3, hi_off=5, hi_len=1)]
    for r in bad_queries:
        assert status(r) == BAD_QUERY, r
    # what is not needed is not checked: lo with RESUME, hi without HAS_HI; an empty extent at the end is inside
    assert status(row(flags=RESUME, pos=10, lo_off=99, lo_len=99)) == DONE
    assert status(row(hi_off=99, hi_len=99)) == DONE
    assert status(row(lo_off=5, lo_len=0)) == DONE and status(row(flags=RESUME | SEEN, pos=0)) == DONE
    # BAD_SEQ comes before BAD_QUERY, NO_TABLE before both
    assert status(row(seq=M)) == MORE_LIMIT and status(row(seq=M + 1)) == BAD_SEQ
    assert status(row(seq=M + 1, flags=8)) == BAD_SEQ and status(row(seq=(1 << 64) - 1, lo_len=6)) == BAD_SEQ
    for tot, kw in ((dict(totals, status=4), {}), (dict(totals, status=1 << 40), {}), (dict(totals, entries=11), {}),
                    (totals, dict(op_cap=9))):
        for r in (row(), row(seq=M + 1), row(flags=8), row(seq=M + 1, flags=SEEN)):
            assert status(r, tot, **kw) == NO_TABLE
    # n != 0 with null ops / order
    L, tot = MT._bind(), MT.Totals(10, 5, 0)
    hits = np.full(4, C.CANARY32, dtype=np.uint32)
    res = np.zeros(1, dtype=MT.RANGE_RESULT_DTYPE)
    q = np.ascontiguousarray(np.asarray(row()).reshape(1))
    pb, kb = ctypes.create_string_buffer(payload), ctypes.create_string_buffer(qkeys)
    for ops_p, order_p in ((None, order.ctypes.data), (ops.ctypes.data, None), (None, None)):
        assert L.lv_memtable_range_host(pb, len(payload), ops_p, order_p, ctypes.byref(tot), 10, kb, 5, q.ctypes.data, 4,
                                        BIG, hits.ctypes.data, res.ctypes.data) == 0
        assert int(res[0]["status"]) == NO_TABLE and (hits == C.CANARY32).all()
    # the empty table needs neither
    empty = MT.Totals(0, 0, 0)
    assert L.lv_memtable_range_host(None, 0, None, None, ctypes.byref(empty), 0, kb, 5, q.ctypes.data, 4, BIG,
                                    hits.ctypes.data, res.ctypes.data) == 0
    assert {f: int(res[0][f]) for f in C.FIELDS} == dict(seek_pos=0, next_pos=0, unparsed=0, count=0, status=DONE, seen=0,
                                                        reserved=0)


def test_damaged_walks_are_no_table():
    """An order index >= op_cap or a key extent outside the payload that the
    walk meets: NO_TABLE with count 0, the predecessor of the first entry
    included; a walk that ends before it is answered."""
    dam, _ = C.damaged_cases()
    for name, broken in (("damaged_order_index", (17, 90)), ("damaged_key_extent", (30, 75, 100))):
        payload, ops, order, totals, cap = dam[name]
        qs = [("resume", p, 0, None, M) for p in (0, broken[0] - 2, broken[0], broken[0] + 1, broken[0] + 2, 110)]
        qkeys, rows = C.pack(qs)
        for limit, max_scan in ((512, BIG), (512, 2), (1, BIG)):
            got = []
            for row in rows:
                want = C.model_range(payload, ops, order, totals, qkeys, row, limit, max_scan, broken=broken)
                slot, r = MT.range_host(payload, ops, order, totals, qkeys, row, limit, max_scan, canary=C.CANARY32)
                assert (slot[: r["count"]].tolist(), r) == want, (name, row, r, want)
                got.append(r["status"])
            assert NO_TABLE in got and got[-1] != NO_TABLE, (name, limit, max_scan, got)


def test_refused_arguments_host():
    L = MT._bind()
    tot = MT.Totals(0, 0, 0)
    q = np.zeros(1, dtype=MT.RANGE_QUERY_DTYPE)
    hits = np.zeros(4, dtype=np.uint32)
    res = np.zeros(1, dtype=MT.RANGE_RESULT_DTYPE)
    t, qp, hp, rp = ctypes.byref(tot), q.ctypes.data, hits.ctypes.data, res.ctypes.data
    buf = ctypes.create_string_buffer(8)
    call = L.lv_memtable_range_host
    assert call(None, 0, None, None, t, 0, None, 0, qp, 4, 1, hp, rp) == 0
    for args in ((None, 0, None, None, None, 0, None, 0, qp, 4, 1, hp, rp),   # null totals
                 (None, 0, None, None, t, 0, None, 0, None, 4, 1, hp, rp),    # null query
                 (None, 0, None, None, t, 0, None, 0, qp, 4, 1, None, rp),    # null hits
                 (None, 0, None, None, t, 0, None, 0, qp, 4, 1, hp, None),    # null result
                 (None, 8, None, None, t, 0, None, 0, qp, 4, 1, hp, rp),      # null payload with bytes
                 (buf, 8, None, None, t, 0, None, 8, qp, 4, 1, hp, rp),       # null qkeys with bytes
                 (None, 0, None, None, t, 0, None, 0, qp, 0, 1, hp, rp),      # limit 0
                 (None, 0, None, None, t, 0, None, 0, qp, 4, 0, hp, rp)):     # max_scan 0
        assert call(*args) == -1, args


def test_refused_arguments_device():
    """LV_ERR_INVALID before any device call, for each refused argument (the
    pointers are never dereferenced: every call fails its checks first)."""
    L = MT._bind()
    vp = ctypes.c_void_p
    P, O, R, T, K, Q, H, S = (0x10000 * (i + 1) for i in range(8))  # far apart: nothing overlaps
    good = dict(payload=vp(P), payload_bytes=64, ops=vp(O), order=vp(R), totals=vp(T), op_cap=8, qkeys=vp(K),
                qkeys_bytes=64, queries=vp(Q), nq=4, limit=4, max_scan=10, hits=vp(H), results=vp(S), flags=0, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return L.lv_memtable_range_device(*(a[k] for k in good)), lvgpu.lib().lv_last_error()

    refused = [
        (dict(flags=1), b"flag"), (dict(totals=None), b"d_totals"), (dict(totals=vp(T + 4)), b"8-byte"),
        (dict(payload=None), b"d_payload"), (dict(qkeys=None), b"d_qkeys"), (dict(ops=vp(O + 8)), b"16-byte"),
        (dict(order=vp(R + 2)), b"4-byte"), (dict(ops=None), b"both or neither"), (dict(order=None), b"both or neither"),
        (dict(op_cap=(1 << 32) - 1), b"op_cap"), (dict(limit=0), b"limit"), (dict(max_scan=0), b"max_scan"),
        (dict(nq=(1 << 32) - 1), b"nq"), (dict(nq=1 << 30, limit=1025), b"2^40"),
        (dict(nq=(1 << 32) - 2, limit=(1 << 32) - 1), b"2^40"),
        (dict(queries=None), b"d_queries"), (dict(hits=None), b"d_hits"), (dict(results=None), b"d_results"),
        (dict(queries=vp(Q + 4)), b"8-byte"), (dict(hits=vp(H + 2)), b"4-byte"), (dict(results=vp(S + 4)), b"8-byte"),
        (dict(hits=vp(S - 8)), b"d_hits overlaps d_results"),
        (dict(hits=vp(P + 60)), b"d_hits overlaps d_payload"), (dict(hits=vp(O + 8 * 32 - 4)), b"d_hits overlaps d_ops"),
        (dict(hits=vp(R + 28)), b"d_hits overlaps d_order"), (dict(hits=vp(T + 20)), b"d_hits overlaps d_totals"),
        (dict(hits=vp(K + 60)), b"d_hits overlaps d_qkeys"), (dict(hits=vp(Q + 4 * 48 - 4)), b"d_hits overlaps d_queries"),
        (dict(results=vp(P + 56)), b"d_results overlaps d_payload"),
        (dict(results=vp(O + 8 * 32 - 8)), b"d_results overlaps d_ops"),
        (dict(results=vp(R + 24)), b"d_results overlaps d_order"), (dict(results=vp(T + 16)), b"d_results overlaps d_totals"),
        (dict(results=vp(K + 56)), b"d_results overlaps d_qkeys"),
        (dict(results=vp(Q + 4 * 48 - 8)), b"d_results overlaps d_queries"),
    ]
    for kw, word in refused:
        rc, err = call(**kw)
        assert rc == -1 and word in err, (kw, rc, err)
