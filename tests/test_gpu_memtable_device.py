"""lv_memtable_build_device and lv_memtable_get_device on the GPU against the
Python model (tests/memtable_cases.py): entry counts around the tile and a
ragged merge tree, surplus passes, corner keys, tags, every key alignment,
every status path, the lookups, the whole device chain from
lv_wal_encode_device on, graph capture."""
import numpy as np
import pytest

import lvgpu.memtable as MT
import lvgpu.write_batch as WB
import memtable_cases as C
from memtable_cases import check, make_table, tag

pytestmark = pytest.mark.gpu

T = MT.MT_TILE


def counted_items(n, seed=1):
    """n items, most behind shared prefixes longer than the sort prefix, so
    merges interleave and ties go to the payload."""
    return C.random_items(np.random.default_rng(seed), n, alphabet=3, maxlen=10, shared=0.7, seqs=5)


@pytest.mark.parametrize("n", [0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 5 * T + 3])
def test_entry_counts(gpu, n):
    """op_cap = the count, and four times it: surplus merge passes run and
    exit, and the buffer parity comes from the count, not the capacity."""
    import torch
    payload, ops = make_table(counted_items(n, seed=n))
    check(torch, gpu, payload, ops, tag_=f"n={n}")
    table, _ = check(torch, gpu, payload, ops, op_cap=max(4 * n, 4), tag_=f"n={n}, op_cap 4n")
    assert table.sync_totals()["entries"] == n


def test_corner_keys_in_one_table(gpu):
    import torch
    payload, ops = make_table(C.corner_items())
    table, order = check(torch, gpu, payload, ops, shift=3)
    keys = [C.key_of(payload, ops[i]) for i in order]
    assert keys == sorted(keys) and keys[0] == b"" and len(keys[-1]) == 2  # ends with b"\xffx"


@pytest.mark.parametrize("group", list(C.corner_groups()))
def test_corner_keys_in_pairs(gpu, group):
    """Every ordered pair of a group alone, as a two-entry table (a key with
    itself included: an exact duplicate but for the op index)."""
    import torch
    keys = C.corner_groups()[group]
    for a in keys:
        for b in keys:
            payload, ops = make_table([(a, tag(1), b"x"), (b, tag(1), b"y")])
            check(torch, gpu, payload, ops, tag_=f"{group} {a[:12]!r} {b[:12]!r}")


def test_tags(gpu):
    import torch
    items = C.tag_items()
    payload, ops = make_table(items)
    table, order = check(torch, gpu, payload, ops)
    vers = [items[i][1] >> 8 for i in order if items[i][0] == b"versions"]
    assert vers == [900, 900, 77, 77, 5, 1]
    dups = [i for i in order if items[i][0] == b"dup" and items[i][1] == tag(42)]
    assert dups == sorted(dups, reverse=True) and len(dups) == 3
    tops = [items[i][1] for i in order if items[i][0] == b"top"]
    assert tops == sorted(tops, reverse=True) and tops[0] >> 63 == 1


def test_one_user_key_across_a_tile_edge(gpu):
    """A run of one user key longer than a tile, between other keys: every
    comparison inside it is decided by the tag or the op index."""
    import torch
    rng = np.random.default_rng(8)
    items = [(b"aaa-before-%d" % i, tag(i), b"") for i in range(T // 2)]
    items += [(b"the-one-user-key", tag(int(rng.integers(1, 40)), int(rng.integers(0, 2))), b"v")
              for _ in range(T + T // 2)]
    items += [(b"zzz-after-%d" % i, tag(i), b"") for i in range(T // 3)]
    items = [items[j] for j in rng.permutation(len(items))]
    payload, ops = make_table(items)
    table, _ = check(torch, gpu, payload, ops)
    assert table.sync_totals()["user_keys"] == T // 2 + 1 + T // 3


@pytest.mark.parametrize("a", range(16))
def test_every_key_alignment(gpu, a):
    """The payload shifted by 0-15 bytes with canaries around it: every key,
    the 5,000-byte ones included, starts at every alignment."""
    import torch
    items = C.corner_items() + counted_items(T + 40, seed=a)
    payload, ops = make_table(items, gaps=[(7 * i) % 5 for i in range(len(items))])
    check(torch, gpu, payload, ops, shift=a, tag_=f"shift={a}")


def test_status_paths(gpu):
    import torch
    payload, ops = make_table(counted_items(2 * T + 9, seed=5))
    n, P = len(ops), len(payload)
    # UPSTREAM: no table, entries = 0
    table, _ = C.run_build(torch, gpu, payload, ops, upstream=2)
    assert table.sync_totals(check=False) == dict(entries=0, user_keys=0, status=C.UPSTREAM) and C.untouched(table)
    with pytest.raises(MT.LvError, match="UPSTREAM"):
        table.sync_totals()
    # a zero upstream status changes nothing
    table, _ = C.run_build(torch, gpu, payload, ops, upstream=0)
    C.compare_build(table, payload, ops, "upstream 0")
    # OP_OVER: *d_n_ops = op_cap + 1
    table, _ = C.run_build(torch, gpu, payload, ops, n_ops=n + 1, op_cap=n)
    assert table.sync_totals(check=False) == dict(entries=n + 1, user_keys=0, status=C.OP_OVER) and C.untouched(table)
    # BAD_OP: a key extent one byte past the payload, an offset near 2^64, a value extent
    for at, field, off, ln in ((0, "key", P - 3, 4), (T + 3, "key", (1 << 64) - 4, 8), (n - 1, "key", P + 1, 0),
                               (T - 1, "val", P - 1, 2), (2 * T, "val", (1 << 64) - 1, 0xFFFFFFFF)):
        bad = ops.copy()
        bad[at][field + "_off"], bad[at][field + "_len"] = off, ln
        table, buf = C.run_build(torch, gpu, payload, bad, shift=at % 16)
        t = table.sync_totals(check=False)
        assert t == dict(entries=n, user_keys=0, status=C.BAD_OP) and C.untouched(table), (at, field, t)
    # an empty extent at the very end of the payload is inside it
    ok = ops.copy()
    ok[5]["key_off"], ok[5]["key_len"] = P, 0
    check(torch, gpu, payload, ok, tag_="empty key at the end")


def test_get(gpu):
    import torch
    rng = np.random.default_rng(31)
    extra = [(b"", 0), (b"", C.MAX_SEQUENCE), (b"\x00", 5), (b"\xff" * 20, 5), (b"versions", 76), (b"versions", 0),
             (b"versions", C.MAX_SEQUENCE + 1), (b"dup", 42), (b"dup", 41), (b"top", C.MAX_SEQUENCE), (b"k", 1 << 60)]
    for name, items in (("tags", C.tag_items()), ("corner", C.corner_items()),
                        ("random", C.random_items(rng, T + 100, alphabet=3, maxlen=6, seqs=6))):
        payload, ops = make_table(items)
        table, order = check(torch, gpu, payload, ops, shift=5, tag_=name)
        queries = C.queries_for(payload, ops, extra=extra)
        got = C.check_get(torch, gpu, table, payload, ops, order, queries, name)
        if name == "random":  # not hollow: every searched status occurs
            assert {C.ABSENT, C.FOUND, C.DELETED, C.BAD_SEQ} <= set(got["status"].tolist())


def test_get_rules(gpu):
    """A snapshot below, at and above each version, a DELETION exactly at the
    snapshot, keys before, between and after the entries, longer and shorter
    query keys."""
    import torch
    items = [(b"k", tag(10), b"ten"), (b"k", tag(20, 0), b""), (b"k", tag(30), b"thirty"), (b"m", tag(5), b"five")]
    payload, ops = make_table(items)
    table, order = check(torch, gpu, payload, ops)
    queries = [(b"k", 9), (b"k", 10), (b"k", 19), (b"k", 20), (b"k", 29), (b"k", 30), (b"k", C.MAX_SEQUENCE),
               (b"k", C.MAX_SEQUENCE + 1), (b"j", 30), (b"l", 30), (b"n", 30), (b"k\x00", 30), (b"", 30), (b"m", 4)]
    got = C.check_get(torch, gpu, table, payload, ops, order, queries)
    A, F, D = C.ABSENT, C.FOUND, C.DELETED
    assert got["status"].tolist() == [A, F, F, D, D, F, F, C.BAD_SEQ, A, A, A, A, A, A]
    assert got["op"].tolist()[:7] == [0, 0, 0, 1, 1, 2, 2]
    assert payload[int(got[5]["val_off"]):][:int(got[5]["val_len"])] == b"thirty"


@pytest.mark.parametrize("nq", [0, 1, 1000])
def test_get_query_counts(gpu, nq):
    import torch
    rng = np.random.default_rng(nq)
    items = C.random_items(rng, 300, alphabet=2, maxlen=5, shared=0.0, seqs=4)
    payload, ops = make_table(items)
    table, order = check(torch, gpu, payload, ops)
    queries = [(items[int(rng.integers(300))][0] + (b"" if rng.random() < 0.8 else b"x"), int(rng.integers(0, 6)))
               for _ in range(nq)]
    C.check_get(torch, gpu, table, payload, ops, order, queries, f"nq={nq}")


def test_get_empty_table_bad_query_and_no_table(gpu):
    import torch
    # the empty table
    payload, ops = make_table([])
    table, order = check(torch, gpu, payload, ops)
    got = C.check_get(torch, gpu, table, payload, ops, order, [(b"k", 5), (b"", 0), (b"k", C.MAX_SEQUENCE + 1)])
    assert got["status"].tolist() == [C.ABSENT, C.ABSENT, C.BAD_SEQ]
    # a query extent outside d_qkeys: a status of its own, its neighbours answered
    payload, ops = make_table([(b"key", tag(7), b"value")])
    table, order = check(torch, gpu, payload, ops)
    qk = b"keykey"
    q_off = np.array([0, 4, 7, (1 << 64) - 2, 3, 6], dtype=np.uint64)
    q_len = np.array([3, 3, 0, 4, 3, 0], dtype=np.uint32)
    got = C.run_get(torch, gpu, table, qk, q_off, q_len, np.full(6, 9, dtype=np.uint64))
    assert got["status"].tolist() == [C.FOUND, C.BAD_QUERY, C.BAD_QUERY, C.BAD_QUERY, C.FOUND, C.ABSENT]
    assert all(int(g["val_len"]) == 0 and int(g["op"]) == 0 for g in got[[1, 2, 3, 5]])
    # NO_TABLE after a failed build
    bad = ops.copy()
    bad[0]["key_len"] = 100
    table, _ = C.run_build(torch, gpu, payload, bad)
    got = C.run_get(torch, gpu, table, qk, q_off[:1], q_len[:1], np.full(1, 9, dtype=np.uint64))
    assert table.sync_totals(check=False)["status"] == C.BAD_OP and got["status"].tolist() == [C.NO_TABLE]


def chain_batches():
    """~2,000 ops over ~300 records: single Puts and mixed batches over a small
    key space, so user keys repeat across records."""
    rng = np.random.default_rng(41)
    reps = []
    for i in range(300):
        b = WB_batch(1000 * i)
        for _ in range(1 if i % 3 else int(rng.integers(10, 30))):
            key = b"user:%06d" % int(rng.integers(0, 400))
            if rng.random() < 0.2:
                b.delete(key)
            else:
                b.put(key, b"v" * int(rng.integers(0, 50)))
        reps.append(b.bytes())
    return reps


def WB_batch(seq):
    from write_batch_cases import WriteBatch
    return WriteBatch().set_sequence(seq)


def test_chain_with_no_host_sync(gpu):
    """lv_wal_encode_device -> scan -> decode -> lv_write_batch_decode_device
    -> build -> get on one stream, one synchronisation at the end."""
    import torch
    import lvgpu.wal as LW
    import write_batch_cases as W
    from wal_encode_cases import to_dev
    reps = chain_batches()
    payload, off, ln = W.pack(reps)
    need, frags = LW.encode_size(ln)
    want_ops = W.model(payload, off, ln)[0]
    assert 1500 <= len(want_ops) <= 3500
    order = C.model_order(payload, want_ops)
    queries = C.queries_for(payload, want_ops[:200], extra=[(b"user:9", 5), (b"", 0)])
    qk, q_off, q_len, q_seq = C.pack_queries(queries)
    d_qk, d_off, d_seq = C.dev_bytes(torch, gpu, qk), C.dev_i64(torch, gpu, q_off), C.dev_i64(torch, gpu, q_seq)
    d_len = torch.from_numpy(q_len.view(np.int32).copy()).to(gpu)
    s = torch.cuda.Stream(device=gpu)
    d_pay = to_dev(torch, payload, gpu, 3)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        log_t = LW.encode_device(d_pay, off, ln, stream=s)
        scan = LW.scan_device(log_t, frags + 8, stream=s)
        dec = LW.decode_device(log_t, *scan, scan_cap=frags + 8, stream=s)
        wops = WB.decode_device(dec.payload, dec.rec_off, dec.rec_len, dec.totals[0:1], dec.totals[4:5],
                                rec_cap=frags + 8, stream=s)
        table = MT.build_device(dec.payload, wops.ops_t, wops.totals[1:2], wops.totals[6:7], stream=s,
                                fill=C.CANARY, guard=C.GUARD)
        res = MT.get_device(table, d_qk, d_off, d_len, d_seq, stream=s)
    s.synchronize()
    # the decode lays the records end to end, as pack did: the offsets are the model's
    assert np.array_equal(wops.ops(), want_ops)
    assert table.sync_totals() == dict(entries=len(want_ops), status=0,
                                       user_keys=len({C.key_of(payload, o) for o in want_ops}))
    assert table.order().tolist() == order
    assert C.tail_is_canary(table.order_t, table.op_cap * 4)
    got = MT.results(res, len(queries))
    get = C.model_get_fast(payload, want_ops, order)
    for i, (key, seq) in enumerate(queries):
        want = get(key, seq)
        assert {k: int(got[i][k]) for k in want} == want, (i, key, seq)


def test_chain_upstream_status_propagates(gpu):
    """An op table that did not fit (OP_OVER upstream): the build reports
    UPSTREAM, writes no order, and a get answers NO_TABLE."""
    import torch
    import write_batch_cases as W
    reps = [W.one_put(i, fill=i) for i in range(20)]
    payload, off, ln = W.pack(reps)
    wops, buf = W.run(torch, gpu, payload, off, ln, op_cap=10)
    table = MT.build_device(wops._keep[0], wops.ops_t, wops.totals[1:2], wops.totals[6:7], op_cap=10, fill=C.CANARY,
                            guard=C.GUARD)
    got = C.run_get(torch, gpu, table, b"k", np.zeros(1, np.uint64), np.ones(1, np.uint32), np.ones(1, np.uint64))
    assert table.sync_totals(check=False) == dict(entries=0, user_keys=0, status=C.UPSTREAM)
    assert C.untouched(table) and got["status"].tolist() == [C.NO_TABLE]


def test_graph_capture(gpu):
    """The build and the get captured into one graph after a warm-up call;
    two replays over different tables of the same capacity."""
    import torch
    sets = []
    for seed, n in ((1, 3 * T + 7), (2, T + 1)):
        payload, ops = make_table(counted_items(n, seed=seed))
        order = C.model_order(payload, ops)
        queries = C.queries_for(payload, ops[:60])[:150]
        sets.append((payload, ops, order, queries))
    size = max(len(s[0]) for s in sets)
    cap = max(len(s[1]) for s in sets)
    nq = 150
    qsize = max(len(C.pack_queries(s[3])[0]) for s in sets)
    d_pay = torch.zeros(size, dtype=torch.uint8, device=gpu)
    d_ops = torch.zeros(cap * 32, dtype=torch.uint8, device=gpu)
    d_n = torch.zeros(1, dtype=torch.int64, device=gpu)
    d_qk = torch.zeros(qsize, dtype=torch.uint8, device=gpu)
    d_off = torch.zeros(nq, dtype=torch.int64, device=gpu)
    d_seq = torch.zeros(nq, dtype=torch.int64, device=gpu)
    d_len = torch.zeros(nq, dtype=torch.int32, device=gpu)
    ws = torch.empty(MT.build_workspace_bytes(cap), dtype=torch.uint8, device=gpu)

    def load(k):
        payload, ops, _, queries = sets[k]
        qk, q_off, q_len, q_seq = C.pack_queries(queries)
        assert len(queries) == nq
        d_pay.zero_()
        d_pay[: len(payload)].copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
        d_ops[: len(ops) * 32].copy_(torch.frombuffer(bytearray(ops.tobytes()), dtype=torch.uint8))
        d_n.fill_(len(ops))
        d_qk[: len(qk)].copy_(torch.frombuffer(bytearray(qk), dtype=torch.uint8))
        d_off.copy_(torch.from_numpy(q_off.view(np.int64).copy()))
        d_seq.copy_(torch.from_numpy(q_seq.view(np.int64).copy()))
        d_len.copy_(torch.from_numpy(q_len.view(np.int32).copy()))

    def verify(k, table, res, what):
        payload, ops, order, queries = sets[k]
        fresh = MT.Table(table.payload, table.ops_t, table.op_cap, table.order_t, table.totals, None)
        C.compare_build(fresh, payload, ops, what)
        got = MT.results(res, nq)
        get = C.model_get_fast(payload, ops, order)
        for i, (key, seq) in enumerate(queries):
            want = get(key, seq)
            assert {f: int(got[i][f]) for f in want} == want, (what, i, key, seq)

    load(0)
    warm = MT.build_device(d_pay, d_ops, d_n, op_cap=cap, workspace=ws, fill=C.CANARY, guard=C.GUARD)
    warm_res = MT.get_device(warm, d_qk, d_off, d_len, d_seq)
    verify(0, warm, warm_res, "warm")
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            table = MT.build_device(d_pay, d_ops, d_n, op_cap=cap, workspace=ws, stream=s, fill=C.CANARY,
                                    guard=C.GUARD)
            res = MT.get_device(table, d_qk, d_off, d_len, d_seq, stream=s)
    torch.cuda.synchronize()
    for k in (1, 0):
        load(k)
        table.order_t.view(torch.uint8).fill_(C.CANARY)
        res.fill_(C.CANARY)
        ws.fill_(0x33)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        verify(k, table, res, f"replay of set {k}")
