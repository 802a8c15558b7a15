"""The expected values of test_gpu_positions64.py against the models the
suite already trusts: the sparse table model against sst_build_cases /
sst_bloom_cases byte for byte, the sparse log model against wal_oracle's
Writer block for block, crc32c_combine against the C oracle, rebase against
its inverse, and every decoy against the case it shadows."""
import numpy as np
import pytest

import compact_cases as CC
import memtable_cases as M
import positions64_cases as P
import sst_bloom_cases as B
import sst_build_cases as S
import wal_encode_cases as WE
import wal_oracle as W
import write_batch_cases as WB
from memtable_cases import tag

BLK = W.BLOCK_SIZE


def test_crc32c_combine_is_the_crc_of_the_concatenation():
    rng = np.random.default_rng(4)
    for la, lb in ((0, 0), (0, 5), (5, 0), (1, 1), (7, 64), (1000, 1), (3, 70000), (70000, 33333)):
        a, b = bytes(rng.integers(0, 256, la, dtype=np.uint8)), bytes(rng.integers(0, 256, lb, dtype=np.uint8))
        assert P.crc32c_combine(W.value(a), W.value(b), lb) == W.value(a + b), (la, lb)
        assert P.crc32c_combine(W.extend(123, a), W.value(b), lb) == W.extend(123, a + b), (la, lb)


def test_splitmix_crc_in_chunks():
    """The chunked, threaded extent CRC equals one oracle pass over the same
    bytes, at chunk edges and for an unaligned start."""
    crc = P.splitmix_crc(99, chunk=4096, threads=4)
    for off, n in ((0, 1), (13, 4096), (13, 4097), (5, 8191), (100000, 50001), (7, 0)):
        assert crc(off, n) == W.value(P.splitmix_bytes(off, n, 99)), (off, n)


# ---- the sparse table model ----
STORE = bytes(np.random.default_rng(8).integers(0, 256, size=80000, dtype=np.uint8))
EXT = ("ext", 1234, 70000)


def _sparse_entries(where, n=40):
    """n small entries with the 70,000-byte ext value first, in the middle of
    or last in its block (block_size 4096: the big entry closes its block)."""
    small = [(S.ikey(b"key%04d" % i, tag(100 + i, 0 if i % 9 == 4 else 1)), b"" if i % 9 == 4 else b"v%d" % i * (i % 5))
             for i in range(n)]
    at = {"first": 0, "middle": 3, "last": n - 1}[where]
    key = small[at][0]
    ents = list(small)
    ents[at] = (key[:-8] + tag(7).to_bytes(8, "little"), EXT)
    return ents


def _dense(ents):
    """The same table as (payload, ops, order) for the dense models."""
    items = [(S.user(k), int.from_bytes(k[-8:], "little"), STORE[v[1]:v[1] + v[2]] if isinstance(v, tuple) else v)
             for k, v in ents]
    payload, ops = M.make_table(items)
    return payload, ops, list(range(len(items)))


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("block_size", [4096, 64])
@pytest.mark.parametrize("bloom", [None, 10])
def test_sparse_table_is_the_dense_model(where, block_size, bloom):
    ents = _sparse_entries(where)
    sp = P.model_build_sparse(ents, block_size, 16, bloom, P.bytes_crc(STORE))
    payload, ops, order = _dense(ents)
    if bloom is None:
        image, handles, tot = S.model_build(payload, ops, block_size, 16, order)
        btot = None
    else:
        image, handles, tot, btot = B.model_build(payload, ops, bloom, block_size, 16, order)
    assert any(isinstance(s, tuple) for s in sp.segments) and sp.size == len(image)
    assert sp.flatten(STORE) == image
    assert sp.handles == handles and sp.totals == tot and sp.bloom_totals == btot
    at = 0
    for off, seg in sp.placed():
        assert off == at
        at += P.seg_len(seg)
    # the entries' value positions and blocks are the image's
    plain = S.model_build(payload, ops, block_size, 16, order)[0]  # (the reader expects an empty metaindex)
    ents_read, index, blocks = S.read_table(plain)
    assert [k for k, _, _, _ in sp.entries] == [k for k, _ in ents_read]
    for (k, blk, vo, vl), (_, v) in zip(sp.entries, ents_read):
        assert image[vo:vo + vl] == v and k in [e[0] for e in blocks[blk]]
    assert [k for k, _ in sp.index] == [k for k, _ in index]


@pytest.mark.parametrize("bloom", [None, 10])
def test_sparse_readers_are_the_dense_models(bloom):
    """table(), bloom(), get() and scan_ops() of the sparse model against
    sst_get_cases / sst_bloom_cases / sst_scan_cases over the flattened image."""
    import sst_get_cases as G
    import sst_scan_cases as SC
    ents = _sparse_entries("middle", 120)
    sp = P.model_build_sparse(ents, 256, 4, bloom, P.bytes_crc(STORE))
    image = sp.flatten(STORE)
    table = G.model_open(image)[0]
    assert sp.table() == table
    keys = sorted({S.user(k) for k, _ in ents})
    queries = [(k, s) for k in keys for s in (0, 6, 7, 150, M.MAX_SEQUENCE)]
    queries += [(k + b"x", M.MAX_SEQUENCE) for k in keys] + [(b"", 5), (b"zzz", 5), (b"key", 5)]
    if bloom is None:
        for k, s in queries:
            assert sp.get(k, s) == G.model_get(image, table, k, s), (k, s)
    else:
        bl = B.model_bloom_open(image, table)
        assert sp.bloom() == bl
        wants = [B.model_get(image, table, bl, k, s) for k, s in queries]
        assert [sp.get(k, s, filtered=True) for k, s in queries] == wants
        assert any(w["reserved"] == B.FILTERED for w in wants) and any(w["status"] == G.FOUND for w in wants)
    tot, ops, arena, _ = SC.model_scan(image, table)
    got_ops, size = sp.scan_ops()
    assert got_ops == ops and size == tot["arena_bytes"] == len(arena)


# ---- the sparse log model ----
SEED = 31


def _log_records(dest_length):
    """(offset, length) records: a 5-block record, records that end 0..7 bytes
    before a block end, an empty record, small ones between them."""
    lens, at = [], dest_length % BLK
    if BLK - at < 7:
        at = 0

    def add(n):
        nonlocal at
        lens.append(n)
        left = n
        while True:
            if BLK - at < 7:
                at = 0
            take = min(left, BLK - at - 7)
            at += 7 + take
            left -= take
            if not left:
                return
    add(50)
    add(0)
    add(5 * BLK + 11)
    for k in range(8):
        add(100 + k)
        room = BLK - at
        if room < 7 + k + 1:  # not enough left for a record that ends k bytes short: fill the block first
            add(room + 10)
            room = BLK - at
        add(room - 7 - k)
        assert BLK - at == k
    add(3)
    recs, off = [], 17
    for n in lens:
        recs.append((off, n))
        off += n + 5
    return recs


@pytest.mark.parametrize("dest_length", [0, 5 * BLK + 17, BLK - 3])
def test_sparse_log_is_the_writer(dest_length):
    recs = _log_records(dest_length)
    data = [P.splitmix_bytes(o, n, SEED) for o, n in recs]
    log = WE.oracle_encode(data, dest_length)
    f = P.Fragments([n for _, n in recs], dest_length)
    assert f.size == len(log)
    hdr, typ, ln = P.expected_fragments(recs, dest_length)
    phys = WE.physical_records(log, dest_length)
    assert [(int(a), int(b), int(c)) for a, b, c in zip(hdr, ln, typ)] == phys
    assert {W.FULL, W.FIRST, W.MIDDLE, W.LAST} <= set(typ.tolist()) and 0 in ln.tolist()
    start = dest_length % BLK
    got = b"".join(P.expected_log_block(k, recs, SEED, dest_length) for k in range(f.blocks()))
    assert got == log
    for k in range(f.blocks()):
        lo, hi = max(k * BLK - start, 0), min((k + 1) * BLK - start, len(log))
        assert P.expected_log_block(k, recs, SEED, dest_length, frags=f) == log[lo:hi], k
    if dest_length == 0:  # the reader's record offsets
        import wal_decode_cases as WD
        _, offs, reports = WD.oracle_read(log)[:3]
        assert not reports and list(offs) == f.rec_log_off.tolist()
        offs2, _, info = W.scan_log(log)
        assert offs2 == hdr.tolist() and info == f.info().tolist()


# ---- rebase and the decoys ----
def test_rebase_and_its_inverse():
    case = P.table_case(200)
    base = P.HI - case.cut
    up = P.rebase(case.ops, base)
    assert (up["key_off"] == case.ops["key_off"] + np.uint64(base)).all() and int(up["val_off"].max()) > P.HI
    assert (up["tag"] == case.ops["tag"]).all() and (up["key_len"] == case.ops["key_len"]).all()
    assert (P.unbase(up, base) == case.ops).all()
    off = np.array([0, 5, case.cut], dtype=np.uint64)
    assert P.rebase(off, base).tolist() == [base, base + 5, P.HI] and (P.unbase(P.rebase(off, base), base) == off).all()
    _, _, rows, _, _ = P.range_case(P.table_case(600))
    rr = np.array(rows, dtype=CC.range_dtype())
    up = P.rebase(rr, base)
    assert (up["lo_off"] == rr["lo_off"] + np.uint64(base)).all() and (up["hi_off"] == rr["hi_off"] + np.uint64(base)).all()
    assert (P.unbase(up, base) == rr).all()


def test_table_decoy_differs_in_every_compared_output():
    """The memtable order, the get answers and the table image (plain and
    bloom) of the decoy differ from the real case's; both are well formed."""
    case = P.table_case(2 * 512 + 1)
    assert len(case.ops) == 1025 and len(case.decoy) == len(case.payload)
    order, dorder = M.model_order(case.payload, case.ops), M.model_order(case.decoy, case.ops)
    assert order != dorder and sorted(order) == sorted(dorder)
    assert M.model_totals(case.payload, case.ops)[1]["user_keys"] < len(case.ops)  # versions and a duplicate
    image = S.model_build(case.payload, case.ops, 1024, 16)[0]
    dimage = S.model_build(case.decoy, case.ops, 1024, 16)[0]
    assert image != dimage and S.read_table(dimage)[0]
    assert B.model_build(case.payload, case.ops, 10, 1024, 16)[0] != B.model_build(case.decoy, case.ops, 10, 1024, 16)[0]
    get, dget = M.model_get_fast(case.payload, case.ops, order), M.model_get_fast(case.decoy, case.ops, dorder)
    queries = M.queries_for(case.payload, case.ops)[::7]
    a, b = [get(k, s) for k, s in queries], [dget(k, s) for k, s in queries]
    assert a != b and any(r["status"] == M.FOUND for r in a)
    # the query window's decoy: other keys, other answers
    c = [get(P.complement(k), s) for k, s in queries]
    assert a != c
    # suffixes and values on both sides of the wave-copy threshold
    assert (case.ops["val_len"] >= 64).any() and (case.ops["val_len"] < 64).any() and (case.ops["key_len"] >= 80).any()


def test_compact_decoy_differs():
    case = P.table_case(1025)
    payload, ops = case.payload, case.ops
    order = np.array(M.model_order(payload, ops), dtype=np.uint32)
    mt = M.model_totals(payload, ops)[1]
    ranges, window, rows, decoy, cut = P.range_case(case)
    assert 0 < cut < len(window) and len(decoy) == len(window)
    rr = np.array(rows, dtype=CC.range_dtype())
    snap = 14
    want = CC.model_filter(payload, ops, order, mt, snap, (rr, window), CC.BASE_LEVEL)
    none = CC.model_filter(payload, ops, order, mt, snap, None, CC.BASE_LEVEL)
    dec = CC.model_filter(payload, ops, order, mt, snap, (rr, decoy), CC.BASE_LEVEL)
    assert want[0]["status"] == dec[0]["status"] == 0
    assert want[0]["dropped_deletions"] > 0 and want[0]["dropped_hidden"] > 0
    assert want[0]["dropped_deletions"] < none[0]["dropped_deletions"]  # the ranges decide some deletions
    assert want[2] != dec[2] and want[0] != dec[0]
    dorder = np.array(M.model_order(case.decoy, ops), dtype=np.uint32)
    assert CC.model_filter(case.decoy, ops, dorder, mt, snap, (rr, window), CC.BASE_LEVEL)[2] != want[2]


def test_batch_decoy_differs():
    window, off, ln, decoy, cut = P.batch_case(3 * 256 + 5)
    assert len(window) == len(decoy) and 0 < cut < len(window)
    a, b = WB.model(window, off, ln), WB.model(decoy, off, ln)
    assert a[3]["bad_records"] == b[3]["bad_records"] == 1 and a[3]["status"] == 0
    assert (a[2] != b[2]).sum() == 2 and a[3] != b[3]
    assert len(a[0]) != len(b[0]) or (a[0]["tag"] != b[0]["tag"]).any()
    below, across, above = P.sides(off, ln, cut)
    assert below and across == 1 and above


def test_hash_decoy_differs():
    import ctypes
    L = W.lib()
    L.oracle_hash_batch.restype = None
    L.oracle_hash_batch.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t]
    window, off, ln, decoy, cut = P.hash_case()
    out = []
    for w in (window, decoy):
        a = np.frombuffer(w, dtype=np.uint8).copy()
        h = np.zeros(len(off), dtype=np.uint32)
        L.oracle_hash_batch(a.ctypes.data, off.ctypes.data, ln.ctypes.data, None, h.ctypes.data, len(off))
        out.append(h)
    assert ((out[0] != out[1]) | (ln == 0)).all()
    assert all(P.sides(off, ln, cut))
