"""lv_write_batch_decode_device on the GPU against the Python model
(tests/write_batch_cases.py): record counts around the scan tile, the edge
between the lane and the wave class, the wave class's window edges, corner
ops, every status on both classes, capacities, the whole device chain from
lv_wal_encode_device on, unordered and overlapping records, graph capture."""
import numpy as np
import pytest

import lvgpu.write_batch as WB
import write_batch_cases as C
from write_batch_cases import WriteBatch, check, hdr, one_put, pack

pytestmark = pytest.mark.gpu

T, SMALL, WINDOW, ROUND = WB.WB_TILE, WB.WB_SMALL, WB.WB_WINDOW, WB.WB_ROUND


def raw_batch(seq, body, count=None):
    """hdr + body with the count the body's entries make (or a given one)."""
    if count is None:
        st, ops, _, _ = C.iterate_ext(hdr(seq, 0) + body)
        assert st in (C.OK, C.WRONG_COUNT), st
        count = len(ops)
    return hdr(seq, count) + body


def filler(n):
    """n bytes of 2- and 3-byte DELETION entries: the parser reads every one
    of their headers, so the wave class's windows follow each other."""
    assert n == 0 or n >= 2, n
    out = bytearray()
    while n:
        if n == 3 or (n > 4 and len(out) % 7 == 0):
            out += bytes([C.DELETION, 1, 0x6B])
            n -= 3
        else:
            out += bytes([C.DELETION, 0])
            n -= 2
    return bytes(out)


def sized_record(total, seq=7):
    """One Put of a 16-byte key whose value makes the rep `total` bytes."""
    for vlen in range(total):
        rep = WriteBatch().set_sequence(seq).put(b"k" * 16, b"v" * vlen).bytes()
        if len(rep) == total:
            return rep
    raise AssertionError(total)


def aligned_pack(reps, a):
    """pack with every record's offset = a (mod 16)."""
    payload, off = bytearray(), []
    for r in reps:
        payload += b"\xEE" * ((a - len(payload)) % 16)
        off.append(len(payload))
        payload += r
    return bytes(payload), np.array(off, dtype=np.uint64), np.array([len(r) for r in reps], dtype=np.uint64)


@pytest.mark.parametrize("n", [0, 1, 2, T - 1, T, T + 1, 3 * T + 5])
def test_record_counts(gpu, n):
    """One-op records with a larger record planted at each tile edge, so the
    scan's carry is not all ones."""
    import torch
    reps = [one_put(10 * i, fill=i) for i in range(n)]
    for edge in range(T - 1, n, T):
        for i in (edge, edge + 1):
            if i < n:
                reps[i] = C.mixed_batch(5 + i % 3, seed=i, seq=i).bytes()
    ops, want = check(torch, gpu, *pack(reps), tag=f"n={n}")
    assert want[3]["records"] == n and want[3]["bad_records"] == 0
    if n > T:
        assert want[1][T] != T  # the carry into the second tile is not the record index


@pytest.mark.parametrize("a", range(16))
def test_class_edge(gpu, a):
    """Records of WB_SMALL - 1, WB_SMALL and WB_SMALL + 1 bytes as neighbours,
    starting at every alignment."""
    import torch
    sizes = [SMALL - 1, SMALL, SMALL + 1, SMALL, SMALL + 1, SMALL - 1, SMALL + 1]
    reps = [sized_record(s, seq=100 * i) for i, s in enumerate(sizes)]
    assert [len(r) for r in reps] == sizes
    check(torch, gpu, *pack(reps), shift=a, tag=f"shift={a}")


def window_edge_records(a):
    """Wave-class records that start at alignment a, with an entry's tag, a
    two-byte varint, the end of a key and a five-byte varint at the last bytes
    before the end of the first round and of the first window.  The window
    opens at the aligned granule under the record's first byte, so its end is
    at record offset E - a."""
    tail = bytes([C.VALUE, 4]) + b"tail" + bytes([1]) + b"x" + bytes([C.DELETION, 2]) + b"zz"
    # a last Put whose (skipped) value makes the record longer than WB_SMALL: the wave class
    tail += bytes([C.VALUE, 3]) + b"pad" + C.varint(SMALL) + bytes(SMALL)
    key130 = bytes(range(130))
    reps = []
    for E in (ROUND, WINDOW):
        for d in range(7):
            q = E - a - d  # record offset of the byte under test
            # an entry whose tag falls there
            reps.append(raw_batch(q, filler(q - 12) + tail))
            # a two-byte varint at q, q + 1 (its tag at q - 1)
            reps.append(raw_batch(q + 1, filler(q - 13) + bytes([C.VALUE, 0x82, 0x01]) + key130 + bytes([0]) + tail))
            # a key that ends exactly there: the next tag is at q
            reps.append(raw_batch(q + 2, filler(q - 19) + bytes([C.DELETION, 5]) + b"abcde" + tail))
            # a five-byte varint (of 3) at q - 2 .. q + 2
            reps.append(raw_batch(q + 3, filler(q - 15) + bytes([C.DELETION, 0x83, 0x80, 0x80, 0x80, 0x00]) + b"xyz"
                                  + tail))
    return reps


@pytest.mark.parametrize("a", range(16))
def test_window_edges(gpu, a):
    import torch
    reps = window_edge_records(a)
    assert all(len(r) > SMALL for r in reps)
    payload, off, ln = aligned_pack(reps, a)
    assert all(int(o) % 16 == a for o in off)
    ops, want = check(torch, gpu, payload, off, ln, tag=f"a={a}")
    assert want[3]["bad_records"] == 0


def test_skip_and_flush(gpu):
    """A value of 3 * WB_WINDOW + 1 bytes followed by more entries (the skip),
    and 64 k +- 1 ops in one record (the staged store's flush)."""
    import torch
    big = WriteBatch().set_sequence(5).put(b"before", b"b").put(b"K" * 20, b"V" * (3 * WINDOW + 1))
    big.put(b"after", b"a" * 10).delete(b"gone").put(b"k" * (WINDOW + 3), b"").put(b"end", b"e")
    big.put(b"pad", bytes(SMALL))
    reps = [big.bytes()]
    for nops in (63, 64, 65, 127, 128, 129, 1, 2):
        b = WriteBatch().set_sequence(1000 * nops)
        for i in range(nops - 1):
            b.put(bytes([i & 0xFF]) * 3, b"vv") if i % 3 else b.delete(b"ddd")
        b.put(b"pad", bytes(SMALL))  # the last of the nops ops; its value makes the record wave class
        reps.append(b.bytes())
    assert all(len(r) > SMALL for r in reps)
    ops, want = check(torch, gpu, *pack(reps, gaps=[3] * len(reps)))
    assert want[3]["bad_records"] == 0


def just_wave_class(nops, seed, seq, bad=False):
    """A record of WB_SMALL + 1 bytes with nops small ops: the wave class by one
    byte.  A last Put's (skipped) value makes up the length; with bad, an entry
    whose key length runs past the record stands in its place (BAD_LENGTH after
    nops ops), then zeros."""
    head = C.mixed_batch(nops, seed=seed, seq=seq, maxlen=12).bytes()
    if bad:
        rep = hdr(seq, nops + 1) + head[12:] + bytes([C.VALUE]) + C.varint(0xFFFFFFFF)
        return rep + bytes(SMALL + 1 - len(rep))
    for vbytes in (2, 3):  # of the value's length varint
        vlen = SMALL + 1 - len(head) - 5 - vbytes  # tag, key length, "pad"
        if len(C.varint(vlen)) == vbytes:
            return C.mixed_batch(nops, seed=seed, seq=seq, maxlen=12).put(b"pad", bytes(vlen)).bytes()
    raise AssertionError(len(head))


def test_wave_dispatch(gpu):
    """One wave's 64 records with the wave class at lanes 0, 1, 31 and 63 among
    lane-class records of a few ops, record 31 failing after its 65th op; then
    the rest of the tile, and a second tile whose only record is wave class: a
    wave with one large record and 63 absent ones.  Every large record has
    more than 64 ops, so the staged store flushes; each lane must keep its own
    walk's result and lane b the wave's."""
    import torch
    reps = [C.mixed_batch(1 + i % 4, seed=i, seq=50 * i, maxlen=10).bytes() for i in range(T)]
    for k, i in enumerate((0, 1, 63)):
        reps[i] = just_wave_class(66 + 3 * k, seed=100 + i, seq=7000 * (k + 1))
    reps[31] = just_wave_class(65, seed=131, seq=31000, bad=True)
    reps.append(just_wave_class(70, seed=200, seq=90000))
    assert len(reps) == T + 1 and [i for i, r in enumerate(reps) if len(r) > SMALL] == [0, 1, 31, 63, T]
    assert all(len(reps[i]) == SMALL + 1 for i in (0, 1, 31, 63, T))
    ops, want = check(torch, gpu, *pack(reps, gaps=[i % 3 for i in range(len(reps))]), shift=3)
    st = want[2].tolist()
    assert st[31] == C.BAD_LENGTH and st.count(C.OK) == T and want[3]["bad_records"] == 1
    counts = np.diff(want[1]).tolist()
    assert counts[31] == 65 and [counts[i] for i in (0, 1, 63, T)] == [67, 70, 73, 71]


def test_corner_ops(gpu):
    """Empty keys and values, a 12-byte record with count 0, and records of
    2-byte deletes only, where ops == (len - 12) / 2: the capacity bound."""
    import torch
    empty = WriteBatch().set_sequence(3).put(b"", b"").delete(b"").put(b"", b"v").put(b"k", b"").bytes()
    reps = [empty, hdr(9, 0), one_put(1)]
    for k in (1, 50, SMALL):  # the last is 2 * WB_SMALL + 12 bytes: the wave class
        reps.append(hdr(77, k) + bytes([C.DELETION, 0]) * k)
    ops, want = check(torch, gpu, *pack(reps))
    assert want[3]["bad_records"] == 0 and want[3]["key_bytes"] == 1 + 16
    assert want[1].tolist()[-3:] == [6, 56, 56 + SMALL]
    # op_cap = payload_bytes // 2 never overflows on delete-only records
    for k in (50, SMALL):
        rep = hdr(1, k) + bytes([C.DELETION, 0]) * k
        ops, want = check(torch, gpu, *pack([rep]), op_cap=len(rep) // 2, tag=f"deletes {k}")
        assert want[3]["ops"] == k == (len(rep) - 12) // 2
        # ... and not even when the records are nothing but such entries
        body = bytes([C.DELETION, 0]) * k
        payload = body * 4
        off = np.array([0, 2 * k], dtype=np.uint64)
        ln = np.array([2 * k, 2 * k], dtype=np.uint64)
        ops, _ = check(torch, gpu, payload, off, ln, op_cap=len(payload) // 2, tag="headerless")
        assert ops.sync_totals()["status"] == 0


def wave_variant(rep):
    """The same ending behind enough good entries to make the record wave class."""
    if len(rep) < 12:
        return None
    nfill = (SMALL + 40) // 2
    seq = int.from_bytes(rep[:8], "little")
    count = int.from_bytes(rep[8:12], "little")
    return hdr(seq, count + nfill) + bytes([C.DELETION, 0]) * nfill + rep[12:]


STATUS = list(C.status_cases())


def test_every_status_with_good_neighbours(gpu):
    """Every status on both classes in one call; the neighbours of a bad
    record decode normally."""
    import torch
    reps, want_st = [], []
    for i, (name, rep, status, nops) in enumerate(STATUS):
        for r in (rep, wave_variant(rep)):
            if r is None:
                continue
            reps += [r, one_put(i, fill=i)]
            want_st += [status, C.OK]
    ops, want = check(torch, gpu, *pack(reps, gaps=[i % 5 for i in range(len(reps))]))
    assert want[2].tolist() == want_st
    assert set(want_st) == {C.OK, C.TOO_SMALL, C.BAD_VARINT, C.BAD_LENGTH, C.WRONG_COUNT, C.BAD_TAG}


@pytest.mark.parametrize("name", [c[0] for c in STATUS])
def test_status_at_the_end_of_the_payload(gpu, name):
    """The failing entry as the last bytes of the payload, on both classes: a
    walk that read past its record would take the canaries behind it for
    entries."""
    import torch
    _, rep, status, nops = next(c for c in STATUS if c[0] == name)
    for r in (rep, wave_variant(rep)):
        if r is None:
            continue
        payload, off, ln = pack([one_put(1), r])
        ops, want = check(torch, gpu, payload, off, ln, shift=(5 + len(payload)) % 16, tag=name)
        assert want[2].tolist() == [C.OK, status]


def test_out_of_range(gpu):
    import torch
    good = [one_put(1), C.wave_batch(SMALL), one_put(2)]
    payload, off, ln = pack(good)
    P = len(payload)
    off = off.tolist() + [P - 20, (1 << 64) - 8, P + 1, P, int(off[1])]
    ln = ln.tolist() + [21, 16, 0, 0, (1 << 64) - 1]
    off, ln = np.array(off, dtype=np.uint64), np.array(ln, dtype=np.uint64)
    ops, want = check(torch, gpu, payload, off, ln)
    assert want[2].tolist() == [0, 0, 0, C.OUT_OF_RANGE, C.OUT_OF_RANGE, C.OUT_OF_RANGE, C.TOO_SMALL, C.OUT_OF_RANGE]


def test_capacities(gpu):
    import torch
    reps = [one_put(i) for i in range(40)] + [C.wave_batch(SMALL), C.mixed_batch(30, maxlen=60).bytes()]
    payload, off, ln = pack(reps)
    want = C.model(payload, off, ln)
    k = want[3]["ops"]
    # op_cap = ops - 1: OP_OVER, the true totals, the arrays untouched
    ops, _ = C.run(torch, gpu, payload, off, ln, op_cap=k - 1)
    t = ops.sync_totals(check=False)
    assert t == dict(want[3], status=C.OP_OVER) and C.untouched(ops)
    with pytest.raises(WB.LvError, match="OP_OVER"):
        ops.sync_totals()
    # op_cap = ops: fits
    ops, _ = C.run(torch, gpu, payload, off, ln, op_cap=k)
    C.compare(ops, want, "exact op_cap")
    # *d_records = rec_cap + 1: REC_OVER, nothing decoded
    ops, _ = C.run(torch, gpu, payload, off, ln, records=len(reps) + 1, rec_cap=len(reps))
    t = ops.sync_totals(check=False)
    assert t == dict(records=len(reps) + 1, ops=0, key_bytes=0, value_bytes=0, bad_records=0, last_sequence=0,
                     status=C.REC_OVER) and C.untouched(ops)
    # *d_upstream_status = 2: UPSTREAM with zero records
    ops, _ = C.run(torch, gpu, payload, off, ln, upstream=2)
    t = ops.sync_totals(check=False)
    assert t == dict(records=0, ops=0, key_bytes=0, value_bytes=0, bad_records=0, last_sequence=0,
                     status=C.UPSTREAM) and C.untouched(ops)
    # a zero upstream status changes nothing
    ops, _ = C.run(torch, gpu, payload, off, ln, upstream=0)
    C.compare(ops, want, "upstream 0")


def chain_batches():
    rng = np.random.default_rng(41)
    reps = []
    for i in range(300):
        if i % 10 == 3:
            reps.append(C.mixed_batch(int(rng.integers(2, 40)), seed=i, seq=1000 * i).bytes())
        else:
            reps.append(one_put(1000 * i, fill=i))
    big = WriteBatch().set_sequence(7777).put(b"bigkey", bytes(40000)).put(b"after", b"big")
    reps.insert(150, big.bytes())
    return reps


def _chain(torch, gpu, s, log_t, scan_cap, rec_cap=None):
    """scan -> decode -> op table on stream s; d_records / d_upstream_status
    point into the decode's totals."""
    import lvgpu.wal as LW
    scan = LW.scan_device(log_t, scan_cap, stream=s)
    dec = LW.decode_device(log_t, *scan, scan_cap=scan_cap, stream=s, rec_cap=rec_cap)
    ops = WB.decode_device(dec.payload, dec.rec_off, dec.rec_len, dec.totals[0:1], dec.totals[4:5],
                           rec_cap=scan_cap if rec_cap is None else rec_cap, stream=s, fill=C.CANARY, guard=C.GUARD)
    return dec, ops


def test_chain_with_no_host_sync(gpu):
    """lv_wal_encode_device -> lv_wal_scan_device -> lv_wal_decode_device ->
    lv_write_batch_decode_device on one stream, nothing read back until the end."""
    import torch
    import lvgpu.wal as LW
    from wal_encode_cases import to_dev
    reps = chain_batches()
    payload, off, ln = pack(reps)
    need, frags = LW.encode_size(ln)
    assert need > 3 * 32768 and max(len(r) for r in reps) > 32768
    s = torch.cuda.Stream(device=gpu)
    d_pay = to_dev(torch, payload, gpu, 3)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        log_t = LW.encode_device(d_pay, off, ln, stream=s)
        dec, ops = _chain(torch, gpu, s, log_t, frags + 8)
    s.synchronize()
    want = C.model(payload, off, ln)
    C.compare(ops, want, "chain")
    assert want[3]["records"] == len(reps) and want[3]["bad_records"] == 0
    assert want[3]["last_sequence"] == 1000 * 299


def test_chain_with_a_flipped_byte_and_a_short_decode(gpu):
    """The same log with one flipped byte: the Reader drops records and
    everything after them shifts.  And a decode whose rec_cap is too small: its
    status propagates as UPSTREAM."""
    import torch
    from wal_decode_cases import oracle_read
    from wal_encode_cases import oracle_encode, to_dev
    reps = chain_batches()
    log = bytearray(oracle_encode(reps))
    log[32768 + 2000] ^= 0x40
    log = bytes(log)
    recs = oracle_read(log)[0]
    assert 0 < len(recs) < len(reps)
    s = torch.cuda.Stream(device=gpu)
    log_t = to_dev(torch, log, gpu, 0)
    cap = len(reps) + 40
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dec, ops = _chain(torch, gpu, s, log_t, cap)
        dec2, ops2 = _chain(torch, gpu, s, log_t, cap, rec_cap=10)
    s.synchronize()
    C.compare(ops, C.model(*pack(recs)), "flipped")
    assert dec.sync_totals()["records"] == len(recs)
    t = ops2.sync_totals(check=False)
    assert t["status"] == C.UPSTREAM and t["records"] == 0 and t["ops"] == 0 and C.untouched(ops2)


def test_unordered_and_overlapping_records(gpu):
    import torch
    reps = [one_put(i) for i in range(70)] + [C.wave_batch(SMALL, seed=i) for i in range(4)]
    payload, off, ln = pack(reps)
    perm = np.random.default_rng(5).permutation(len(reps))
    off, ln = off[perm], ln[perm]
    check(torch, gpu, payload, off, ln, tag="permuted")
    # records sharing bytes: the whole of a batch, its first 200 bytes, itself again, and a
    # 131-byte window into the middle of it
    big = int(np.nonzero(ln > SMALL)[0][0])
    off2 = np.array([off[big], off[big], off[big], off[big] + 40, off[0]], dtype=np.uint64)
    ln2 = np.array([ln[big], 200, ln[big], 131, ln[0]], dtype=np.uint64)
    ops, want = check(torch, gpu, payload, off2, ln2, tag="overlapping")
    assert want[2][0] == want[2][2] == C.OK and want[2][4] == C.OK


def test_graph_capture(gpu):
    """The call can be captured into a graph; two replays over different
    payload contents in the same buffers write what the model says."""
    import torch
    sets = [pack([one_put(i) for i in range(50)] + [C.wave_batch(SMALL, nops=40, seed=1)]),
            pack([C.wave_batch(SMALL, nops=25, seed=2)] + [one_put(9 * i, fill=i) for i in range(30)]
                 + [hdr(1, 3) + bytes([C.DELETION, 0])])]
    size = max(len(p) for p, _, _ in sets)
    cap = max(len(o) for _, o, _ in sets)
    d_pay = torch.zeros(size, dtype=torch.uint8, device=gpu)
    d_off = torch.zeros(cap, dtype=torch.int64, device=gpu)
    d_len = torch.zeros(cap, dtype=torch.int64, device=gpu)
    d_n = torch.zeros(1, dtype=torch.int64, device=gpu)
    ws = torch.empty(WB.decode_workspace_bytes(cap), dtype=torch.uint8, device=gpu)

    def load(k):
        p, o, l = sets[k]
        d_pay.zero_()
        d_pay[: len(p)].copy_(torch.frombuffer(bytearray(p), dtype=torch.uint8))
        d_off[: len(o)].copy_(torch.from_numpy(o.view(np.int64).copy()))
        d_len[: len(l)].copy_(torch.from_numpy(l.view(np.int64).copy()))
        d_n.fill_(len(o))

    load(0)
    warm = WB.decode_device(d_pay, d_off, d_len, d_n, rec_cap=cap, workspace=ws, fill=C.CANARY, guard=C.GUARD)
    C.compare(warm, C.model(*sets[0]), "warm")
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ops = WB.decode_device(d_pay, d_off, d_len, d_n, rec_cap=cap, workspace=ws, stream=s, fill=C.CANARY,
                                   guard=C.GUARD)
    torch.cuda.synchronize()
    for k in (1, 0):
        load(k)
        for t in (ops.ops_t, ops.rec_op, ops.rec_status):
            t.view(torch.uint8).fill_(C.CANARY)
        ws.fill_(0x33)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        fresh = WB.Ops(ops.ops_t, ops.op_cap, ops.rec_op, ops.rec_status, ops.totals, None)
        # the payload buffer is `size` bytes in both replays: the model sees the same
        C.compare(fresh, C.model(bytes(sets[k][0]) + bytes(size - len(sets[k][0])), sets[k][1], sets[k][2]),
                  f"replay of set {k}")
