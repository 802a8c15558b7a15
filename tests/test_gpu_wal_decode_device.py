"""lv_wal_decode_device: the WAL Reader replayed in HBM over scan_device's
arrays.  Every case compares the records, each record's rec_log_off, the report
list in order and the totals with oracle/wal_oracle.py's Reader
(ReportCollector, checksum on, initial_offset 0) and with lvgpu.wal.Reader over
Scan.from_arrays of the very arrays the decode was fed."""
import numpy as np
import pytest

import wal_oracle as W
from wal_decode_cases import (B, BIG, CANARY, H, carry_log, check, collect, first_of_type, flip, guards_ok, headers,
                              mixed_log, oracle_read, reason_cases, run_decode, set_type, shape_cases, untouched)
from wal_encode_cases import oracle_encode, pack, random_records, to_dev

pytestmark = pytest.mark.gpu

SHAPES = list(shape_cases())
REASONS = list(reason_cases())


@pytest.mark.parametrize("name", [n for n, _ in SHAPES if not n.startswith(("recipe_edge", "trailer_edge"))])
def test_shapes(gpu, name):
    import torch
    log = dict(SHAPES)[name]
    _, want = check(torch, gpu, log, tag=name)
    assert not want[2]  # nothing wrong with these logs
    if name == "multiple_of_block":
        assert len(log) % B == 0 and len(log) > 0


def test_writer_edges(gpu):
    """The EDGES recipes and the trailer edges of wal_encode_cases.py (among
    them the zero-length FIRST when exactly 7 bytes remain)."""
    import torch
    zero_first = 0
    for name, log in SHAPES:
        if name.startswith(("recipe_edge", "trailer_edge")):
            _, want = check(torch, gpu, log, tag=name)
            assert not want[2], name
            zero_first += any(ln == 0 and t == W.FIRST for _, ln, t in headers(log))
    assert zero_first > 0


@pytest.mark.parametrize("name", [n for n, _, _ in REASONS])
def test_report_reasons(gpu, name):
    import torch
    log, reasons = next((l, r) for n, l, r in REASONS if n == name)
    _, want = check(torch, gpu, log, tag=name)
    got = [r for _, r in want[2]]
    assert (set(reasons) <= set(got)) if reasons else not got, want[2]


def test_every_reason_is_covered():
    """(No GPU work: the cases above name all nine reasons between them.)"""
    import lvgpu.wal as LW
    seen = set()
    for _, log, _ in REASONS:
        seen |= {r for _, r in oracle_read(bytes(log))[2]}
    assert seen == set(LW.DROP_REASONS.values())


def test_mismatch_drops_rest_of_block(gpu):
    """A mismatch in the first record of a block: the good records after it in
    that block are dropped, and the next block resumes."""
    import torch
    log = next(l for n, l, _ in REASONS if n == "mismatch_first_of_block")
    whole = oracle_read(oracle_encode([b"x" * 200] * 400))[0]
    r, want = check(torch, gpu, log)
    in_block = sum(1 for p, _, t in headers(oracle_encode([b"x" * 200] * 400)) if B <= p < 2 * B)
    assert 100 < in_block and len(want[0]) <= len(whole) - in_block + 2
    assert want[1][-1] > 2 * B  # records of the third block are back


# ---- scan carries ----
def test_carry(gpu):
    import torch
    r, want = check(torch, gpu, carry_log())
    assert len(want[0]) == 10001 and len(want[0][5000]) == 70000


def _sweep():
    import lvgpu.wal as LW
    ps = set(range(0, 41)) | set(range(40, 4201, 97))
    # the big record's FIRST is entry p + 5000 + (blocks' worth of shift): also aim at the tile edges
    T = LW.DECODE_TILE
    for m in range(5, 10):
        ps |= {m * T - 5000 + d for d in range(-5, 4) if 0 <= m * T - 5000 + d <= 4200}
    return sorted(ps)


def test_carry_sweep(gpu):
    """p extra one-byte records in front: the FIRST / MIDDLE / LAST triple moves
    across every boundary of the scan's tiles (and +-3 around their multiples)."""
    import torch
    import lvgpu.wal as LW
    T = LW.DECODE_TILE
    crossed = set()
    for p in _sweep():
        log = carry_log(p)
        i = p + 5000  # the FIRST's entry: every one-byte record before it is one entry of 8 bytes
        assert log[8 * i + 6] == W.FIRST
        crossed.add((i % T, (i + 1) % T, (i + 2) % T))
        entries = len(headers(log))  # BIG makes three fragments, or four when its FIRST is a short one
        assert entries in (p + 10003, p + 10004), p
        r = collect(torch, run_decode(torch, gpu, log, cap=entries + 2))
        assert r.count == entries, p
        got = r.dec.records()
        assert len(got) == p + 10001, p
        assert got[p + 5000] == BIG, p
        assert got[: p + 5000] == [b"a"] * (p + 5000) and got[p + 5001:] == [b"z"] * 5000, p
        assert r.dec.reports() == [] and r.dec.record_log_offsets()[p + 5000] == 8 * i, p
        assert guards_ok(r, r.dec.sync_totals()["payload_bytes"]), p
    # the triple straddled a tile edge at each of its two joints, and lay wholly on either side
    firsts = {c[0] for c in crossed}
    assert {T - 1, T - 2, 0, T - 3} <= firsts, sorted(firsts)[:8]


def test_carry_with_mismatch_in_middle(gpu):
    import torch
    for p in (0, 23, 24 + 97):
        log = bytearray(carry_log(p))
        flip(log, first_of_type(log, W.MIDDLE) + H + 9)
        _, want = check(torch, gpu, log, tag=p)
        assert [r for _, r in want[2]][:2] == ["checksum mismatch", "error in middle of record"]


def test_second_round_of_tile_scan(gpu):
    """More scan tiles than one workgroup has threads: wal_dec_tiles goes round
    twice.  256 tiles of one-byte records, then 1,025 more; a FIRST / MIDDLE /
    LAST triple of them lies astride the round boundary (its FIRST is the last
    entry of the first round, so the open record is carried into the second and
    the FIRST learns of its LAST from there), and a checksum mismatch follows
    in the second round."""
    import torch
    import lvgpu.wal as LW
    R = 256 * LW.DECODE_TILE  # entries of one round
    assert R == 262144
    log = bytearray(oracle_encode([b"a"]) * (R + 1025))  # entry i is the 8 bytes at 8 i
    for i, t in ((R - 1, W.FIRST), (R, W.MIDDLE), (R + 1, W.LAST)):
        set_type(log, 8 * i, t)
    flip(log, 8 * (R + 500) + H)
    r, want = check(torch, gpu, log)
    assert r.count == R + 1025
    assert len(want[0]) == R + 500 - 2 and want[0][R - 1] == b"aaa" and want[1][R - 1] == 8 * (R - 1)
    assert [x for _, x in want[2]] == ["checksum mismatch"]


def test_more_blocks_than_compute_units(gpu):
    """More log blocks than wal_unframe_kernel has workgroups: sized from the
    launcher's cap (tests/loop_trips.py), so every workgroup takes a second
    block whatever the cap becomes."""
    import torch
    import loop_trips as LT
    cus = LT.device_cus(gpu)
    nb = max(LT.size_for("wal_unframe_kernel", 2, cus, 5), 600)
    log = mixed_log(nb)
    assert len(log) >= nb * B
    assert LT.trips("wal_unframe_kernel", -(-len(log) // B), cus) >= 2
    check(torch, gpu, log, pay_shift=9)


def test_alignment(gpu):
    """d_payload at each of the 16 byte alignments, canaries on both sides."""
    import torch
    rng = np.random.default_rng(31)
    recs = random_records(rng, 36, maxlog=13) + [rng.integers(0, 256, size=2 * B + 100, dtype=np.uint8).tobytes(), b"",
                                                 b"abc", rng.integers(0, 256, size=9000, dtype=np.uint8).tobytes(), b"q"]
    log = oracle_encode(recs)
    for s in range(16):
        r, want = check(torch, gpu, log, pay_shift=s, tag=s)
        assert want[0] == recs
    # a span shorter than a granule, at every alignment
    for s in range(16):
        check(torch, gpu, oracle_encode([b"abcde"]), pay_shift=s, tag=("short", s))


# ---- capacities ----
def _cap_log():
    rng = np.random.default_rng(32)
    log = bytearray(oracle_encode(random_records(rng, 60, maxlog=12) + [bytes(2 * B)] + random_records(rng, 20, maxlog=9)))
    flip(log, first_of_type(log, W.MIDDLE) + H + 1)
    flip(log, first_of_type(log, W.FULL, 3) + H)
    return bytes(log)


def test_capacities(gpu):
    """Each capacity one short of the need, one at a time: only the totals are
    written, with the true totals and the right status bit."""
    import torch
    import lvgpu
    log = _cap_log()
    recs, _, reps, dropped = oracle_read(log)
    pay = sum(len(x) for x in recs)
    assert len(recs) > 2 and len(reps) > 2
    true = {"records": len(recs), "payload_bytes": pay, "reports": len(reps), "dropped_bytes": dropped}
    for kw, bit in ((dict(rec_cap=len(recs) - 1), 2), (dict(payload_cap=pay - 1), 4), (dict(rep_cap=len(reps) - 1), 8)):
        r = collect(torch, run_decode(torch, gpu, log, **kw))
        t = dict(zip(("records", "payload_bytes", "reports", "dropped_bytes", "status"),
                     (int(v) for v in r.dec.totals.cpu().numpy())))
        assert t == dict(true, status=bit), (kw, t)
        assert untouched(torch, r.dec) and guards_ok(r, 0), kw
        with pytest.raises(lvgpu.LvError, match=r"_OVER"):
            r.dec.records()
    # exactly enough of each
    r = collect(torch, run_decode(torch, gpu, log, rec_cap=len(recs), payload_cap=pay, rep_cap=len(reps)))
    assert r.dec.records() == recs and r.dec.reports() == reps and guards_ok(r, pay)


def test_reports_only_counted(gpu):
    """rep_cap = 0 with NULL report arrays: counted, never REPORT_OVER."""
    import torch
    import lvgpu
    log = _cap_log()
    recs, _, reps, dropped = oracle_read(log)
    r = collect(torch, run_decode(torch, gpu, log, reports=False))
    t = r.dec.sync_totals()
    assert t["status"] == 0 and t["reports"] == len(reps) and t["dropped_bytes"] == dropped
    assert r.dec.records() == recs and r.dec.rep_bytes is None
    with pytest.raises(lvgpu.LvError):
        r.dec.reports()


def test_scan_over(gpu):
    """A scan run with cap one short of its count wrote nothing: SCAN_OVER."""
    import torch
    log = _cap_log()
    n = len(W.scan_log(log)[0])
    r = collect(torch, run_decode(torch, gpu, log, cap=n - 1))
    assert r.count == n
    t = [int(v) for v in r.dec.totals.cpu().numpy()]
    assert t[4] == 1 and t[:4] == [0, 0, 0, 0]
    assert untouched(torch, r.dec) and guards_ok(r, 0)
    # and at exactly its count
    r = collect(torch, run_decode(torch, gpu, log, cap=n))
    assert r.dec.records() == oracle_read(log)[0]


def test_no_checksum(gpu):
    """LV_WAL_DECODE_NO_CHECKSUM equals the oracle Reader with checksum=False
    on a log with planted mismatches; d_crc may be NULL."""
    import torch
    log = _cap_log()
    assert oracle_read(log, False) != oracle_read(log, True)
    for null_crc in (False, True):
        r, want = check(torch, gpu, log, checksum=False, null_crc=null_crc)
        assert len(want[0]) == 81
    for name, lg, _ in REASONS:
        check(torch, gpu, lg, checksum=False, null_crc=True, tag=name)


def test_streams(gpu):
    """Two decodes on two streams with separate workspaces, enqueued back to
    back with no sync between them; and both on one stream."""
    import torch
    import lvgpu.wal as LW
    rng = np.random.default_rng(35)
    logs = [oracle_encode(random_records(rng, 300, maxlog=14)), _cap_log() + oracle_encode([b"tail"] * 30, len(_cap_log()))]
    want = [oracle_read(l) for l in logs]
    caps = [len(W.scan_log(l)[0]) + 1 for l in logs]
    d_logs = [to_dev(torch, l, gpu) for l in logs]
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    for streams in ((s1, s2), (s1, s1)):
        with torch.cuda.stream(streams[0]):  # allocations belong to the streams that use them
            bufs = [(torch.empty(LW.scan_workspace_bytes(len(logs[i]), caps[i]), dtype=torch.uint8, device=gpu),
                     torch.empty(LW.decode_workspace_bytes(caps[i]), dtype=torch.uint8, device=gpu),
                     torch.zeros(len(logs[i]), dtype=torch.uint8, device=gpu)) for i in range(2)]
        torch.cuda.synchronize()
        decs = []
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                scan = LW.scan_device(d_logs[i], caps[i], workspace=bufs[i][0], stream=streams[i])
                decs.append(LW.decode_device(d_logs[i], *scan, scan_cap=caps[i], payload=bufs[i][2],
                                             workspace=bufs[i][1], stream=streams[i]))
        torch.cuda.synchronize()
        for i in range(2):
            assert decs[i].records() == want[i][0], (i, streams[0] is streams[1])
            assert decs[i].reports() == want[i][2] and decs[i].record_log_offsets() == want[i][1]


def test_round_trip_in_hbm(gpu):
    """encode_device -> scan_device -> decode_device on one stream, nothing
    read back until the end: the payload and the lengths are the input's, in
    input order."""
    import torch
    import lvgpu.wal as LW
    rng = np.random.default_rng(36)
    recs = [b"", b"foo"] + random_records(rng, 150) + [bytes(2 * B + 5), b""]
    payload, off, ln = pack(recs)
    need, frags = LW.encode_size(ln)
    s = torch.cuda.Stream(device=gpu)
    d_pay = to_dev(torch, payload, gpu, 3)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        log_t = LW.encode_device(d_pay, off, ln, stream=s)
        scan = LW.scan_device(log_t, frags + 8, stream=s)
        dec = LW.decode_device(log_t, *scan, scan_cap=frags + 8, stream=s)
    s.synchronize()
    t = dec.sync_totals()
    assert t == {"records": len(recs), "payload_bytes": len(payload), "reports": 0, "dropped_bytes": 0, "status": 0}
    assert dec.payload[: len(payload)].cpu().numpy().tobytes() == payload
    assert dec.rec_len[: len(recs)].cpu().numpy().tolist() == ln.tolist()
    assert dec.rec_off[: len(recs)].cpu().numpy().tolist() == off.tolist()
    assert dec.records() == recs


def test_graph_capture(gpu):
    """The call asks the runtime nothing about the stream's progress: it can be
    captured into a graph; the replay writes the same outputs."""
    import torch
    import lvgpu.wal as LW
    logs = [_cap_log(), oracle_encode([b"r" * 100] * 50 + [bytes(B)])]
    size = max(len(l) for l in logs)
    cap = max(len(W.scan_log(l)[0]) for l in logs) + 2
    d_log = torch.zeros(size, dtype=torch.uint8, device=gpu)
    d_log[: len(logs[0])].copy_(torch.frombuffer(bytearray(logs[0]), dtype=torch.uint8))
    hdr, crc, info, count = LW.scan_device(d_log[: len(logs[0])], cap)
    ws = torch.empty(LW.decode_workspace_bytes(cap), dtype=torch.uint8, device=gpu)
    pay = torch.zeros(size, dtype=torch.uint8, device=gpu)
    warm = LW.decode_device(d_log[: len(logs[0])], hdr, crc, info, count, scan_cap=cap, payload=pay, workspace=ws)
    assert warm.records() == oracle_read(logs[0])[0]
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dec = LW.decode_device(d_log[: len(logs[0])], hdr, crc, info, count, scan_cap=cap, payload=pay,
                                   workspace=ws, stream=s)
    torch.cuda.synchronize()
    pay.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert dec.records() == oracle_read(logs[0])[0] and dec.reports() == oracle_read(logs[0])[2]


def test_graph_replayed_in_a_longer_chain(gpu):
    """scan -> decode -> WriteBatch decode captured as one graph and replayed
    three times over two logs of one length.  The per-block arrays and the
    WriteBatch decode's head are set by kernels: set by memset nodes, the chain
    replayed correctly once, and in the second replay the decode handed on 65
    of 120 records with status 0 (tests/test_gpu_store.py found it)."""
    import torch
    import lvgpu.wal as LW
    import lvgpu.write_batch as WB
    from write_batch_cases import WriteBatch
    sets = []
    for seed in (3, 4):
        rng = np.random.default_rng(seed)
        reps, seq = [], 1
        for _ in range(120):
            wb = WriteBatch().set_sequence(seq)
            for _ in range(int(rng.integers(1, 9))):
                if rng.random() < 0.4:
                    wb.delete(b"k%02d" % rng.integers(50))
                else:
                    wb.put(b"k%02d" % rng.integers(50), bytes(int(rng.integers(0, 30))))
            seq += wb.count
            reps.append(bytes(wb.rep))
        sets.append((reps, seq - 1))
    size = max(len(oracle_encode(r)) for r, _ in sets) + 200  # both pads take a two-byte varint
    logs = []
    for reps, last in sets:  # the same log length: a last record of one put takes up the difference
        pad = size - len(oracle_encode(reps)) - H - 12 - 1 - 2 - 2
        reps.append(bytes(WriteBatch().set_sequence(last + 1).put(b"p", b"p" * pad).rep))
        logs.append(oracle_encode(reps))
    assert len(logs[0]) == len(logs[1]) == size and size < B
    cap = size // H + 2
    d_log = torch.zeros((size + 15) & ~7, dtype=torch.uint8, device=gpu)[:size]

    def run():
        hdr, crc, info, count = LW.scan_device(d_log, cap)
        dec = LW.decode_device(d_log, hdr, crc, info, count, fill=CANARY)
        ops = WB.decode_device(dec.payload, dec.rec_off, dec.rec_len, dec.totals[0:1], dec.totals[4:5], rec_cap=cap)
        return dec, ops, (hdr, crc, info, count)

    def verify(k, dec, ops, what):
        torch.cuda.synchronize()
        dec._tot = ops._tot = None
        assert dec.records() == sets[k][0] and dec.reports() == [], what
        t = ops.sync_totals()
        assert (t["records"], t["bad_records"], t["last_sequence"]) == (121, 0, sets[k][1] + 1), (what, t)

    def load(k):
        d_log.copy_(torch.frombuffer(bytearray(logs[k]), dtype=torch.uint8))
    load(0)
    dec, ops, keep = run()
    verify(0, dec, ops, "warm-up")
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dec, ops, keep = run()
    torch.cuda.synchronize()
    for k in (1, 0, 1):
        load(k)
        torch.cuda.synchronize()
        g.replay()
        verify(k, dec, ops, f"replay of log {k}")
