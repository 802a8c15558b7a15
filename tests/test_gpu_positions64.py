"""Every pipeline stage with positions beyond 4 GiB, on paths that produce
output.

A. Inputs above the line: each stage reads a small case from a HIGH WINDOW
   (positions64_cases.high_window) laid across position 2^32 of a tensor that
   is otherwise not initialised, with a decoy where a position cut to 32 bits
   would land; all models run on the local layout.
C. A log larger than 4 GiB with one record of 2^32 + 100,000 bytes: encode,
   scan, decode and a damaged record above log position 2^32.
B. A table image larger than 4 GiB: build with a filter, verify, open, get,
   scan and the rewrite chain, against the sparse table model.

Every test asserts in itself that the u64 quantity it is about exceeded 2^32,
and frees its tensors before it returns; the module's peak device memory is
checked at the end.  Not covered: the host twins (a 4 GiB host buffer per CPU
test is another trade) and lv_crc32c_batch_*, whose offsets beyond 4 GiB
test_gpu_batch.py covers at full size."""
import ctypes
import gc

import numpy as np
import pytest

import compact_cases as CC
import memtable_cases as M
import positions64_cases as P
import sst_bloom_cases as B
import sst_build_cases as S
import sst_get_cases as G
import wal_oracle as W
import write_batch_cases as WBC
from positions64_cases import HI
from write_batch_cases import CANARY, GUARD, tail_is_canary

pytestmark = pytest.mark.gpu
PEAK_LIMIT = 16 << 30
BLK = W.BLOCK_SIZE


def _free(torch):
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def peak(gpu):
    import torch
    torch.zeros(1, device=gpu)  # (the allocator has no statistics for a device before its first allocation)
    _free(torch)
    torch.cuda.reset_peak_memory_stats(gpu)
    yield
    _free(torch)


def _window(torch, gpu, window, cut, decoy):
    """The high window as (owner tensor, base, the view that ends with the
    window: what a stage is given as its arena and its byte count)."""
    t, base = P.high_window(torch, gpu, window, cut, decoy)
    assert base < HI < base + len(window)
    return t, base, t[: base + len(window)]


def _dev_equal(torch, a, b, chunk=1 << 28):
    """torch.equal over two uint8 device views in pieces (no 4 GiB temporary)."""
    if a.numel() != b.numel():
        return False
    return all(torch.equal(a[i:i + chunk], b[i:i + chunk]) for i in range(0, a.numel(), chunk))


def _read(t, off, n):
    return t[off:off + n].cpu().numpy().tobytes()


def _dirty(torch, gpu, nbytes):
    return torch.full((max(nbytes, 16),), 0x5A, dtype=torch.uint8, device=gpu)


# ======================= A. inputs above the line ==========================
def test_write_batch_records_above_the_line(gpu):
    """d_rec_off beyond 2^32: 3 T + 5 records across the line, one malformed."""
    import torch
    import lvgpu.write_batch as WB
    n = 3 * WB.WB_TILE + 5
    window, off, ln, decoy, cut = P.batch_case(n)
    want_ops, bounds, st, tot = WBC.model(window, off, ln)
    t, base, pay = _window(torch, gpu, window, cut, decoy)
    rec_off = P.rebase(off, base)
    assert int(rec_off.max()) > HI and int(rec_off.min()) < HI and all(P.sides(off, ln, cut))
    ops = WB.decode_device(pay, WBC.dev_i64(torch, gpu, rec_off), WBC.dev_i64(torch, gpu, ln),
                           WBC.dev_i64(torch, gpu, [n]), rec_cap=n, op_cap=len(want_ops) + 3,
                           workspace=_dirty(torch, gpu, WB.decode_workspace_bytes(n)), fill=CANARY, guard=GUARD)
    WBC.compare(ops, (P.rebase(want_ops, base), bounds, st, tot), "high window")
    got = ops.ops()
    assert int(got["key_off"].max()) > HI and int(got["val_off"].max()) > HI and tot["bad_records"] == 1
    assert (P.unbase(got, base) == want_ops).all()
    del ops, pay, t
    _free(torch)


def _high_table(torch, gpu, case, order=None):
    """The TableCase in a high window: (owner, base, Table).  With `order`
    (the model's) no device build runs: the quadruple is laid down as it is."""
    import lvgpu.memtable as MT
    t, base, pay = _window(torch, gpu, case.payload, case.cut, case.decoy)
    ops = P.rebase(case.ops, base)
    assert int(ops["key_off"].max()) > HI and int(ops["val_off"].max()) > HI and int(ops["key_off"].min()) < HI
    n = len(ops)
    d_ops = M.dev_bytes(torch, gpu, ops)
    if order is not None:
        mt = M.model_totals(case.payload, case.ops)[1]
        d_order = M.dev_bytes(torch, gpu, np.asarray(order, dtype=np.uint32)).view(torch.int32)
        return t, base, MT.Table(pay, d_ops, n, d_order, M.dev_i64(torch, gpu, [mt["entries"], mt["user_keys"], 0]), None)
    table = MT.build_device(pay, d_ops, M.dev_i64(torch, gpu, [n]), op_cap=n,
                            workspace=_dirty(torch, gpu, MT.build_workspace_bytes(n)), fill=CANARY, guard=GUARD)
    return t, base, table


def test_memtable_build_and_get_above_the_line(gpu):
    """key_off / val_off beyond 2^32 for 2 T + 1 ops whose comparisons go to
    the payload, and d_q_off beyond 2^32 in a second window."""
    import torch
    import lvgpu.memtable as MT
    case = P.table_case(2 * MT.MT_TILE + 1)
    t, base, table = _high_table(torch, gpu, case)
    order = M.compare_build(table, case.payload, case.ops, "high window")
    queries = M.queries_for(case.payload, case.ops)[::3]
    qk, off, ln, sq = M.pack_queries(queries, gaps=[i % 5 for i in range(len(queries))])
    mid = next(i for i in range(len(queries) // 2, len(queries)) if ln[i] >= 8)
    qcut = int(off[mid]) + 3
    tq, qbase, d_qk = _window(torch, gpu, qk, qcut, P.complement(qk))
    q_off = P.rebase(off, qbase)
    assert int(q_off.max()) > HI and all(P.sides(off, ln, qcut))
    nq = len(queries)
    d_len = torch.from_numpy(ln.view(np.int32).copy()).to(gpu)
    res = MT.get_device(table, d_qk, M.dev_i64(torch, gpu, q_off), d_len, M.dev_i64(torch, gpu, sq), nq=nq,
                        fill=CANARY, guard=GUARD)
    torch.cuda.synchronize()
    assert tail_is_canary(res, nq * 24)
    got = MT.results(res, nq)
    get = M.model_get_fast(case.payload, case.ops, order)
    seen, above = set(), 0
    for i, (key, seq) in enumerate(queries):
        want = get(key, seq)
        g = {k: int(got[i][k]) for k in want}
        if want["status"] == M.FOUND:
            above += g["val_off"] > HI
            g["val_off"] -= base
        assert g == want, (i, key[:40], seq, g, want)
        seen.add(want["status"])
    assert {M.FOUND, M.DELETED, M.ABSENT} <= seen and above > 0
    del res, table, t, tq, d_qk
    _free(torch)


@pytest.mark.parametrize("bloom", [None, 10], ids=["plain", "bloom"])
def test_sst_build_above_the_line(gpu, bloom):
    """Payload offsets beyond 2^32 for T + 1 entries with suffixes and values
    on both sides of the wave-copy threshold: the image does not depend on
    where the payload lies."""
    import torch
    import lvgpu.table as T
    case = P.table_case(T.SB_TILE + 1)
    ln = case.ops["val_len"]
    assert (ln >= T.SB_WAVE_COPY).any() and (ln < T.SB_WAVE_COPY).any() and (case.ops["key_len"] >= T.SB_WAVE_COPY + 16).any()
    t, base, table = _high_table(torch, gpu, case, order=M.model_order(case.payload, case.ops))
    if bloom is None:
        want = S.model_build(case.payload, case.ops, 1024, 16)
        ws = _dirty(torch, gpu, T.build_workspace_bytes(table.op_cap, len(want[1])))
    else:
        want = B.model_build(case.payload, case.ops, bloom, 1024, 16)
        ws = _dirty(torch, gpu, T.build_bloom_workspace_bytes(table.op_cap, len(want[1])))
    built = T.build_device(table, block_size=1024, restart_interval=16, file_cap=len(want[0]), block_cap=len(want[1]),
                           workspace=ws, fill=CANARY, guard=GUARD, bits_per_key=bloom)
    if bloom is None:
        S.compare_device(built, case.payload, case.ops, 1024, 16, "high window")
    else:
        B.compare_device(built, want, "high window")
    assert want[2]["data_blocks"] > 16
    del built, table, t, ws
    _free(torch)


def test_compact_filter_above_the_line(gpu):
    """The payload and d_range_keys in high windows (lo_off / hi_off beyond
    2^32), LV_COMPACT_BASE_LEVEL with ranges that decide deletions either way."""
    import torch
    import lvgpu.compact as CP
    case = P.table_case(CP.CF_TILE + 1)
    order = np.array(M.model_order(case.payload, case.ops), dtype=np.uint32)
    mt = M.model_totals(case.payload, case.ops)[1]
    ranges, rwin, rows, rdecoy, rcut = P.range_case(case)
    rr = np.array(rows, dtype=CP.RANGE_DTYPE)
    snap = 14
    want = CC.model_filter(case.payload, case.ops, order, mt, snap, (rr, rwin), CC.BASE_LEVEL)
    none = CC.model_filter(case.payload, case.ops, order, mt, snap, None, CC.BASE_LEVEL)
    assert 0 < want[0]["dropped_deletions"] < none[0]["dropped_deletions"] and want[0]["dropped_hidden"] > 0
    t, base, table = _high_table(torch, gpu, case, order=order)
    tr, rbase, d_rk = _window(torch, gpu, rwin, rcut, rdecoy)
    rr_hi = P.rebase(rr, rbase)
    assert int(rr_hi["lo_off"].max()) > HI and int(rr_hi["hi_off"].max()) > HI and int(rr_hi["lo_off"].min()) < HI
    f = CP.filter_device(table, snap, (rr_hi, d_rk), CC.BASE_LEVEL,
                         workspace=_dirty(torch, gpu, CP.filter_workspace_bytes(table.op_cap)), fill=CANARY, guard=GUARD)
    assert f.sync() == want[0]
    assert f.sync_totals() == want[1]
    kept = want[0]["kept"]
    assert f.order_t[:kept].cpu().numpy().view(np.uint32).tolist() == want[2]
    assert tail_is_canary(f.order_t, 4 * kept)
    del f, table, t, tr, d_rk
    _free(torch)


def test_hash_above_the_line(gpu):
    """d_off and 8-byte bounds beyond 2^32 against the hash oracle."""
    import torch
    from lvgpu import hash as H
    L = W.lib()
    L.oracle_hash_batch.restype = None
    L.oracle_hash_batch.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t]
    window, off, ln, decoy, cut = P.hash_case()
    n = len(off)
    arena = np.frombuffer(window, dtype=np.uint8).copy()
    rng = np.random.default_rng(6)
    seeds = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    want = np.zeros(n, dtype=np.uint32)
    L.oracle_hash_batch(arena.ctypes.data, off.ctypes.data, ln.ctypes.data, seeds.ctypes.data, want.ctypes.data, n)
    t, base, view = _window(torch, gpu, window, cut, decoy)
    hi_off = P.rebase(off, base)
    assert int(hi_off.max()) > HI and int(hi_off.min()) < HI and all(P.sides(off, ln, cut))
    d_seed = torch.from_numpy(seeds.view(np.int32).copy()).to(gpu)
    d_len = torch.from_numpy(ln.view(np.int32).copy()).to(gpu)
    got = H.hash_batch(view, M.dev_i64(torch, gpu, hi_off), d_len, d_seed)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    bounds = np.concatenate([hi_off, [hi_off[-1] + np.uint64(ln[-1])]]).astype(np.uint64)
    got = H.hash_batch_packed(view, M.dev_i64(torch, gpu, bounds), d_seed)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    sh = H.hash_batch_packed(view, M.dev_i64(torch, gpu, bounds), d_seed, shard=True)
    assert np.array_equal(sh.cpu().numpy().view(np.uint32), want >> 28)
    del got, sh, view, t
    _free(torch)


def test_seal_and_verify_above_the_line(gpu):
    """Handles beyond 2^32 in a file tensor of 4 GiB and a little, one block
    across the line: the trailers are the model's, every block verifies, and
    one flipped byte above the line fails that block only."""
    import torch
    import lvgpu.table as T
    rng = np.random.default_rng(12)
    sizes = [300, 2500, 64, 1, 4097, 700]
    types = np.array([0, 1, 0, 0, 1, 0], dtype=np.uint8)
    window, handles = bytearray(), []
    for sz in sizes:
        window += b"\xEE" * int(rng.integers(0, 9))
        handles.append((len(window), sz))
        window += bytes(rng.integers(0, 256, size=sz, dtype=np.uint8)) + b"\xEE" * 5
    window = bytes(window)
    cut = handles[1][0] + 1000  # block 1 lies across the line
    decoy = bytearray(P.complement(window))
    t, base, file_t = _window(torch, gpu, window, cut, bytes(decoy))
    want = bytearray(window)
    for (o, sz), ty in zip(handles, types.tolist()):
        crc = W.mask(W.value(window[o:o + sz] + bytes([ty])))
        want[o + sz:o + sz + 5] = bytes([ty]) + crc.to_bytes(4, "little")
    hs = np.array(handles, dtype=np.uint64)
    hs[:, 0] += np.uint64(base)
    assert int(hs[:, 0].max()) > HI and int(hs[0, 0]) < HI < int(hs[1, 0] + hs[1, 1])
    d_h = M.dev_i64(torch, gpu, hs.reshape(-1)).view(-1, 2)
    T.seal_blocks(file_t, d_h, torch.from_numpy(types).to(gpu))
    assert _read(file_t, base, len(window)) == bytes(want)
    # the decoy's part above the line, at the start of the tensor, is as it was
    assert _read(t, 0, len(window) - cut) == bytes(decoy[cut:])
    st, crc = T.verify_blocks(file_t, d_h, out_crc=True)
    assert st.cpu().tolist() == [T.BLOCK_OK] * len(handles)
    assert crc.cpu().numpy().view(np.uint32).tolist() == [W.value(bytes(want[o:o + sz + 1])) for o, sz in handles]
    victim = 4
    at = base + handles[victim][0] + 2000
    assert at > HI
    file_t[at] ^= 0x10
    st = T.verify_blocks(file_t, d_h).cpu().tolist()
    assert st == [T.BLOCK_CHECKSUM_MISMATCH if i == victim else T.BLOCK_OK for i in range(len(handles))]
    del st, crc, d_h, file_t, t
    _free(torch)


# ======================= C. a log larger than 4 GiB ========================
LOG_SEED = 0x4C4F4736
BIG_RECORD = HI + 100_000


def _log_layout():
    """(recs [(rec_off, rec_len)], index of the big record, index of the
    record to damage): about 20 small records (an empty one, one that ends 3
    bytes before a block end), the record of 2^32 + 100,000 bytes, then about
    20 small ones that lie behind it in the payload, one of them the last of
    its block (3 bytes short of the end)."""
    rng = np.random.default_rng(21)
    lens = []

    def short_of_end():
        room = BLK - P.Fragments(lens).size % BLK
        if room < 7 + 3 + 1:
            lens.append(40)
            room = BLK - P.Fragments(lens).size % BLK
        lens.append(room - 7 - 3)
    for i in range(18):
        lens.append(0 if i == 4 else int(rng.integers(1, 3000)))
    short_of_end()
    lens.append(17)
    big = len(lens)
    lens.append(BIG_RECORD)
    for i in range(10):
        lens.append(int(rng.integers(1, 3000)))
    short_of_end()
    victim = len(lens) - 1
    for i in range(9):
        lens.append(int(rng.integers(1, 3000)))
    recs, at = [], 11
    for n in lens:
        recs.append((at, n))
        at += n + int(rng.integers(0, 9))
    return recs, big, victim


class TestLogBeyond4GiB:
    @pytest.fixture(scope="class")
    def log(self, gpu):
        import torch
        import lvgpu
        import lvgpu.wal as LW
        recs, big, victim = _log_layout()
        frags = P.Fragments([n for _, n in recs])
        total = recs[-1][0] + recs[-1][1]
        arena = torch.empty(total + 64, dtype=torch.uint8, device=gpu)
        lvgpu.fill_splitmix(arena, 0, LOG_SEED)
        off = np.array([o for o, _ in recs], dtype=np.uint64)
        ln = np.array([n for _, n in recs], dtype=np.uint64)
        need, nfrag = LW.encode_size(ln, 0)
        buf = torch.empty(need + GUARD, dtype=torch.uint8, device=gpu)
        buf[need:] = CANARY
        out = LW.encode_device(arena, off, ln, 0, out=buf[:need])
        torch.cuda.synchronize()
        box = dict(recs=recs, big=big, victim=victim, frags=frags, arena=arena, off=off, ln=ln, need=need, nfrag=nfrag,
                   buf=buf, out=out)
        yield box
        box.clear()
        del arena, buf, out
        _free(torch)

    def test_encode(self, gpu, log):
        """rec_len and rec_off beyond 2^32; the blocks at the start, on either
        side of log position 2^32, where the big record ends and at the end
        equal the Writer's."""
        recs, frags, out = log["recs"], log["frags"], log["out"]
        assert int(log["ln"].max()) > HI and int(log["off"].max()) > HI
        assert out.numel() == log["need"] == frags.size > HI and log["nfrag"] == len(frags.hdr_off)
        assert tail_is_canary(log["buf"], log["need"])
        last = frags.blocks() - 1
        end_of_big = int(frags.hdr_off[np.nonzero(frags.rec == log["big"])[0][-1]]) // BLK
        line = HI // BLK
        assert 1 < line - 1 and line < end_of_big <= last and int(frags.rec_log_off[-1]) // BLK == last
        for k in sorted({0, 1, line - 1, line, end_of_big, last - 1, last}):
            want = P.expected_log_block(k, recs, LOG_SEED, frags=frags)
            got = _read(out, k * BLK, len(want))
            assert got == want, ("block", k, next(i for i, (a, b) in enumerate(zip(got, want)) if a != b))

    def _scan(self, torch, log):
        import lvgpu.wal as LW
        cap = log["nfrag"] + 8
        return LW.scan_device(log["out"], cap) + (cap,)

    def test_scan(self, gpu, log):
        """d_hdr_off beyond 2^32: every fragment's offset, type, status and
        length, compared on the device."""
        import torch
        frags = log["frags"]
        hdr, crc, info, count, cap = self._scan(torch, log)
        n = int(count.cpu()[0])
        assert n == len(frags.hdr_off) == log["nfrag"]
        want_hdr = torch.from_numpy(frags.hdr_off.view(np.int64).copy()).to(gpu)
        want_info = torch.from_numpy(frags.info().view(np.int32).copy()).to(gpu)
        assert int(hdr[:n].max()) > HI
        assert torch.equal(hdr[:n], want_hdr) and torch.equal(info[:n], want_info)
        del hdr, crc, info, count, want_hdr, want_info
        _free(torch)

    def test_decode(self, gpu, log):
        """d_rec_len, d_rec_off and d_rec_log_off beyond 2^32; the decoded
        payload is the input extents end to end."""
        import torch
        import lvgpu.wal as LW
        recs, frags, arena = log["recs"], log["frags"], log["arena"]
        hdr, crc, info, count, cap = self._scan(torch, log)
        total = int(log["ln"].sum())
        pay = torch.empty(total + GUARD, dtype=torch.uint8, device=gpu)
        pay[total:] = CANARY
        dec = LW.decode_device(log["out"], hdr, crc, info, count, payload=pay[:total], scan_cap=cap,
                               rec_cap=len(recs) + 4, rep_cap=16, fill=CANARY)
        t = dec.sync_totals()
        assert t == dict(records=len(recs), payload_bytes=total, reports=0, dropped_bytes=0, status=0)
        n = len(recs)
        rec_len = dec.rec_len[:n].cpu().numpy().view(np.uint64)
        rec_off = dec.rec_off[:n].cpu().numpy().view(np.uint64)
        rec_log = dec.rec_log_off[:n].cpu().numpy().view(np.uint64)
        assert rec_len.tolist() == log["ln"].tolist() and int(rec_len.max()) > HI
        assert rec_off.tolist() == (np.cumsum(log["ln"]) - log["ln"]).tolist() and int(rec_off.max()) > HI
        assert rec_log.tolist() == frags.rec_log_off.tolist() and int(rec_log.max()) > HI
        assert tail_is_canary(pay, total) and tail_is_canary(dec.rec_len, 8 * n) and tail_is_canary(dec.rep_bytes, 0)
        for (o, ln), ro in zip(recs, rec_off.tolist()):
            assert _dev_equal(torch, pay[ro:ro + ln], arena[o:o + ln]), ("record at", o, ln)
        del dec, pay, hdr, crc, info, count
        _free(torch)

    def test_damaged_record_above_the_line(self, gpu, log):
        """One flipped payload byte in a small record above log position 2^32:
        one LV_WAL_DROP_CHECKSUM report at that record's header, with the bytes
        the oracle Reader drops for the same flip in a log scaled down by whole
        blocks; every other record is unchanged."""
        import torch
        import lvgpu.wal as LW
        import wal_decode_cases as WD
        import wal_encode_cases as WE
        recs, frags, out, big, victim = log["recs"], log["frags"], log["out"], log["big"], log["victim"]
        vhdr = int(frags.rec_log_off[victim])
        assert vhdr > HI and 3 < recs[victim][1] < BLK - 7
        # the scaled-down log: the big record shorter by whole blocks of payload
        m = (BIG_RECORD // (BLK - 7)) - 3
        small = [(o, n - m * (BLK - 7) if i == big else n) for i, (o, n) in enumerate(recs)]
        data = [P.splitmix_bytes(o + (m * (BLK - 7) if i == big else 0), n, LOG_SEED) for i, (o, n) in enumerate(small)]
        slog = bytearray(WE.oracle_encode(data))
        sf = P.Fragments([n for _, n in small])
        assert int(sf.rec_log_off[victim]) == vhdr - m * BLK and sf.size == frags.size - m * BLK
        slog[vhdr - m * BLK + 7 + 2] ^= 0x40
        want_recs, want_offs, want_reports, _ = WD.oracle_read(bytes(slog))
        assert len(want_reports) == 1 and want_reports[0][1] == "checksum mismatch" and len(want_recs) == len(recs) - 1
        out[vhdr + 7 + 2] ^= 0x40
        try:
            hdr, crc, info, count, cap = self._scan(torch, log)
            dec = LW.decode_device(out, hdr, crc, info, count, scan_cap=cap, rec_cap=len(recs) + 4, rep_cap=16,
                                   payload=torch.empty(int(log["ln"].sum()), dtype=torch.uint8, device=gpu), fill=CANARY)
            t = dec.sync_totals()
        finally:
            out[vhdr + 7 + 2] ^= 0x40
            torch.cuda.synchronize()
        assert t["reports"] == 1 and t["records"] == len(recs) - 1 and t["status"] == 0
        assert int(dec.rep_reason[0].cpu()) == 2  # LV_WAL_DROP_CHECKSUM
        assert int(dec.rep_log_off[0].cpu()) == vhdr
        assert int(dec.rep_bytes[0].cpu()) == want_reports[0][0] == t["dropped_bytes"]
        keep = [i for i in range(len(recs)) if i != victim]
        n = len(keep)
        assert dec.rec_len[:n].cpu().numpy().view(np.uint64).tolist() == [recs[i][1] for i in keep]
        assert [len(r) + (m * (BLK - 7) if i == big else 0) for i, r in zip(keep, want_recs)] == [recs[i][1] for i in keep]
        rec_log = dec.rec_log_off[:n].cpu().numpy().view(np.uint64).tolist()
        assert rec_log == frags.rec_log_off[keep].tolist()
        assert rec_log == [o + (m * BLK if i > big else 0) for i, o in zip(keep, want_offs)]
        rec_off = dec.rec_off[:n].cpu().numpy().view(np.uint64).tolist()
        for i, ro in zip(keep, rec_off):
            if i != big:
                assert _read(dec.payload, ro, recs[i][1]) == P.splitmix_bytes(*recs[i], LOG_SEED), i
        del dec, hdr, crc, info, count
        _free(torch)


# ================= B. a table image larger than 4 GiB ======================
TABLE_SEED = 0x54424C36
BIG_VALUE = (1 << 31) + 4096
KEY_AREA = 1 << 16


def _table_layout():
    """(key area bytes, ops in log order, entries for the sparse model): about
    50 small entries, two whose values are one shared extent of 2^31 + 4096
    bytes, then 2,100 entries of 2,100 to 3,000 bytes, two to a block, so that
    the scan sees more than a tile of blocks and runs.  Keys lie in a key area
    at the start of the payload; values are extents of the splitmix arena
    behind it."""
    rng = np.random.default_rng(33)
    items = []
    for i in range(50):
        # (9 more bytes in front: the big blocks then end 9 bytes past a 16-byte granule, see test_big_table_build)
        items.append((b"a%04d" % i, ((100 + i) << 8) | (0 if i % 10 == 7 else 1), int(rng.integers(0, 200)) + (9 if i == 0 else 0)))
    items.append((b"big0", (5 << 8) | 1, BIG_VALUE))
    items.append((b"big1", (6 << 8) | 1, BIG_VALUE))
    for i in range(2100):
        items.append((b"k%05d" % (i // 2 if i % 50 == 1 else i), ((200 + i) << 8) | 1, int(rng.integers(2100, 3000))))
    keys, ops, at = bytearray(), [], KEY_AREA + 5
    big_off = None
    for key, tg, vlen in items:
        ko = len(keys)
        keys += key
        if tg & 0xFF == 0:
            vlen = 0
        if vlen == BIG_VALUE:
            if big_off is None:
                big_off, at = at, at + vlen
            vo = big_off
        else:
            vo, at = at, at + vlen + int(rng.integers(0, 4))
        ops.append((tg, ko, vo, len(key), vlen))
    assert len(keys) <= KEY_AREA
    ops = np.array(ops, dtype=M.op_dtype())
    perm = rng.permutation(len(ops))
    return bytes(keys), ops[perm], at


def _model_entries(keys, ops):
    """The entries in memtable order for model_build_sparse: small values as
    bytes of the arena, the big ones as extents."""
    order = sorted(range(len(ops)), key=lambda i: (keys[int(ops[i]["key_off"]):int(ops[i]["key_off"]) + int(ops[i]["key_len"])],
                                                   -int(ops[i]["tag"]), -i))
    ents = []
    for i in order:
        o = ops[i]
        ko, kl, vo, vl = int(o["key_off"]), int(o["key_len"]), int(o["val_off"]), int(o["val_len"])
        value = ("ext", vo, vl) if vl == BIG_VALUE else P.splitmix_bytes(vo, vl, TABLE_SEED)
        ents.append((S.ikey(keys[ko:ko + kl], int(o["tag"])), value))
    return order, ents


@pytest.fixture(scope="module")
def big_table(gpu):
    """The payload, the memtable, the image built by lv_sst_build_bloom_device
    and the sparse model, built once."""
    import torch
    import lvgpu
    import lvgpu.memtable as MT
    import lvgpu.table as T
    keys, ops, total = _table_layout()
    payload = torch.empty(total + 64, dtype=torch.uint8, device=gpu)
    lvgpu.fill_splitmix(payload, 0, TABLE_SEED)
    payload[: len(keys)].copy_(torch.frombuffer(bytearray(keys), dtype=torch.uint8))
    n = len(ops)
    table = MT.build_device(payload[:total], M.dev_bytes(torch, gpu, ops), M.dev_i64(torch, gpu, [n]), op_cap=n)
    order, ents = _model_entries(keys, ops)
    crc = P.splitmix_crc(TABLE_SEED)
    model = P.model_build_sparse(ents, 4096, 16, 10, crc)
    file_cap = T.bloom_file_bound(total, n, 10)
    assert file_cap >= model.size
    built = T.build_bloom_device(table, 10, block_size=4096, restart_interval=16, file_cap=file_cap, block_cap=n,
                                 fill=CANARY, guard=GUARD)
    tot = built.sync_totals()
    box = dict(keys=keys, ops=ops, order=order, ents=ents, payload=payload, total=total, table=table, model=model,
               built=built, tot=tot, crc=crc)
    yield box
    box.clear()
    del payload, table, built
    _free(torch)


def _check_image(torch, file_t, model, payload):
    """Every bytes segment by read-back, every ext segment against its payload
    extent on the device."""
    exts = 0
    for at, seg in model.placed():
        if isinstance(seg, tuple):
            assert _dev_equal(torch, file_t[at:at + seg[2]], payload[seg[1]:seg[1] + seg[2]]), ("ext segment at", at)
            exts += 1
        else:
            got = _read(file_t, at, len(seg))
            if got != bytes(seg):
                d = next(i for i, (a, b) in enumerate(zip(got, seg)) if a != b)
                raise AssertionError(("file differs at", at + d, got[d:d + 16].hex(), bytes(seg[d:d + 16]).hex()))
    return exts


def test_big_table_build(gpu, big_table):
    """Totals, handles and every byte of the image against the sparse model.
    The two blocks of more than 2^31 bytes end off the 16-byte grid with a
    nonzero byte in their last granule: their trailers pin the CRC walk's tail
    for a unit that long.  The filter block is one of the compared segments,
    its offset array included: with a 2 KiB window to every filter, the lanes
    of sb_bloom_offsets go round their capped grid several times here."""
    import torch
    import loop_trips as LT
    model, built = big_table["model"], big_table["built"]
    filters = model.bloom_totals["filters"]
    grid, per = LT.grid_of("sb_bloom_offsets", built.file_cap >> 11, 1)  # the launch: sized by file_cap
    assert filters == len(model.filter.offsets) == model.bloom()["num"] and -(-filters // per) >= 2 * grid
    assert LT.grid_of("sb_bloom_offsets", filters, 1) == (grid, per) and LT.trips("sb_bloom_offsets", filters, 1) >= 2
    array = model.bloom_totals["filter_offset"] + model.bloom()["array_offset"]
    assert any(not isinstance(seg, tuple) and at <= array and array + 4 * filters <= at + len(seg)
               for at, seg in model.placed()), "the offset array is not inside a compared segment"
    big = [(o, sz) for o, sz in model.handles if sz > (1 << 31)]
    assert len(big) == 2 and all((o + sz) % 16 >= 4 for o, sz in big)
    assert big_table["tot"] == model.totals and built.sync_bloom_totals() == model.bloom_totals
    assert model.size > HI and model.bloom_totals["filter_offset"] > HI and model.totals["metaindex_offset"] > HI
    assert model.totals["index_offset"] > HI and model.totals["data_blocks"] > 1024
    assert built.handles() == model.handles
    assert sum(1 for o, _ in model.handles if o > HI) > 1024
    assert _check_image(torch, built.file_t, model, big_table["payload"]) == 2
    assert tail_is_canary(built.file_t, model.size)


def test_big_table_verify(gpu, big_table):
    import lvgpu.table as T
    built = big_table["built"]
    st = T.verify_blocks(built.file_t[: big_table["model"].size], built.handles_view())
    assert int(built.handles_view()[:, 0].max()) > HI
    assert st.cpu().tolist() == [T.BLOCK_OK] * len(big_table["model"].handles)


def _open(big_table):
    import lvgpu.table as T
    built, model = big_table["built"], big_table["model"]
    op = T.open_device(built.file_t[: built.file_cap], built.totals[2:3], built.totals[7:8],
                       block_cap=model.totals["data_blocks"], fill=CANARY, guard=GUARD)
    return op, T.bloom_open_device(op)


def test_big_table_open(gpu, big_table):
    import torch
    import lvgpu.table as T
    model = big_table["model"]
    op, bloom_t = _open(big_table)
    assert op.sync() == model.table()
    assert T.bloom_dict(bloom_t) == model.bloom()
    assert model.table()["index_offset"] > HI and model.bloom()["filter_offset"] > HI
    assert op.handles() == model.block_handles + model.handles[-2:]
    assert tail_is_canary(op.handles_t, 16 * (len(model.block_handles) + 2))
    del op, bloom_t
    _free(torch)


def test_big_table_get(gpu, big_table):
    """Every user key, 200 absent keys and both big keys through both gets."""
    import torch
    import lvgpu.table as T
    model, built, payload = big_table["model"], big_table["built"], big_table["payload"]
    users = sorted({S.user(k) for k, _, _, _ in model.entries})
    rng = np.random.default_rng(44)
    absent = [b"k%05d" % int(v) for v in rng.integers(2100, 99999, size=100)] + [b"a%04dx" % i for i in range(50)] + \
             [b"b%04d" % i for i in range(48)] + [b"", b"big"]
    queries = [(k, M.MAX_SEQUENCE) for k in users] + [(k, 150) for k in users[::7]] + [(k, M.MAX_SEQUENCE) for k in absent]
    assert (b"big0", M.MAX_SEQUENCE) in queries and (b"big1", M.MAX_SEQUENCE) in queries
    qk, off, ln, sq = M.pack_queries(queries)
    op, bloom_t = _open(big_table)
    dq = G.dev_queries(torch, gpu, qk, off, ln, sq)
    nq = len(queries)
    plain = T.get_device(op, *dq, nq=nq, fill=CANARY, guard=GUARD)
    filt = T.get_bloom_device(op, bloom_t, *dq, nq=nq, fill=CANARY, guard=GUARD)
    for g, filtered in ((plain, False), (filt, True)):
        got = g.sync()
        assert tail_is_canary(g.res, nq * 32)
        wants = [model.get(k, s, filtered=filtered) for k, s in queries]
        seen = G.compare_results(got, wants, "filtered" if filtered else "plain")
        assert {G.FOUND, G.DELETED, G.ABSENT} <= seen
        found = [(w, q) for w, q in zip(wants, queries) if w["status"] == G.FOUND]
        assert sum(w["val_off"] > HI for w, _ in found) > len(found) // 2
        if filtered:
            # not vacuous: 198 of the 200 absent keys reach a filter, which at 10 bits per key passes about 1 %
            rejected = sum(w["reserved"] == B.FILTERED for w in wants)
            assert rejected >= 150 and all(w["status"] == G.ABSENT for w in wants if w["reserved"])
    # the value bytes: small ones by read-back, the big ones on the device
    got = filt.sync()
    by_key = {}
    for (k, v) in big_table["ents"]:
        by_key.setdefault(S.user(k), v)  # the newest version of a user key comes first
    for i, (k, s) in enumerate(queries):
        if s != M.MAX_SEQUENCE or int(got[i]["status"]) != G.FOUND:
            continue
        vo, vl = int(got[i]["val_off"]), int(got[i]["val_len"])
        v = by_key[k]
        if isinstance(v, tuple):
            assert vl == BIG_VALUE and _dev_equal(torch, built.file_t[vo:vo + vl], payload[v[1]:v[1] + v[2]]), k
        else:
            assert _read(built.file_t, vo, vl) == v, k
    del plain, filt, op, bloom_t, dq
    _free(torch)


@pytest.fixture(scope="module")
def big_scan(gpu, big_table):
    import torch
    import lvgpu.table as T
    model = big_table["model"]
    ops, size = model.scan_ops()
    op, _ = _open(big_table)
    n = len(ops)
    arena = torch.empty(size + GUARD, dtype=torch.uint8, device=gpu)
    arena[size:] = CANARY
    sc = T.scan_device(op, arena_cap=size, op_cap=n, block_cap=model.totals["data_blocks"], order=True,
                       arena_t=arena[:size], fill=CANARY, guard=GUARD)
    tot = sc.sync()
    box = dict(sc=sc, arena=arena, ops=ops, size=size, tot=tot)
    yield box
    box.clear()
    del sc, arena, op
    _free(torch)


def test_big_table_scan(gpu, big_table, big_scan):
    """The op table and every arena position are the model's; keys and small
    values by read-back, the big values on the device."""
    import torch
    model, payload = big_table["model"], big_table["payload"]
    sc, arena, ops, size, tot = (big_scan[k] for k in ("sc", "arena", "ops", "size", "tot"))
    n = len(ops)
    assert size > HI
    assert tot["entries"] == tot["table_entries"] == n and tot["arena_bytes"] == tot["table_bytes"] == size
    assert tot["data_blocks"] == model.totals["data_blocks"] > 1024 and tot["runs"] > 1024 and tot["status"] == 0
    got = sc.ops()
    want = np.array(ops, dtype=M.op_dtype())
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ("op", int(bad[0]), got[bad[0]], want[bad[0]])
    assert int(got["key_off"].max()) > HI and (got["key_off"] > HI).sum() > 2000
    assert sc.mt() == dict(entries=n, user_keys=len({S.user(k) for k, _ in big_table["ents"]}), status=0)
    assert sc.order_t[:n].cpu().numpy().view(np.uint32).tolist() == list(range(n))
    assert tail_is_canary(arena, size) and tail_is_canary(sc.ops_t, 32 * n)
    for (tg, ko, vo, kl, vl), (k, v) in zip(ops, big_table["ents"]):
        if isinstance(v, tuple):
            assert _read(arena, ko, kl) == S.user(k)
            assert _dev_equal(torch, arena[vo:vo + vl], payload[v[1]:v[1] + v[2]]), ("big value at", vo)
    # everything that is not a big value, in three read-backs
    bigs = [(vo, vl) for (_, _, vo, _, vl), (_, v) in zip(ops, big_table["ents"]) if isinstance(v, tuple)]
    flat = [(S.user(k), v) for k, v in big_table["ents"]]
    pieces, cur = [], bytearray()
    for k, v in flat:
        cur += k
        if isinstance(v, tuple):
            pieces.append(bytes(cur))
            cur = bytearray()
        else:
            cur += v
    pieces.append(bytes(cur))
    starts = [0] + [vo + vl for vo, vl in bigs]
    assert len(pieces) == len(starts) == 3
    for at, want_bytes in zip(starts, pieces):
        assert _read(arena, at, len(want_bytes)) == want_bytes, ("arena piece at", at)


def test_big_table_chain(gpu, big_table, big_scan):
    """Memtable build -> compaction filter (snapshot above every sequence, no
    ranges) -> table build with another block size over the scan's quadruple,
    all of whose positions after the first big value exceed 2^32."""
    import torch
    import lvgpu.compact as CP
    import lvgpu.memtable as MT
    import lvgpu.table as T
    sc, size = big_scan["sc"], big_scan["size"]
    n = len(big_scan["ops"])
    src = sc.memtable()
    table = MT.build_device(src.payload, src.ops_t, sc.totals[0:1], sc.totals[7:8], op_cap=n)
    assert table.order().tolist() == list(range(n))
    f = CP.filter_device(table, M.MAX_SEQUENCE - 1, None, 0)
    ct = f.sync()
    # the snapshot sees every sequence: only the newest version of a user key stays
    ents = big_table["ents"]
    kept = [i for i, (k, _) in enumerate(ents) if i == 0 or S.user(ents[i - 1][0]) != S.user(k)]
    assert ct["kept"] == len(kept) < n and ct["dropped_hidden"] == n - len(kept) and ct["dropped_deletions"] == 0
    model = P.model_build_sparse([ents[i] for i in kept], 1500, 5, None, big_table["crc"])
    assert model.size > HI
    built = T.build_device(f, block_size=1500, restart_interval=5, file_cap=model.size, block_cap=len(model.block_handles),
                           fill=CANARY, guard=GUARD)
    assert built.sync_totals() == model.totals
    assert built.handles() == model.handles and sum(1 for o, _ in model.handles if o > HI) > 1000
    assert _check_image(torch, built.file_t, model, big_table["payload"]) == 2
    assert tail_is_canary(built.file_t, model.size)
    del built, f, table, src
    _free(torch)


def test_peak_device_memory(gpu, big_table, big_scan):
    """The module stays at or under 16 GiB of device memory."""
    import torch
    assert torch.cuda.max_memory_allocated(gpu) <= PEAK_LIMIT, torch.cuda.max_memory_allocated(gpu)
