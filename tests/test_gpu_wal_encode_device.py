"""lv_wal_encode_device: the WAL group-commit encode with the payload and the
log in HBM.  Every output is compared byte for byte with oracle/wal_oracle.py's
Writer."""
import ctypes

import numpy as np
import pytest

from wal_encode_cases import (B, CANARY, EDGES, H, encode_checked, first_diff, oracle_encode, pack, random_records,
                               to_dev, trailer_edge, writer_recipe)
import wal_oracle as W

pytestmark = pytest.mark.gpu


def _check(torch, dev, recs, dest_length=0, **kw):
    payload, off, ln = pack(recs)
    got, guards_ok = encode_checked(torch, dev, payload, off, ln, dest_length, **kw)
    assert first_diff(got, oracle_encode(recs, dest_length)) is None, first_diff(got, oracle_encode(recs, dest_length))
    assert guards_ok, "bytes outside d_out[0, out_len) were written"


@pytest.mark.parametrize("dest_length", EDGES)
def test_block_edges(gpu, dest_length):
    import torch
    _check(torch, gpu, writer_recipe(dest_length), dest_length)


@pytest.mark.parametrize("dest_length", EDGES)
def test_trailer_edges(gpu, dest_length):
    import torch
    for k in range(9):
        _check(torch, gpu, trailer_edge(k, dest_length), dest_length, out_shift=k, pay_shift=(3 * k) % 16)


def test_dense_headers(gpu):
    import torch
    import lvgpu.wal as LW
    recs = [bytes([k & 0xFF]) * (k % 9) for k in range(20000)]
    for dest_length in (0, B - 20):
        _check(torch, gpu, recs, dest_length, out_shift=5)
    for dest_length in (0, B - H - 2, B - 3):
        _check(torch, gpu, [b""] * 5, dest_length)
    # no records: out_len 0, LV_OK, nothing written
    out = torch.full((64,), CANARY, dtype=torch.uint8, device=gpu)
    pay = torch.zeros(16, dtype=torch.uint8, device=gpu)
    got = LW.encode_device(pay, [], [], 0, out=out)
    torch.cuda.synchronize()
    assert got.numel() == 0 and bool((out == CANARY).all())
    assert LW.encode_device(torch.empty(0, dtype=torch.uint8, device=gpu), [], []).numel() == 0


def test_alignment(gpu):
    import torch
    rng = np.random.default_rng(11)
    recs = random_records(rng, 36, maxlog=13) + [rng.integers(0, 256, size=2 * B + 100, dtype=np.uint8).tobytes(), b"",
                                                 b"abc", rng.integers(0, 256, size=9000, dtype=np.uint8).tobytes()]
    payload, off, ln = pack(recs)
    want = oracle_encode(recs, 100)
    assert 2 * B < len(want) + 100 <= 3 * B  # the log's tail spans three blocks
    for s in range(16):
        for ps in (0, 1, 3, 8, 13):
            got, guards_ok = encode_checked(torch, gpu, payload, off, ln, 100, out_shift=s, pay_shift=ps)
            assert first_diff(got, want) is None, (s, ps, first_diff(got, want))
            assert guards_ok, (s, ps)


def test_arbitrary_record_slices(gpu):
    """Records that overlap, repeat one slice and run in descending order."""
    import torch
    rng = np.random.default_rng(12)
    payload = rng.integers(0, 256, size=3 * B, dtype=np.uint8).tobytes()
    off = [2 * B, 100, 100, 90, 0, 2 * B + 5, 50, 3 * B, 7]
    ln = [B - 5, 40000, 40000, 500, 3 * B, 0, 1, 0, 33]
    assert all(o + n <= len(payload) for o, n in zip(off, ln))
    recs = [payload[o:o + n] for o, n in zip(off, ln)]
    got, guards_ok = encode_checked(torch, gpu, payload, np.array(off, dtype=np.uint64), np.array(ln, dtype=np.uint64),
                                    B - 9, out_shift=7, pay_shift=2)
    assert first_diff(got, oracle_encode(recs, B - 9)) is None and guards_ok


def test_capacity(gpu):
    import torch
    import lvgpu
    import lvgpu.wal as LW
    L = LW._bind()
    recs = random_records(np.random.default_rng(13), 50, maxlog=12)
    payload, off, ln = pack(recs)
    need, frags = LW.encode_size(ln)
    d_pay = to_dev(torch, payload, gpu)
    out = torch.full((need + 64,), CANARY, dtype=torch.uint8, device=gpu)
    ws = torch.empty(LW.encode_workspace_bytes(frags), dtype=torch.uint8, device=gpu)
    got = ctypes.c_size_t(0)
    args = lambda cap: (ctypes.c_void_p(d_pay.data_ptr()), d_pay.numel(), off.ctypes.data, ln.ctypes.data, ln.size, 0,
                        ctypes.c_void_p(out.data_ptr()), cap, ctypes.byref(got), ctypes.c_void_p(ws.data_ptr()),
                        ws.numel(), lvgpu._stream_ptr(None))
    assert L.lv_wal_encode_device(*args(need - 1)) == -1 and got.value == need
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    got.value = 0
    assert L.lv_wal_encode_device(*args(need)) == 0 and got.value == need
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert host[:need].tobytes() == oracle_encode(recs) and (host[need:] == CANARY).all()


def test_more_blocks_than_compute_units(gpu):
    """Skewed records over more log blocks than wal_frame_kernel has
    workgroups: sized from the launcher's cap (tests/loop_trips.py), so every
    workgroup takes a second block whatever the cap becomes."""
    import torch
    import loop_trips as LT
    cus = LT.device_cus(gpu)
    nb = max(LT.size_for("wal_frame_kernel", 2, cus, 3), 512)
    r = W.Random(301)
    sizes, tot = [], 0
    while tot < nb * B:
        sizes.append(r.skewed(17))
        tot += sizes[-1]
    payload = np.random.default_rng(14).integers(0, 256, size=tot, dtype=np.uint8).tobytes()
    ln = np.array(sizes, dtype=np.uint64)
    off = np.zeros(ln.size, dtype=np.uint64)
    off[1:] = np.cumsum(ln[:-1])
    recs = [payload[int(o):int(o + n)] for o, n in zip(off, ln)]
    got, guards_ok = encode_checked(torch, gpu, payload, off, ln, 0, out_shift=9, pay_shift=4)
    want = oracle_encode(recs)
    assert len(want) >= nb * B and LT.trips("wal_frame_kernel", -(-len(want) // B), cus) >= 2
    assert first_diff(got, want) is None, first_diff(got, want)
    assert guards_ok


def test_streams(gpu):
    """A non-default stream; then two calls with different records enqueued
    back to back with no sync between them (each call's staged fragment table
    must survive until its copy has run), on one stream and on two."""
    import torch
    import lvgpu.wal as LW
    rng = np.random.default_rng(15)
    sets = [random_records(rng, 300, maxlog=14), random_records(rng, 280, maxlog=15) + [b""] * 30]
    packed = [pack(r) for r in sets]
    want = [oracle_encode(r, 17 * i) for i, r in enumerate(sets)]
    pays = [to_dev(torch, p[0], gpu, 1 + i) for i, p in enumerate(packed)]
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    got = LW.encode_device(pays[0], packed[0][1], packed[0][2], 0, stream=s1)
    s1.synchronize()
    assert got.cpu().numpy().tobytes() == want[0]
    for streams in ((s1, s1), (s1, s2)):
        outs = []
        with torch.cuda.stream(streams[0]):  # allocations belong to the streams that use them
            bufs = [(torch.zeros(len(want[i]), dtype=torch.uint8, device=gpu),
                     torch.empty(LW.encode_workspace_bytes(LW.encode_size(packed[i][2], 17 * i)[1]), dtype=torch.uint8,
                                 device=gpu)) for i in range(2)]
        torch.cuda.synchronize()
        for i in range(2):
            outs.append(LW.encode_device(pays[i], packed[i][1], packed[i][2], 17 * i, out=bufs[i][0],
                                         workspace=bufs[i][1], stream=streams[i]))
        torch.cuda.synchronize()
        for i in range(2):
            assert first_diff(outs[i].cpu().numpy().tobytes(), want[i]) is None, (i, streams[0] is streams[1])


def test_round_trip_in_hbm(gpu):
    """encode_device -> scan_device on the same tensor: every physical record
    found and OK, each header's stored CRC unmasks to the scan's CRC of
    [type || payload], and a host Reader over the copied-back log returns the
    records."""
    import torch
    import lvgpu
    import lvgpu.wal as LW
    rng = np.random.default_rng(16)
    recs = [b"", b"foo"] + random_records(rng, 150) + [bytes(2 * B + 5), b""]
    payload, off, ln = pack(recs)
    need, frags = LW.encode_size(ln)
    log_t = LW.encode_device(to_dev(torch, payload, gpu, 3), off, ln)
    assert log_t.numel() == need and log_t.data_ptr() % 8 == 0
    hdr, crc, info, count = LW.scan_device(log_t, frags + 8)
    torch.cuda.synchronize()
    assert int(count.item()) == frags
    log = log_t.cpu().numpy().tobytes()
    info = info.cpu().numpy().view(np.uint32)[:frags]
    crc = crc.cpu().numpy().view(np.uint32)[:frags]
    hdr = hdr.cpu().numpy()[:frags]
    assert ((info >> 8) & 0xFF == LW.REC_OK).all()
    assert hdr.tolist() == [p for p, _, _ in W.wal_physical_records(log)]
    for p, c in zip(hdr.tolist(), crc.tolist()):
        assert lvgpu.unmask(W.decode_fixed_32(log[p:p + 4])) == c, p
    rd = LW.Reader(log, LW.Scan.from_arrays(hdr.astype(np.uint64), crc, info))
    back = []
    while (r := rd.read_record()) is not None:
        back.append(r)
    assert back == recs
