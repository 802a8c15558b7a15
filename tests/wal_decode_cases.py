"""Logs, corruptions and comparison helpers shared by the WAL decode tests
(test_gpu_wal_decode_device.py, test_gpu_wal_decode_stress.py).  The reference
for every record, offset and report is oracle/wal_oracle.py's Reader with a
ReportCollector, checksum on, initial_offset 0; the in-repo host Reader over the
very scan arrays fed to the decode is the second yardstick."""
import numpy as np

import wal_oracle as W
from wal_encode_cases import B, H, oracle_encode, random_records, to_dev

CANARY = 0xA5
CANARY64 = int.from_bytes(bytes([CANARY]) * 8, "little", signed=True)
CANARY32 = int.from_bytes(bytes([CANARY]) * 4, "little", signed=True)
GUARD = 64


class ListCollector(W.ReportCollector):
    """A ReportCollector that also keeps each (bytes, reason) in order."""

    def __init__(self):
        super().__init__()
        self.items = []

    def corruption(self, nbytes, reason):
        super().corruption(nbytes, reason)
        self.items.append((int(nbytes), reason))


def oracle_read(log, checksum=True):
    """(records, last_record_offset after each, reports, dropped bytes)."""
    rep = ListCollector()
    rd = W.Reader(W.StringSource(log), rep, checksum, 0)
    recs, offs = [], []
    while (r := rd.read_record()) is not None:
        recs.append(r)
        offs.append(rd.last_record_offset)
    return recs, offs, rep.items, rep.dropped_bytes


def host_read(log, hdr, crc, info, checksum=True):
    """The same through lvgpu.wal.Reader over Scan.from_arrays of these arrays."""
    import lvgpu.wal as LW
    rep = ListCollector()
    rd = LW.Reader(log, LW.Scan.from_arrays(hdr, crc, info), rep, checksum, 0)
    recs, offs = [], []
    while (r := rd.read_record()) is not None:
        recs.append(r)
        offs.append(rd.last_record_offset())
    return recs, offs, rep.items, rep.dropped_bytes


# ---- edits of a written log (the reference's fix_checksum, log_writer.rs tests) ----
def fix_checksum(log, pos):
    """Recomputes the header CRC of the physical record at pos, in place."""
    ln = log[pos + 4] | (log[pos + 5] << 8)
    log[pos:pos + 4] = W.encode_fixed_32(W.mask(W.value(bytes(log[pos + 6:pos + 7 + ln]))))


def set_type(log, pos, t):
    log[pos + 6] = t
    fix_checksum(log, pos)


def set_length(log, pos, ln):
    """Edits the length field only (the stored CRC is left as it was)."""
    log[pos + 4], log[pos + 5] = ln & 0xFF, ln >> 8


def flip(log, pos):
    log[pos] ^= 0x40


def headers(log):
    """(offset, length, type) of every physical record of a well-formed log."""
    return W.wal_physical_records(bytes(log))


def first_of_type(log, t, nth=0):
    return [p for p, _, ty in headers(log) if ty == t][nth]


def corrupt(rng, log):
    """0 to 3 random corruptions of a written log: a byte flip, a type edit
    with the checksum fixed, a length edit, a truncation."""
    log = bytearray(log)
    for _ in range(int(rng.integers(0, 4))):
        hs = headers(log)
        if not log or not hs:
            break
        kind = int(rng.integers(0, 4))
        p, ln, _ = hs[int(rng.integers(0, len(hs)))]
        if kind == 0:
            flip(log, int(rng.integers(0, len(log))))
        elif kind == 1:
            set_type(log, p, int(rng.integers(0, 7)))
        elif kind == 2:
            new = [0, 1, max(ln - 1, 0), ln + 1, B, 0xFFFF, int(rng.integers(0, 1 << 16))][int(rng.integers(0, 7))]
            set_length(log, p, new)
            if rng.random() < 0.5 and p + H + new <= len(log):
                fix_checksum(log, p)
        else:
            cut = [p + int(rng.integers(0, H + ln + 1)), int(rng.integers(0, len(log) + 1)),
                   (len(log) // B) * B][int(rng.integers(0, 3))]
            del log[cut:]
    return bytes(log)


# ---- GPU side ----
class Run:
    """One scan_device + decode_device of a log: the Decoded, the payload's
    guarded buffer and, after collect(), the scan arrays on the host."""


def run_decode(torch, dev, log, *, checksum=True, pay_shift=0, cap=None, rec_cap=None, rep_cap=None,
               payload_cap=None, reports=True, stream=None, null_crc=False):
    """Scans and decodes `log` on the GPU.  Output tensors are filled with the
    canary first and the payload lies between two guards at the byte alignment
    pay_shift.  Returns a Run with the Decoded (.dec), the scan arrays as numpy
    (.hdr / .crc / .info, .count) and helpers' inputs."""
    import lvgpu.wal as LW
    r = Run()
    d_log = to_dev(torch, log, dev, 0)
    want_cap = len(W.scan_log(log)[0]) + 3 if cap is None else cap
    hdr, crc, info, count = LW.scan_device(d_log, want_cap, stream=stream)
    scan_cap = want_cap
    need = len(log) if payload_cap is None else payload_cap
    buf = torch.full((need + 2 * GUARD + 32,), CANARY, dtype=torch.uint8, device=dev)
    base = (-buf.data_ptr()) % 16 + pay_shift + GUARD
    payload = buf[base:base + need]
    r.dec = LW.decode_device(d_log, hdr[:scan_cap], None if null_crc else crc[:scan_cap], info[:scan_cap], count,
                             checksum=checksum, payload=payload, stream=stream, reports=reports, rec_cap=rec_cap,
                             rep_cap=rep_cap, scan_cap=scan_cap, fill=CANARY)
    r.buf, r.base, r.need = buf, base, need
    r.d = (hdr, crc, info, count)
    return r


def collect(torch, r):
    """Synchronises and copies the scan arrays back (.hdr, .crc, .info)."""
    torch.cuda.synchronize()
    hdr, crc, info, count = r.d
    n = int(count.item())
    r.count = n
    n = min(n, hdr.numel())
    r.hdr = hdr.cpu().numpy()[:n].astype(np.uint64)
    r.crc = crc.cpu().numpy().view(np.uint32)[:n]
    r.info = info.cpu().numpy().view(np.uint32)[:n]
    r.host = r.buf.cpu().numpy()
    return r


def guards_ok(r, used):
    h = r.host
    return bool((h[:r.base] == CANARY).all() and (h[r.base + used:] == CANARY).all())


def untouched(torch, dec):
    """True if every output but the totals still holds the canary."""
    ok = bool((dec.payload == CANARY).all())
    for t in (dec.rec_off, dec.rec_len, dec.rec_log_off, dec.rep_bytes, dec.rep_log_off):
        if t is not None:
            ok = ok and bool((t == CANARY64).all())
    if dec.rep_reason is not None:
        ok = ok and bool((dec.rep_reason == CANARY32).all())
    return ok


def check(torch, dev, log, *, checksum=True, pay_shift=0, null_crc=False, tag=""):
    """The whole comparison of one log: records, rec_log_off, reports in order,
    totals -- against the oracle Reader and against the host Reader over the
    scan arrays the decode was fed -- and the payload's guards."""
    log = bytes(log)
    r = collect(torch, run_decode(torch, dev, log, checksum=checksum, pay_shift=pay_shift, null_crc=null_crc))
    want = oracle_read(log, checksum)
    host = host_read(log, r.hdr, r.crc, r.info, checksum)
    t = r.dec.sync_totals()
    got = (r.dec.records(), r.dec.record_log_offsets(), r.dec.reports(), t["dropped_bytes"])
    for name, ref in (("oracle", want), ("host reader", host)):
        assert got[2] == ref[2], (tag, name, "reports", got[2][:6], ref[2][:6])
        assert len(got[0]) == len(ref[0]), (tag, name, "records", len(got[0]), len(ref[0]))
        bad = [i for i, (a, b) in enumerate(zip(got[0], ref[0])) if a != b]
        assert not bad, (tag, name, "record", bad[0], len(got[0][bad[0]]), len(ref[0][bad[0]]))
        assert got[1] == ref[1], (tag, name, "rec_log_off")
        assert got[3] == ref[3], (tag, name, "dropped_bytes", got[3], ref[3])
    assert t["records"] == len(want[0]) and t["reports"] == len(want[2]), (tag, t)
    assert t["payload_bytes"] == sum(len(x) for x in want[0]) and t["status"] == 0, (tag, t)
    # the records lie end to end from 0
    off = r.dec.rec_off[: t["records"]].cpu().numpy()
    ln = r.dec.rec_len[: t["records"]].cpu().numpy()
    assert off.tolist() == ([0] + np.cumsum(ln).tolist()[:-1] if len(ln) else []), (tag, "rec_off")
    assert guards_ok(r, t["payload_bytes"]), (tag, "bytes outside d_payload[0, payload_bytes) were written")
    return r, want


# ---- logs ----
BIG = np.random.default_rng(7).integers(0, 256, size=70000, dtype=np.uint8).tobytes()
_ONE_A = oracle_encode([b"a"])  # 8 bytes: 4,096 of them fill a block exactly


def carry_log(p=0):
    """p + 5,000 one-byte records, the 70,000-byte record BIG (FIRST / MIDDLE /
    LAST over three blocks), 5,000 more one-byte records."""
    head = _ONE_A * (p + 5000)
    return head + oracle_encode([BIG] + [b"z"] * 5000, len(head))


def mixed_log(nblocks, seed=5):
    """At least nblocks blocks of mixed records: empty, tiny, and long ones."""
    rng = np.random.default_rng(seed)
    recs, tot = [], 0
    while tot < nblocks * B:
        recs += random_records(rng, 40, maxlog=16)
        recs += [b"", bytes([len(recs) & 0xFF]) * 3]
        tot = sum(len(x) + H for x in recs)
    return oracle_encode(recs)


def shape_cases():
    """(name, log): the shapes with nothing wrong in them."""
    from wal_encode_cases import EDGES, trailer_edge, writer_recipe
    rng = np.random.default_rng(21)
    mk = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    yield "empty", b""
    for n in range(1, 7):
        yield f"bytes{n}", bytes(range(1, n + 1))
    yield "one_empty_full", oracle_encode([b""])
    yield "ends_at_block_end", oracle_encode([mk(B - H)])
    yield "ends_at_block_end_then_more", oracle_encode([mk(100), mk(B - 2 * H - 100), b"next", mk(5000)])
    for e in EDGES:
        # the Writer's records for a log that already holds e bytes, behind a filler of that size
        pre = e % B
        filler = [mk(pre - H)] if pre >= H else []
        if pre and not filler:
            continue  # 1..6 existing bytes cannot be stood in for by a record
        yield f"recipe_edge{e}", oracle_encode(filler + writer_recipe(e))
        for k in range(9):
            yield f"trailer_edge{e}_{k}", oracle_encode(filler + trailer_edge(k, e))
    yield "two_blocks", oracle_encode([b"x", mk(B + 100), b"y"])
    yield "three_blocks", oracle_encode([mk(17), mk(2 * B + 100), b"", mk(3 * B + 5)])
    log = oracle_encode([mk(1000)] * 40 + [mk(B)])
    pad = (-len(log)) % B
    yield "multiple_of_block", (log + oracle_encode([mk(pad - H)], len(log)) if pad >= H else log[: len(log) - len(log) % B])


def reason_cases():
    """(name, log, reasons that must appear): every report reason at least
    once, and the silent ends."""
    rng = np.random.default_rng(22)
    mk = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    base = lambda: bytearray(oracle_encode([mk(300), mk(2 * B + 500), mk(40), b"", mk(B + 9), mk(77)]))
    for t, name in ((W.FULL, "full"), (W.FIRST, "first"), (W.MIDDLE, "middle"), (W.LAST, "last")):
        log = base()
        flip(log, first_of_type(log, t) + H + 3)
        yield f"mismatch_{name}", log, ["checksum mismatch"]
    # a mismatch in the first record of a block with good records after it: they
    # are dropped with it, and the next block resumes
    log = bytearray(oracle_encode([mk(200)] * 400))
    assert len(log) > 2 * B
    second = [p for p, _, _ in headers(log) if p >= B][0]
    flip(log, second + H)
    yield "mismatch_first_of_block", log, ["checksum mismatch"]
    log = base()
    set_length(log, first_of_type(log, W.FULL, 0), B)  # mid-file: the first block is whole
    yield "bad_length_mid_file", log, ["bad record length"]
    log = base()
    set_length(log, [p for p, _, _ in headers(log)][-1], 5000)  # in the short final block: silent
    yield "bad_length_final_block", log, []
    log = base()
    yield "truncated_header", bytes(log) + b"\x01\x02\x03", []
    yield "truncated_header_6", bytes(log) + bytes(6), []
    yield "first_without_last_at_end", oracle_encode([mk(50), mk(B)])[:B], []
    # ... and with its LAST cut short in the final block: a bad length at the end of the file, silent too
    yield "open_record_then_truncated_last", oracle_encode([mk(50), mk(B)])[: B + 100], []
    # FULL / FIRST inside an open record
    log = base()
    set_type(log, first_of_type(log, W.MIDDLE), W.FULL)
    yield "full_in_open_record", log, ["partial record without end(1)"]
    log = base()
    set_type(log, first_of_type(log, W.MIDDLE), W.FIRST)
    yield "first_in_open_record", log, ["partial record without end(2)"]
    log = base()
    set_type(log, first_of_type(log, W.FIRST), W.MIDDLE)
    yield "middle_without_start", log, ["missing start of fragmented record(1)"]
    log = base()
    set_type(log, first_of_type(log, W.FULL, 1), W.LAST)
    yield "last_without_start", log, ["missing start of fragmented record(2)"]
    log = base()
    set_type(log, first_of_type(log, W.FULL, 1), 0)  # 40 bytes: type 0 with length > 0
    yield "type0_with_length", log, ["unexpected record type"]
    log = base()
    set_type(log, first_of_type(log, W.MIDDLE), 0)  # inside an open record
    yield "type0_in_open_record", log, ["unexpected record type"]
    log = base()
    set_type(log, first_of_type(log, W.FULL, 1), 5)  # the Reader's own Eof code: it stops there, silently
    yield "type5", log, []
    log = base()
    set_type(log, first_of_type(log, W.MIDDLE), 5)
    yield "type5_in_open_record", log, []
    log = base()
    set_type(log, first_of_type(log, W.MIDDLE), 6)  # its BadRecord code: the block is read on
    yield "type6_in_open_record", log, ["error in middle of record"]
    log = base()
    set_type(log, first_of_type(log, W.FULL, 0), 7)
    yield "type7", log, ["unknown record type"]
    log = base()
    set_type(log, first_of_type(log, W.LAST), 200)
    yield "type200_in_open_record", log, ["unknown record type"]
    # a ZERO entry in mid-block: the rest of the block is dropped without a report
    log = bytearray(oracle_encode([mk(100), b"", mk(100), mk(B - 2 * (100 + H) - 2 * H), mk(10), mk(B + 3)]))
    p = [p for p, ln, _ in headers(log) if ln == 0][0]
    log[p + 6] = 0
    yield "zero_mid_block", log, []
    # a kill inside an open record: two reports from one entry
    log = base()
    flip(log, first_of_type(log, W.LAST) + H + 1)
    yield "mismatch_closes_open_record", log, ["checksum mismatch", "error in middle of record"]
    log = base()
    set_length(log, first_of_type(log, W.LAST, 1), B)
    log += oracle_encode([mk(B)], len(log))  # so the bad length is not in the final block
    yield "bad_length_in_open_record", log, ["bad record length", "error in middle of record"]


STRESS_TRIALS = 300


def stress_log(seed):
    """The log of one stress trial: random records (a few trials run to
    ~2 MiB, most stay under 100 KiB) with 0 to 3 random corruptions."""
    rng = np.random.default_rng(1000 + seed)
    if seed % 50 == 0:
        recs = random_records(rng, 200, maxlog=17)  # cut at 2 MiB
    else:
        recs = random_records(rng, int(rng.integers(1, 40)), maxlog=int(rng.integers(3, 15)))
        if rng.random() < 0.3:
            recs += [b""] * int(rng.integers(1, 50))
    log = oracle_encode(recs)[: 2 << 20]
    return corrupt(rng, log)
