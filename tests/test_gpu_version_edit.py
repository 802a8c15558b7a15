"""lv_version_edit_decode_device, lv_version_edit_encode_device and
lv_version_edit_files_device on the GPU, byte for byte and canary for canary
against the serial model (tests/version_edit_cases.py), at the smallest shapes
at which the kernels can go wrong.  Every output is canary-filled and guarded,
every workspace dirty."""
import gc

import numpy as np
import pytest

import lvgpu.version_edit as VE
import positions64_cases as P64
import version_edit_cases as C
from positions64_cases import HI

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA7, 64
M64 = C.M64
T = VE.VD_TILE
DEL = bytes.fromhex("060209")  # the three-byte record: deleted (2, 9)


# ---- helpers ---------------------------------------------------------------------
def dev_bytes(torch, gpu, b, shift=0):
    """`b` on the device at byte alignment `shift` (allocations are 256-B aligned)."""
    buf = torch.full((shift + max(len(b), 1) + 16,), 0x3C, dtype=torch.uint8, device=gpu)
    if len(b):
        buf[shift:shift + len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return buf[shift:shift + len(b)]


def dev_i64(torch, gpu, a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64)
    return torch.from_numpy(a.copy()).to(gpu) if a.size else torch.zeros(0, dtype=torch.int64, device=gpu)


def dev_rows(torch, gpu, a):
    """A structured array as a uint8 tensor (at least 16 bytes, so it has a pointer)."""
    raw = np.frombuffer(a.tobytes() + bytes(16), dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(gpu)


def dirty(torch, gpu, nbytes):
    return torch.full((max(nbytes, 16),), 0x5A, dtype=torch.uint8, device=gpu)


def tail_is_canary(t, used_bytes):
    import torch
    return bool((t.view(torch.uint8)[used_bytes:] == CANARY).all())


def run_decode(torch, gpu, payload, rec_off, rec_len, *, shift=0, caps=None, records=None, rec_cap=None, upstream=None):
    n = len(rec_off)
    d = VE.decode_device(dev_bytes(torch, gpu, payload, shift), dev_i64(torch, gpu, rec_off), dev_i64(torch, gpu, rec_len),
                         dev_i64(torch, gpu, [n if records is None else records]),
                         None if upstream is None else dev_i64(torch, gpu, [upstream]),
                         rec_cap=n if rec_cap is None else rec_cap, caps=caps,
                         workspace=dirty(torch, gpu, VE.decode_workspace_bytes(n if rec_cap is None else rec_cap)),
                         fill=CANARY, guard=GUARD)
    return d


def untouched(d):
    return all(tail_is_canary(t, 0) for t in (d.edits_t, d.files_t, d.deleted_t, d.pointers_t, d.rec_file, d.rec_deleted,
                                              d.rec_pointer))


def check_decode(torch, gpu, payload, rec_off, rec_len, *, shift=0, want=None, tag=""):
    """The decode with exactly the model's capacities, everything compared."""
    want = want or C.decode_batch(payload, rec_off, rec_len)
    edits, F, D, Pt, bounds, tot = want
    d = run_decode(torch, gpu, payload, rec_off, rec_len, shift=shift, caps=(len(F), len(D), len(Pt)))
    assert d.sync_totals() == tot, tag
    assert d.edits().tobytes() == edits.tobytes(), tag
    assert d.files().tobytes() == F.tobytes() and d.deleted().tobytes() == D.tobytes(), tag
    assert d.pointers().tobytes() == Pt.tobytes(), tag
    for got, w in zip(d.bounds(), bounds):
        assert np.array_equal(got, w), tag
    n = len(rec_off)
    assert tail_is_canary(d.edits_t, 64 * n) and tail_is_canary(d.files_t, 48 * len(F)), tag
    assert tail_is_canary(d.deleted_t, 16 * len(D)) and tail_is_canary(d.pointers_t, 16 * len(Pt)), tag
    assert all(tail_is_canary(b, 8 * (n + 1)) for b in (d.rec_file, d.rec_deleted, d.rec_pointer)), tag
    return d, want


def run_encode(torch, gpu, t, *, shift=0, records=None, rec_cap=None, caps=None, out_cap=None, out_shift=0, upstream=None):
    src, E, F, bf, D, bd, Pt, bp = t
    n = len(E)
    rec_cap = n if rec_cap is None else rec_cap
    caps = (len(F), len(D), len(Pt)) if caps is None else caps
    out = None
    if out_cap is not None:
        buf = torch.full((out_shift + out_cap + GUARD + 16,), CANARY, dtype=torch.uint8, device=gpu)
        out = buf[out_shift:]
    e = VE.encode_device(dev_bytes(torch, gpu, src, shift), dev_rows(torch, gpu, E), dev_rows(torch, gpu, F),
                         dev_i64(torch, gpu, bf), dev_rows(torch, gpu, D), dev_i64(torch, gpu, bd), dev_rows(torch, gpu, Pt),
                         dev_i64(torch, gpu, bp), dev_i64(torch, gpu, [n if records is None else records]),
                         None if upstream is None else dev_i64(torch, gpu, [upstream]), rec_cap=rec_cap, caps=caps,
                         out=out, out_cap=out_cap,
                         workspace=dirty(torch, gpu, VE.encode_workspace_bytes(rec_cap, *caps)), fill=CANARY, guard=GUARD)
    if out is not None:
        e._buf = buf
    return e


def check_encode(torch, gpu, t, *, shift=0, out_shift=0, tag=""):
    """The encode with exactly the model's out_cap, everything compared."""
    src = t[0]
    out, ro, rl, tot = C.encode_batch(len(src), *t[1:], src=src)
    assert tot["status"] == 0
    e = run_encode(torch, gpu, t, shift=shift, out_cap=tot["out_bytes"], out_shift=out_shift)
    assert e.sync_totals() == tot, tag
    host = e._buf.cpu().numpy()
    assert host[out_shift:out_shift + len(out)].tobytes() == out, tag
    assert (host[:out_shift] == CANARY).all() and (host[out_shift + len(out):] == CANARY).all(), tag
    assert np.array_equal(e.rec_off(), np.array(ro, dtype=np.uint64)), tag
    assert np.array_equal(e.rec_len(), np.array(rl, dtype=np.uint64)), tag
    n = len(t[1])
    assert tail_is_canary(e.rec_off_t, 8 * n) and tail_is_canary(e.rec_len_t, 8 * n), tag
    return e, out


def long_record(rows=900, key=9):
    """A wave-class record: beyond kVdSmall bytes, more than 64 rows of each kind."""
    e = C.new_edit(comparator=b"c" * 40, log_number=1 << 40, last_sequence=5,
                   pointers=[(k % 7, bytes([k & 255]) * (key + k % 5)) for k in range(rows // 4)],
                   deleted=sorted((k % 7, (1 << 63) + k) for k in range(rows)),
                   files=[(k % 7, k, k << 20, bytes([k & 255]) * (key + k % 3), b"z" * key) for k in range(rows // 3)])
    b = C.encode_to(e)
    if len(b) <= VE.VD_SMALL:  # the comparator makes up the length
        e["comparator"] = b"c" * (VE.VD_SMALL + 100 - len(b))
        b = C.encode_to(e)
    assert len(b) > VE.VD_SMALL
    return b


# ---- decode -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [T - 1, T, T + 1, 64 * T + 1, 2 * 64 * T + 1])
def test_decode_record_counts_around_the_tiles(gpu, n):
    """Three-byte records around the count tile and the carry's second and third round."""
    import torch
    payload = DEL * n
    off = np.arange(n, dtype=np.uint64) * np.uint64(3)
    ln = np.full(n, 3, dtype=np.uint64)
    ED, FD, DD, PD = C._dtypes()
    edits = np.zeros(n, dtype=ED)
    D = np.zeros(n, dtype=DD)
    D["number"], D["level"] = 9, 2
    ar = np.arange(n + 1, dtype=np.uint64)
    zero = np.zeros(n + 1, dtype=np.uint64)
    tot = dict(records=n, files=0, deleted=n, pointers=0, bad_records=0, first_bad=n, status=0,
               **{f"last_has{b}": 0 for b in range(5)})
    if n <= T + 1:  # the closed form is the model's
        m = C.decode_batch(payload, off, ln)
        assert m[5] == tot and m[2].tobytes() == D.tobytes() and np.array_equal(m[4][1], ar)
    check_decode(torch, gpu, payload, off, ln, want=(edits, np.zeros(0, dtype=FD), D, np.zeros(0, dtype=PD), (zero, ar, zero), tot))


def test_decode_lengths_either_side_of_the_class_boundary(gpu):
    """Records of kVdSmall - 1, kVdSmall, kVdSmall + 1 bytes and a long one with
    rows of every kind, among small ones: lane and wave walks in one wave."""
    import torch
    recs = [C.encode_to(e) for e in C.random_edits(21, 5)]
    for extra in (-1, 0, 1, 40):
        e = C.new_edit(log_number=7, pointers=[(1, b"k" * 9)], deleted=[(3, 4)], files=[(2, 1, 2, b"a" * 8, b"b" * 10)])
        pad = VE.VD_SMALL + extra - len(C.encode_to(e)) - 3  # tag, two length bytes
        e["comparator"] = b"p" * pad
        b = C.encode_to(e)
        assert len(b) == VE.VD_SMALL + extra
        recs.append(b)
    recs += [long_record(), C.encode_to(C.example_edit()), long_record(300, key=3)]
    payload, off, ln = C.lay_out(recs, gap=3)
    _, want = check_decode(torch, gpu, payload, off, ln, shift=5)
    assert want[5]["bad_records"] == 0 and want[5]["files"] > 400 and sum(l > VE.VD_SMALL for l in ln) == 4


def just_wave_class(k, bad=False):
    """A record of kVdSmall + 1 bytes with more than 64 rows: the wave class by
    one byte.  Good: rows of every kind behind a comparator that makes up the
    length.  bad: 65 deleted rows, an unknown tag, then zeros."""
    if bad:
        b = C.encode_to(C.new_edit(deleted=sorted((j % 7, 1000 * k + j) for j in range(65)))) + bytes([8])
        return b + bytes(VE.VD_SMALL + 1 - len(b))
    e = C.new_edit(log_number=k, last_sequence=1 << (20 + k % 40),
                   pointers=[(j % 7, bytes([j + k & 255]) * (8 + j % 3)) for j in range(30 + k % 5)],
                   deleted=sorted((j % 7, (k << 32) + j) for j in range(70)),
                   files=[(j % 7, j, (j + k) << 12, bytes([j & 255]) * (8 + j % 4), b"y" * 9) for j in range(25)])
    e["comparator"] = b"w" * (VE.VD_SMALL + 1 - len(C.encode_to(e)) - 3)  # tag, two length bytes
    b = C.encode_to(e)
    assert len(b) == VE.VD_SMALL + 1
    return b


def test_decode_wave_dispatch(gpu):
    """One wave's 64 records with the wave class at lanes 0, 1, 31 and 63 among
    lane-class records of a few rows, record 31 failing after its 65th row; then
    the rest of the tile, and a second tile whose only record is wave class: a
    wave with one large record and 63 absent ones.  Each lane must keep its own
    walk's result and lane b the wave's."""
    import torch
    recs = [C.encode_to(e) for e in C.random_edits(77, T, max_rows=3)]
    for i in (0, 1, 63):
        recs[i] = just_wave_class(i + 1)
    recs[31] = just_wave_class(31, bad=True)
    recs.append(just_wave_class(200))
    assert len(recs) == T + 1 and [i for i, r in enumerate(recs) if len(r) > VE.VD_SMALL] == [0, 1, 31, 63, T]
    payload, off, ln = C.lay_out(recs, gap=1, lead=2)
    _, want = check_decode(torch, gpu, payload, off, ln, shift=7)
    edits, F, D, Pt, bounds, tot = want
    assert int(edits[31]["status"]) == C.UNKNOWN_TAG and tot["first_bad"] == 31 and tot["bad_records"] == 1
    assert [int(np.diff(bounds[1])[i]) for i in (0, 1, 31, 63, T)] == [70, 70, 0, 70, 70]
    assert [int(np.diff(bounds[0])[i]) for i in (0, 1, 31, 63, T)] == [25, 25, 0, 25, 25]


@pytest.mark.parametrize("shift", range(16))
def test_decode_payload_alignments_and_window_edges(gpu, shift):
    """Every payload alignment; a wave-class record of 12-byte deleted rows whose
    ten-byte varints straddle the edges of the LDS window; a key longer than two
    windows behind a first round's worth of rows."""
    import torch
    rows = C.encode_to(C.new_edit(deleted=sorted((k % 7, M64 - k) for k in range(1500))))
    assert len(rows) == 12 * 1500 > VE.VD_SMALL and len(rows) % 16 == 0
    rows6 = C.encode_to(C.new_edit(log_number=1 << 30)) + rows  # the same rows, six bytes on
    assert len(rows6) == len(rows) + 6
    big_key = C.encode_to(C.new_edit(pointers=[(1, b"q" * 5)] * 70 + [(2, bytes(range(256)) * 40)] + [(3, b"r" * 8)] * 70,
                                     files=[(0, 1, 2, b"s" * (2 * VE.VD_WINDOW + 77), b"t" * 8), (1, 3, 4, b"", b"u" * 9)]))
    recs = [C.encode_to(e) for e in C.random_edits(shift, 6)] + [rows, big_key, rows6]
    payload, off, ln = C.lay_out(recs, lead=1)
    # a ten-byte varint lies across the first window's end in one of the two, whatever the alignment

    def straddles(at, first):
        lo = (shift + at) & ~15
        return any(shift + at + first + 12 * k + 2 - lo < VE.VD_WINDOW <= shift + at + first + 12 * k + 11 - lo
                   for k in range(1500))
    assert straddles(off[6], 0) or straddles(off[8], 6)
    _, want = check_decode(torch, gpu, payload, off, ln, shift=shift)
    assert int(want[0][7]["status"]) == 0 and want[5]["pointers"] >= 141


def test_decode_statuses_order_and_extents(gpu):
    """Empty records first, last and in a run; records out of order, overlapping
    and out of range; every status; first_bad and last_has with a bad record in
    the middle."""
    import torch
    ex = C.encode_to(C.example_edit())
    pieces = [ex] + [bytes.fromhex(h) for h in C.STATUS_RECORDS.values()] + [bytes.fromhex(h) for h, _, _ in C.QUIRKS]
    payload, off, ln = C.lay_out(pieces, gap=2)
    n0 = len(payload)
    # (off, len): empties first / in a run / last, out of order, overlapping (a suffix of the example), out of range
    recs = [(0, 0), (off[1], ln[1]), (off[0], ln[0]), (7, 0), (9, 0), (n0, 0), (off[0] + 5, ln[0] - 5), (off[0], ln[0])]
    recs += [(off[k], ln[k]) for k in range(len(pieces) - 1, 0, -1)]
    recs += [(n0 + 1, 0), (n0 - 2, 3), (M64, 1), (1, M64), (off[0], ln[0]), (n0, 0)]
    ro, rl = [r[0] for r in recs], [r[1] for r in recs]
    _, want = check_decode(torch, gpu, payload, ro, rl, shift=3)
    st = [int(s) for s in want[0]["status"]]
    assert set(st) == set(range(8)) and st[:8] == [0] * 8 and st[-6:-2] == [C.OUT_OF_RANGE] * 4
    tot = want[5]
    # record 8 is the last quirk (a log number alone), record 9 the first bad one; the example at 7 carries every bit
    assert tot["first_bad"] == 9 == st.index(C.BAD_LENGTH) and tot["bad_records"] > 10
    assert [tot[f"last_has{b}"] for b in range(5)] == [8, 9, 8, 8, 8]
    # a clean batch: first_bad = records, and last_has follows the last carrier
    good = [ex, b"", bytes.fromhex("0203"), bytes.fromhex("0405"), b""]
    payload, off, ln = C.lay_out(good)
    _, want = check_decode(torch, gpu, payload, off, ln)
    assert want[5]["first_bad"] == 5 and [want[5][f"last_has{b}"] for b in range(5)] == [1, 3, 1, 1, 4]


def test_decode_status_bits(gpu):
    """Each overflow bit alone with the true totals, UPSTREAM and REC_OVER: only
    the totals are written."""
    import torch
    recs = [C.encode_to(e) for e in C.random_edits(33, 300, max_rows=3)] + [bytes.fromhex("08")]
    payload, off, ln = C.lay_out(recs)
    *_, tot = C.decode_batch(payload, off, ln)
    full = (tot["files"], tot["deleted"], tot["pointers"])
    assert min(full) > 100 and tot["bad_records"] == 1
    for k, bit in enumerate((4, 8, 16)):
        caps = tuple(c - (1 if j == k else 0) for j, c in enumerate(full))
        d = run_decode(torch, gpu, payload, off, ln, caps=caps)
        assert d.sync_totals(check=False) == dict(tot, status=bit) and untouched(d)
    d = run_decode(torch, gpu, payload, off, ln, caps=(0, 0, 0))
    assert d.sync_totals(check=False) == dict(tot, status=28) and untouched(d)
    zero = {k: 0 for k in tot}
    d = run_decode(torch, gpu, payload, off, ln, caps=full, upstream=9)
    assert d.sync_totals(check=False) == dict(zero, status=1) and untouched(d)
    d = run_decode(torch, gpu, payload, off, ln, caps=full, records=len(off) + 1)
    assert d.sync_totals(check=False) == dict(zero, records=len(off) + 1, status=2) and untouched(d)
    # fewer records than the capacity: the rest of the arrays is not looked at
    d = run_decode(torch, gpu, payload, off, ln, caps=full, records=10)
    w = C.decode_batch(payload, off[:10], ln[:10])
    assert d.sync_totals() == w[5] and d.files().tobytes() == w[1].tobytes() and tail_is_canary(d.edits_t, 640)
    # no records at all
    d = run_decode(torch, gpu, b"", [], [], caps=(0, 0, 0))
    assert d.sync_totals() == dict(zero) and [int(b[0]) for b in d.bounds()] == [0, 0, 0]


# ---- encode -----------------------------------------------------------------------
@pytest.mark.parametrize("rows", [VE.VE_TILE - 2, VE.VE_TILE - 1, VE.VE_TILE, 64 * VE.VE_TILE + 1, 2 * 64 * VE.VE_TILE + 1])
def test_encode_item_counts_around_the_tiles(gpu, rows):
    """Deleted rows (with cap + 1 slots) around the scan tile and the carry's
    second and third round, over a few records with leading rows."""
    import torch
    cuts = sorted({0, 1, rows // 3, rows // 3, rows - 1, rows})
    edits = []
    for a, b in zip([0] + cuts, cuts + [rows]):
        edits.append(C.new_edit(deleted=[(k >> 16, k) for k in range(a, b)], next_file_number=b))
    edits[1]["pointers"] = [(1, b"x" * 70)]
    edits[-1]["files"] = [(6, 1, 2, b"y" * 9, b"z" * 100)]
    t = C.tables_of(edits, lead=(1, 1 if rows < 70000 else 0, 1))
    check_encode(torch, gpu, t)


def test_encode_record_counts_around_the_tile(gpu):
    import torch
    for n in (VE.VE_TILE - 1, VE.VE_TILE, VE.VE_TILE + 1):
        edits = [C.new_edit(log_number=k) if k % 3 else C.new_edit() for k in range(n)]
        edits[n // 2]["files"] = [(1, 2, 3, b"k" * 8, b"l" * 8)]
        check_encode(torch, gpu, C.tables_of(edits), tag=f"n={n}")


@pytest.mark.parametrize("shift", [0, 1, 7, 15])
def test_encode_copy_classes_and_alignments(gpu, shift):
    """Every class of lvk::group_copy (a lane's own copy below kVeWaveCopy, a
    group's with ragged heads and tails, more jobs than groups) at source and
    destination alignments."""
    import torch
    W = VE.VE_WAVE_COPY
    lens = [0, 1, 15, 16, W - 1, W, W + 1, W + 15, W + 16, 200, 1000, 5000]
    key = lambda n, s: bytes((s + 7 * i) & 255 for i in range(n))
    edits = [C.new_edit(comparator=key(n, 1), pointers=[(n % 7, key(n, 2))],
                        files=[(3, n, n, key(n, 3), key(lens[-1 - i], 4))]) for i, n in enumerate(lens)]
    edits += C.random_edits(shift, 20, max_key=100)
    for out_shift in (0, 3, 13):
        check_encode(torch, gpu, C.tables_of(edits, lead=(2, 0, 1)), shift=shift, out_shift=out_shift,
                     tag=f"{shift}/{out_shift}")


def test_encode_every_status_in_its_order(gpu):
    """One input with every fault at once; each bit is reported alone, in the
    header's order, as the faults before it are mended.  Then OUT_OVER and the
    retry with the size it reported."""
    import torch
    edits = C.random_edits(44, 8, max_rows=3)
    edits[5]["deleted"] = [(1, 5), (2, 3)]
    edits[6]["pointers"] = [(1, b"pointerkey")]
    good = C.tables_of(edits, lead=(1, 1, 1))
    want = C.encode_batch(len(good[0]), *good[1:], src=good[0])
    none = dict(files=0, deleted=0, pointers=0, key_bytes=0, out_bytes=0, bad_record=M64, bad_kind=M64, bad_row=M64)

    def faulty(bounds=True, rows=True):
        t = [np.array(x) if not isinstance(x, bytes) else x for x in good]
        if bounds:
            t[5][4], t[5][3] = t[5][3], t[5][4] + 1       # deleted bounds of record 3 out of order
            t[7][2] = len(t[6]) + 1                       # pointer bounds of record 1 beyond the capacity
        if rows:
            lo = int(good[5][5])
            t[4][lo + 1] = t[4][lo]                       # record 5: a duplicate deleted row
            t[6][int(good[7][6])]["level"] = 7            # record 6: a pointer's level
            t[1][7]["has"] |= 64                          # record 7: undefined has bits
        return t
    e = run_encode(torch, gpu, faulty(), upstream=3, records=99, out_cap=1)
    assert e.sync_totals(check=False) == dict(none, records=0, status=1)
    e = run_encode(torch, gpu, faulty(), records=99, out_cap=1)
    assert e.sync_totals(check=False) == dict(none, records=99, status=2)
    e = run_encode(torch, gpu, faulty(), out_cap=1)
    assert e.sync_totals(check=False) == dict(none, records=8, status=4, bad_record=1, bad_kind=VE.KIND_POINTER)
    t = faulty(bounds=False)
    for kind, row, rec in ((VE.KIND_EDIT, 7, 7), (VE.KIND_POINTER, int(good[7][6]), 6), (VE.KIND_DELETED, int(good[5][5]) + 1, 5)):
        e = run_encode(torch, gpu, t, out_cap=1)
        got = e.sync_totals(check=False)
        assert got == dict(none, records=8, status=8, bad_record=rec, bad_kind=kind, bad_row=row), got
        m = C.encode_batch(len(t[0]), *t[1:])[3]
        assert m == got
        assert tail_is_canary(e._buf, 0) and tail_is_canary(e.rec_off_t, 0) and tail_is_canary(e.rec_len_t, 0)
        if kind == VE.KIND_EDIT:
            t[1][7]["has"] &= 31
        elif kind == VE.KIND_POINTER:
            t[6][row]["level"] = 1
    short = want[3]["out_bytes"] - 1
    e = run_encode(torch, gpu, good, out_cap=short)
    got = e.sync_totals(check=False)
    assert got == dict(want[3], status=16) and tail_is_canary(e._buf, 0)
    e = run_encode(torch, gpu, good, out_cap=got["out_bytes"])
    assert e.sync_totals() == want[3] and e.out() == want[0]
    # extents outside the source, the comparator's and a file's
    for name, t, _, _ in C.damaged_encode_inputs():
        e = run_encode(torch, gpu, t, out_cap=16)
        assert e.sync_totals(check=False) == C.encode_batch(len(t[0]), *t[1:])[3], name


# ---- chains -----------------------------------------------------------------------
def test_chains_on_one_stream(gpu):
    """encode -> decode gives the same rows, and decode -> encode the same
    bytes, the counts and statuses handed on in device memory."""
    import torch
    edits = C.random_edits(55, 400, max_rows=4) + [C.example_edit()] + C.reference_test_edits()
    t = C.tables_of(edits, lead=(2, 1, 3))
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        e, out = check_encode(torch, gpu, t)
    assert out == b"".join(C.encode_to(x) for x in edits)
    with torch.cuda.stream(s):
        d = VE.decode_device(e.out_t[: len(out)], e.rec_off_t, e.rec_len_t, e.totals[0:1], e.totals[6:7],
                             rec_cap=len(edits), stream=s)
        e2 = VE.encode_device(e.out_t[: len(out)], d.edits_t, d.files_t, d.rec_file, d.deleted_t,
                              d.rec_deleted, d.pointers_t, d.rec_pointer, d.totals[0:1], d.totals[11:12],
                              rec_cap=len(edits), caps=d.caps, out_cap=len(out), stream=s, fill=CANARY, guard=GUARD)
    w = C.decode_batch(out, e.rec_off(), e.rec_len())
    assert d.sync_totals() == w[5] and w[5]["bad_records"] == 0
    assert d.files().tobytes() == w[1].tobytes() and d.deleted().tobytes() == w[2].tobytes()
    assert d.pointers().tobytes() == w[3].tobytes() and d.edits().tobytes() == w[0].tobytes()
    # the same rows: levels, numbers and key bytes are the input's
    src = t[0]
    for got, inp, keys in ((d.files(), t[2][2:], ("smallest", "largest")), (d.pointers(), t[6][3:], ("key",))):
        assert len(got) == len(inp) and np.array_equal(got["level"], inp["level"])
        for k in keys:
            assert np.array_equal(got[k + "_len"], inp[k + "_len"])
            assert all(out[int(a):int(a) + int(n)] == src[int(b):int(b) + int(n)]
                       for a, b, n in zip(got[k + "_off"], inp[k + "_off"], got[k + "_len"]))
    assert d.deleted().tobytes() == t[4][1:].tobytes()
    assert e2.sync_totals()["out_bytes"] == len(out) and e2.out() == out
    assert np.array_equal(e2.rec_off(), e.rec_off()) and np.array_equal(e2.rec_len(), e.rec_len())


def test_compaction_to_manifest_and_back(gpu):
    """lv_compact_output_device -> lv_version_edit_files_device -> encode, then
    the MANIFEST round trip lv_wal_encode_device -> lv_wal_scan_device ->
    lv_wal_decode_device -> decode: the file rows equal the compaction's files."""
    import torch
    import compact_output_cases as CO
    import lvgpu.wal as LW
    import sst_build_cases as S
    from memtable_cases import make_table
    payload, ops = make_table(S.seq_items(120, klen=5, vlen=7))
    out, w = CO.run_device(torch, gpu, payload, ops, 300, None, 48, 3, level=2, first_number=40)
    nf = w.totals["files"]
    assert 4 <= nf <= 40
    files_t, rec_file, status = VE.files_device(out.version_files_t, out.tables_t, out.totals[1:2], files_cap=nf)
    ED = VE.EDIT_DTYPE
    edit = np.zeros(1, dtype=ED)
    edit["next_file_number"], edit["has"] = 40 + nf, VE.HAS_NEXT_FILE
    none16 = torch.zeros(16, dtype=torch.uint8, device=gpu)
    zeros2 = torch.zeros(2, dtype=torch.int64, device=gpu)
    one = dev_i64(torch, gpu, [1])
    enc = VE.encode_device(out.bounds_t, dev_rows(torch, gpu, edit), files_t, rec_file, none16, zeros2, none16, zeros2,
                           one, status, rec_cap=1, caps=(nf, 0, 0), fill=CANARY, guard=GUARD)
    t = enc.sync_totals()
    assert int(status.cpu()[0]) == 0 and t["files"] == nf and t["records"] == 1
    bounds = bytes(5) + w.bounds  # the cursor began at 5
    model = C.new_edit(next_file_number=40 + nf,
                       files=[(2, v["number"], w.tables[k]["file_bytes"],
                               bounds[v["smallest_off"]:v["smallest_off"] + v["smallest_len"]],
                               bounds[v["largest_off"]:v["largest_off"] + v["largest_len"]]) for k, v in enumerate(w.vfiles)])
    record = C.encode_to(model)
    assert enc.out() == record and [int(x) for x in enc.rec_len()] == [len(record)]
    log = LW.encode_device(enc.out_t, enc.rec_off(), enc.rec_len())  # host extents: wal.h's rule
    aligned = torch.zeros((log.numel() + 7) & ~7, dtype=torch.uint8, device=gpu)[: log.numel()]
    aligned.copy_(log)
    hdr, crc, info, count = LW.scan_device(aligned, 8)
    dec = LW.decode_device(aligned, hdr, crc, info, count)
    d = VE.decode_device(dec.payload, dec.rec_off, dec.rec_len, dec.totals[0:1], dec.totals[4:5], rec_cap=8,
                         fill=CANARY, guard=GUARD)
    tot = d.sync_totals()
    assert tot["records"] == 1 and tot["files"] == nf and tot["bad_records"] == 0 and tot["last_has3"] == 1
    assert dec.records() == [record]
    got = d.files()
    assert [int(x) for x in got["number"]] == [v["number"] for v in w.vfiles]
    assert [int(x) for x in got["file_size"]] == [x["file_bytes"] for x in w.tables]
    assert set(int(x) for x in got["level"]) == {2}
    pay = dec.payload.cpu().numpy().tobytes()
    for g, f in zip(got, model["files"]):
        assert pay[int(g["smallest_off"]):int(g["smallest_off"]) + int(g["smallest_len"])] == f[3]
        assert pay[int(g["largest_off"]):int(g["largest_off"]) + int(g["largest_len"])] == f[4]
    assert int(d.edits()[0]["next_file_number"]) == 40 + nf
    # a failed file stops the encode: its status is the encode's upstream status
    bad_tables = out.tables_t.clone()
    bad_tables.view(torch.int64)[7] = 2  # tables[0].status
    _, _, st2 = VE.files_device(out.version_files_t, bad_tables, out.totals[1:2], files_cap=nf - 1)
    assert int(st2.cpu()[0]) == 2  # the failed file and the one beyond the capacity


def test_decode_then_encode_in_a_graph(gpu):
    """The decode -> encode chain (linear) captured once and replayed over
    other inputs of the same capacities."""
    import torch
    sets = []
    for seed in (0, 1, 2):
        recs = [C.encode_to(e) for e in C.random_edits(70 + seed, 300 + 20 * seed, max_rows=3)]
        recs[5] = long_record(200 + seed)
        sets.append(C.lay_out(recs))
    rcap, pcap = 400, max(len(s[0]) for s in sets) + 16
    caps = (pcap // 6, pcap // 3, pcap // 3)
    d_pay = torch.zeros(pcap, dtype=torch.uint8, device=gpu)
    d_off = torch.zeros(rcap, dtype=torch.int64, device=gpu)
    d_len = torch.zeros(rcap, dtype=torch.int64, device=gpu)
    d_n = torch.zeros(1, dtype=torch.int64, device=gpu)
    dws = torch.empty(VE.decode_workspace_bytes(rcap), dtype=torch.uint8, device=gpu)
    ews = torch.empty(VE.encode_workspace_bytes(rcap, *caps), dtype=torch.uint8, device=gpu)
    d_out = torch.zeros(pcap, dtype=torch.uint8, device=gpu)

    def load(k):
        payload, off, ln = sets[k]
        d_pay.fill_(0x11)
        d_pay[: len(payload)].copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
        d_off[: len(off)].copy_(dev_i64(torch, gpu, off))
        d_len[: len(ln)].copy_(dev_i64(torch, gpu, ln))
        d_n.fill_(len(off))

    def run(stream=None):
        d = VE.decode_device(d_pay, d_off, d_len, d_n, rec_cap=rcap, caps=caps, workspace=dws, stream=stream)
        e = VE.encode_device(d_pay, d.edits_t, d.files_t, d.rec_file, d.deleted_t, d.rec_deleted, d.pointers_t,
                             d.rec_pointer, d.totals[0:1], d.totals[11:12], rec_cap=rcap, caps=caps, out=d_out,
                             workspace=ews, stream=stream)
        return d, e

    def check(k, d, e):
        payload, off, ln = sets[k]
        torch.cuda.synchronize()
        d._tot = e._tot = None
        w = C.decode_batch(payload, off, ln)
        assert d.sync_totals() == w[5] and d.files().tobytes() == w[1].tobytes()
        assert e.sync_totals()["out_bytes"] == sum(ln) and e.out() == b"".join(payload[o:o + n] for o, n in zip(off, ln))

    load(0)
    check(0, *run())
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            d, e = run(s)
    torch.cuda.synchronize()
    for k in (1, 2, 0):
        load(k)
        d_out.fill_(0)
        dws.fill_(0x33)
        ews.fill_(0x44)
        torch.cuda.synchronize()
        g.replay()
        check(k, d, e)


# ---- positions beyond 4 GiB -----------------------------------------------------------
def _free(torch):
    gc.collect()
    torch.cuda.empty_cache()


def test_decode_payload_above_the_line(gpu):
    """Records on both sides of and across position 2^32 of d_payload; a
    position cut to 32 bits would read the decoy, other well-formed records."""
    import torch
    recs = [C.encode_to(e) for e in C.random_edits(81, 60, max_rows=3)] + [long_record(250)]
    decoy = [C.encode_to(e) for e in C.random_edits(82, 60, max_rows=3)] + [long_record(250, key=10)]
    payload, off, ln = C.lay_out(recs)
    other = b"".join(decoy)[: len(payload)].ljust(len(payload), b"\x00")
    cut = off[30] + 2
    t, base = P64.high_window(torch, gpu, payload, cut, other)
    w = C.decode_batch(payload, off, ln)
    d = VE.decode_device(t[: base + len(payload)], dev_i64(torch, gpu, P64.rebase(np.array(off, dtype=np.uint64), base)),
                         dev_i64(torch, gpu, ln), dev_i64(torch, gpu, [len(off)]),
                         caps=(w[5]["files"], w[5]["deleted"], w[5]["pointers"]),
                         workspace=dirty(torch, gpu, VE.decode_workspace_bytes(len(off))), fill=CANARY, guard=GUARD)
    assert d.sync_totals() == w[5] and w[5]["bad_records"] == 0
    F, Pt, E = d.files(), d.pointers(), d.edits()
    assert int(F["smallest_off"].max()) > HI > int(F["smallest_off"].min()) and base < HI < base + len(payload)
    for got, want, fields in ((F, w[1], ("smallest_off", "largest_off")), (Pt, w[3], ("key_off",)), (E, w[0], ("comparator_off",))):
        got = got.copy()
        for f in fields:
            mask = got[f] != 0 if f == "comparator_off" else np.ones(len(got), dtype=bool)
            got[f][mask] -= np.uint64(base)
        assert got.tobytes() == want.tobytes()
    assert d.deleted().tobytes() == w[2].tobytes()
    del d, t
    _free(torch)


def test_encode_source_above_the_line(gpu):
    """Comparator and key extents beyond 2^32 of d_src, one across the line; a
    position cut to 32 bits would copy the complement."""
    import torch
    edits = C.random_edits(91, 80, max_rows=3, max_key=60)
    src, E, F, bf, D, bd, Pt, bp = C.tables_of(edits)
    j = next(i for i in range(len(F) // 2, len(F)) if int(F[i]["largest_len"]) >= 8)
    cut = int(F[j]["largest_off"]) + 4  # inside a key
    out, ro, rl, tot = C.encode_batch(len(src), E, F, bf, D, bd, Pt, bp, src=src)
    t, base = P64.high_window(torch, gpu, src, cut, P64.complement(src))
    E2, F2, P2 = E.copy(), F.copy(), Pt.copy()
    E2["comparator_off"] += np.uint64(base)
    F2["smallest_off"] += np.uint64(base)
    F2["largest_off"] += np.uint64(base)
    P2["key_off"] += np.uint64(base)
    assert int(F2["largest_off"].max()) > HI > int(F2["largest_off"].min())
    e = VE.encode_device(t[: base + len(src)], dev_rows(torch, gpu, E2), dev_rows(torch, gpu, F2), dev_i64(torch, gpu, bf),
                         dev_rows(torch, gpu, D), dev_i64(torch, gpu, bd), dev_rows(torch, gpu, P2), dev_i64(torch, gpu, bp),
                         dev_i64(torch, gpu, [len(E)]), rec_cap=len(E), caps=(len(F), len(D), len(Pt)),
                         out_cap=tot["out_bytes"], fill=CANARY, guard=GUARD)
    assert e.sync_totals() == tot and e.out() == out
    assert tail_is_canary(e.out_t, len(out))
    del e, t
    _free(torch)
