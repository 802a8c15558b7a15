"""lv_write_batch_encode_host against the Python model
(tests/write_batch_encode_cases.py, built on the restated WriteBatch::put /
delete / set_sequence), the reference's own cases (write_batch.rs:240-297),
the round trip through lv_write_batch_iterate, and what needs no GPU of
lv_write_batch_encode_device: its argument checks, the header against the
Python mirror, the mirrored kernel constants, the exported symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

import lvgpu
import lvgpu.write_batch as WB
import write_batch_cases as C
import write_batch_encode_cases as E
from conftest import ROOT
from write_batch_cases import M64

HEADER = os.path.join(ROOT, "include", "lvgpu", "write_batch.h")
SOURCE = os.path.join(ROOT, "leveldb-rs_amd", "csrc", "write_batch_encode.hip")


def host(src, ops, rec_op, first, **kw):
    return WB.encode_host(src, ops, rec_op, first, **kw)


def agree(src, ops, rec_op, first, *, op_cap=None, out_cap=None, tag=""):
    """The host twin against the model, and every record back through
    lv_write_batch_iterate."""
    records = len(rec_op) - 1
    cap = len(ops) if op_cap is None else op_cap
    want = E.model(src, ops, rec_op, records, first, cap, out_cap)
    out, off, ln, ops_out, tot = host(src, ops, rec_op, first, op_cap=cap, out_cap=out_cap)
    assert tot == want[4], (tag, tot, want[4])
    if tot["status"]:
        return tot
    assert out == want[0], tag
    assert np.array_equal(off, want[1]) and np.array_equal(ln, want[2]), tag
    assert (ops_out == want[3]).all(), tag
    base = int(rec_op[0]) if records else 0
    for r in range(records):
        o, n = int(off[r]), int(ln[r])
        st, rops, seq, cnt = WB.iterate(out[o:o + n])
        a, b = int(rec_op[r]) - base, int(rec_op[r + 1]) - base
        assert st == WB.OK and seq == (first + a) & M64 and cnt == b - a, (tag, r)
        back = [(t, ko + o, kl, vo + o, vl) for t, ko, kl, vo, vl in rops]
        mine = [(int(x["tag"]), int(x["key_off"]), int(x["key_len"]), int(x["val_off"]), int(x["val_len"]))
                for x in ops_out[a:b]]
        assert back == mine, (tag, r)
    return tot


def test_reference_multiple():
    src, ops, rec_op = E.ref_multiple_table()
    out, off, ln, ops_out, tot = host(src, ops, rec_op, 100)
    assert out == C.ref_multiple().bytes()
    assert tot["last_sequence"] == 102 and tot["ops"] == 3 and ln.tolist() == [len(out)]
    assert C.print_contents(out) == "Put(baz, boo)@102Delete(box)@101Put(foo, bar)@100"
    agree(src, ops, rec_op, 100)


def test_reference_append_stages():
    stages = C.ref_append_stages()
    tables = E.ref_append_tables()
    assert len(stages) == len(tables) == 4
    for k, ((rep, contents), (src, ops, rec_op)) in enumerate(zip(stages, tables)):
        out, _, _, _, tot = host(src, ops, rec_op, 200)
        assert out == rep and C.print_contents(out) == contents, k
        assert tot["ops"] == len(ops) and tot["records"] == 1
        agree(src, ops, rec_op, 200, tag=f"stage {k}")
    assert len(stages[0][0]) == 12  # an empty record is its header


def test_append_over_any_split():
    """The record's bytes are what WriteBatchInternal::append leaves over any
    split of its ops into batches."""
    specs = [(b"k%d" % i, None if i % 3 == 0 else b"v" * i) for i in range(7)]
    src, ops, rec_op = E.table([specs])
    out = host(src, ops, rec_op, 50)[0]
    for cut1 in range(8):
        for cut2 in range(cut1, 8):
            whole = C.WriteBatch().set_sequence(50)
            for part in (specs[:cut1], specs[cut1:cut2], specs[cut2:]):
                b = C.WriteBatch().set_sequence(999)
                for k, v in part:
                    b.delete(k) if v is None else b.put(k, v)
                whole.append(b)
            assert whole.bytes() == out, (cut1, cut2)


def test_mixed_tables_against_the_model():
    for seed in range(12):
        counts = [0, 3, 1, 0, 0, 12, 1, 40, 0][seed % 4:] + [seed]
        src, ops, rec_op = E.pool_table(counts, E.short_len, seed=seed, lead=seed % 3)
        tot = agree(src, ops, rec_op, 1000 * seed + 1, tag=f"seed {seed}")
        assert tot["status"] == 0 and tot["records"] == len(counts) and tot["ops"] == sum(counts)
    # no records at all
    src, ops, rec_op = E.pool_table([], E.short_len)
    tot = agree(src, ops, rec_op, 7)
    assert tot == dict(records=0, ops=0, key_bytes=0, value_bytes=0, out_bytes=0, last_sequence=6, status=0,
                       bad_record=M64, bad_op=M64)
    # repeated and overlapping extents
    src = bytes(range(200))
    dt = WB.OP_DTYPE
    ops = np.array([(1, 10, 12, 20, 100), (1, 10, 10, 20, 20), (0, 0, 0, 200, 0), (1, 199, 0, 1, 200)], dtype=dt)
    agree(src, ops, np.array([0, 2, 4], dtype=np.uint64), 3, tag="overlapping")


@pytest.mark.parametrize("n", E.VARINT_EDGES)
def test_varint_edges(n):
    """Key and value lengths on both sides of every varint size."""
    src = bytes((7 * i + 3) & 0xFF for i in range(n + 5))
    dt = WB.OP_DTYPE
    ops = np.array([(1, 1, 2, n, 3), (1, 0, 3, 2, n), (0, 5, 0, n, 0), (1, 2, 1, n, n)], dtype=dt)
    tot = agree(src, ops, np.array([0, 1, 4], dtype=np.uint64), 9, tag=f"n={n}")
    assert tot["key_bytes"] == 3 * n + 2 and tot["value_bytes"] == 2 * n + 3
    # two headers, four type bytes, five varints of n, those of 3 and 2, the strings
    assert tot["out_bytes"] == 24 + 4 + 5 * len(C.varint(n)) + 2 + 5 * n + 5


@pytest.mark.parametrize("n", [(1 << 28) - 1, 1 << 28])
def test_five_byte_varint_on_the_host(n):
    """The first five-byte length: one Put of a 3-byte key and an n-byte value."""
    src = np.zeros(n + 3, dtype=np.uint8)
    src[:3] = (1, 2, 3)
    src[3::4099] = 0xC3
    src = src.tobytes()
    ops = np.array([(1, 0, 3, 3, n)], dtype=WB.OP_DTYPE)
    out, off, ln, ops_out, tot = host(src, ops, np.array([0, 1], dtype=np.uint64), 5)
    v = C.varint(n)
    assert len(v) == (4 if n < 1 << 28 else 5)
    head = (5).to_bytes(8, "little") + (1).to_bytes(4, "little") + bytes([1, 3, 1, 2, 3]) + v
    assert tot["status"] == 0 and tot["out_bytes"] == len(head) + n == len(out)
    assert out[:len(head)] == head and out[len(head):] == src[3:]
    assert int(ops_out[0]["val_off"]) == len(head) and int(ops_out[0]["val_len"]) == n


STATUS = list(E.status_cases())


@pytest.mark.parametrize("name", [c[0] for c in STATUS])
def test_status_cases(name):
    _, src, ops, rec_op, op_cap, out_cap, status = next(c for c in STATUS if c[0] == name)
    tot = agree(src, ops, rec_op, 77, op_cap=op_cap, out_cap=out_cap, tag=name)
    assert tot["status"] == status
    if status in (E.BAD_BOUNDS, E.BAD_OP):
        assert tot["ops"] == tot["out_bytes"] == 0 and tot["last_sequence"] == 76
        assert (tot["bad_op"] == M64) == (status == E.BAD_BOUNDS) and tot["bad_record"] != M64
    if name == "second_op_bad":
        assert (tot["bad_record"], tot["bad_op"]) == (3, 1)  # behind the empty records
    if name == "out_one_short":
        assert tot["out_bytes"] == out_cap + 1 and tot["ops"] == 2  # the true totals: size and call again


def test_status_leaves_the_arrays_alone():
    """In every status case the host twin writes nothing but the totals."""
    L = WB._bind()
    for name, src, ops, rec_op, op_cap, out_cap, status in STATUS:
        if not status:
            continue
        records = len(rec_op) - 1
        out = np.full(64, 0xA5, dtype=np.uint8)
        off, ln = np.full(records, 0xA5A5, dtype=np.uint64), np.full(records, 0xA5A5, dtype=np.uint64)
        oo = np.full(max(op_cap, 1) * 32, 0xA5, dtype=np.uint8)
        tot = WB.EncodeTotals()
        buf = ctypes.create_string_buffer(bytes(src), len(src))
        rc = L.lv_write_batch_encode_host(buf, len(src), ops.ctypes.data, op_cap, rec_op.ctypes.data, records, 1,
                                          out.ctypes.data, 64 if out_cap is None else out_cap, off.ctypes.data,
                                          ln.ctypes.data, oo.ctypes.data, ctypes.byref(tot))
        assert rc == 0 and tot.status == status, name
        assert (out == 0xA5).all() and (off == 0xA5A5).all() and (ln == 0xA5A5).all() and (oo == 0xA5).all(), name


def test_sizing_mode():
    """out == NULL with out_cap == 0: the arrays and the totals as if the
    capacity sufficed, no OUT_OVER, and src is never read (it may be NULL)."""
    src, ops, rec_op = E.pool_table([3, 0, 5, 1], E.short_len, seed=5)
    full = host(src, ops, rec_op, 40)
    _, off, ln, ops_out, tot = host(None, ops, rec_op, 40, sizing=True, src_bytes=len(src))
    assert tot == full[4] and tot["status"] == 0 and tot["out_bytes"] > 0
    assert np.array_equal(off, full[1]) and np.array_equal(ln, full[2]) and (ops_out == full[3]).all()
    assert int(off[-1] + ln[-1]) == tot["out_bytes"]
    # the extents are still checked
    ops2 = ops.copy()
    ops2[2]["key_off"] = len(src)
    ops2[2]["key_len"] = 1
    t2 = host(None, ops2, rec_op, 40, sizing=True, src_bytes=len(src))[4]
    assert t2["status"] == E.BAD_OP and t2["bad_op"] == 2


def test_sequence_wrap():
    src, ops, rec_op = E.table([[(b"a", b"1"), (b"b", None)], [], [(b"c", b"3"), (b"d", b"4"), (b"e", None)]])
    first = (1 << 64) - 2
    tot = agree(src, ops, rec_op, first, tag="wrap")
    out, off, _, ops_out, _ = host(src, ops, rec_op, first)
    assert tot["last_sequence"] == 2 and tot["ops"] == 5
    assert [int(t) >> 8 for t in ops_out["tag"]] == [(first + i) & ((1 << 56) - 1) for i in range(5)]
    assert [int.from_bytes(out[int(o):int(o) + 8], "little") for o in off] == [first, 0, 0]


def test_host_argument_checks():
    L = WB._bind()
    tot = WB.EncodeTotals()
    one = (ctypes.c_uint64 * 2)(0, 0)
    fake = ctypes.c_void_p(0x1000)
    ok = L.lv_write_batch_encode_host(None, 0, None, 0, one, 0, 1, None, 0, None, None, None, ctypes.byref(tot))
    assert ok == 0 and tot.status == 0 and tot.last_sequence == 0
    bad = [
        (None, 0, None, 0, one, 0, 1, None, 0, None, None, None, None),                      # totals
        (None, 0, None, 0, None, 0, 1, None, 0, None, None, None, ctypes.byref(tot)),        # rec_op
        (None, 1, None, 0, one, 0, 1, fake, 1, None, None, None, ctypes.byref(tot)),         # src (not sizing)
        (None, 0, None, 1, one, 0, 1, None, 0, None, None, None, ctypes.byref(tot)),         # ops
        (None, 0, None, 0, one, 0, 1, None, 1, None, None, None, ctypes.byref(tot)),         # out
        (None, 0, None, 0, one, 1, 1, None, 0, None, None, None, ctypes.byref(tot)),         # rec_off / rec_len
        (None, 0, fake, (1 << 30) + 1, one, 0, 1, None, 0, None, None, None, ctypes.byref(tot)),
        (None, 0, None, 0, one, (1 << 32) - 1, 1, None, 0, fake, fake, None, ctypes.byref(tot)),
    ]
    for args in bad:
        assert L.lv_write_batch_encode_host(*args) == -1, args


def test_device_argument_checks_before_any_device_call():
    """Every check of lv_write_batch_encode_device runs before it touches the
    GPU: LV_ERR_INVALID and a message, with pointers that are never
    dereferenced."""
    L = WB._bind()
    err = lambda: lvgpu.lib().lv_last_error()
    vp = ctypes.c_void_p
    A = 0x10000  # 16-B aligned, far from everything below
    need = WB.encode_workspace_bytes(8, 8)
    # a prefix per op and three sums per tile of 1,024 ops (each region a multiple of 16 bytes)
    assert need > 0 and WB.encode_workspace_bytes(8, 8 + 2048) - need == 2048 * 8 + 3 * 16
    assert WB.encode_workspace_bytes(1 << 32, 8) == 0 and WB.encode_workspace_bytes(8, (1 << 30) + 1) == 0

    def call(*, src=A, src_bytes=64, ops=2 * A, op_cap=8, rec_op=3 * A, records=4 * A, up=None, rec_cap=8, out=5 * A,
             out_cap=64, rec_off=6 * A, rec_len=7 * A, ops_out=8 * A, totals=9 * A, flags=0, ws=10 * A, ws_bytes=need,
             desc=True):
        o = WB.EncodeOut(out, out_cap, rec_off, rec_len, ops_out, totals)
        return L.lv_write_batch_encode_device(vp(src) if src else None, src_bytes, vp(ops) if ops else None, op_cap,
                                              vp(rec_op) if rec_op else None, vp(records) if records else None, up,
                                              rec_cap, 1, ctypes.byref(o) if desc else None, flags,
                                              vp(ws) if ws else None, ws_bytes, None)
    cases = [
        (dict(flags=1), b"flag"), (dict(desc=False), b"descriptor"), (dict(totals=None), b"d_totals"),
        (dict(totals=9 * A + 4), b"8-byte"), (dict(records=None), b"d_records"), (dict(src=None), b"d_src"),
        (dict(rec_cap=(1 << 32) - 1), b"2^32 - 2"), (dict(op_cap=(1 << 30) + 1), b"2^30"),
        (dict(rec_op=None), b"d_rec_op"), (dict(rec_op=3 * A + 4), b"8-byte"), (dict(rec_off=None), b"record array"),
        (dict(rec_len=None), b"record array"), (dict(rec_off=6 * A + 4), b"8-byte"), (dict(rec_len=7 * A + 2), b"8-byte"),
        (dict(ops=None), b"d_ops"), (dict(ops=2 * A + 8), b"16-byte"), (dict(ops_out=8 * A + 8), b"16-byte"),
        (dict(out=None), b"d_out"), (dict(ws=None), b"workspace"), (dict(ws=10 * A + 8), b"16-byte"),
        (dict(ws_bytes=need - 1), b"workspace too small"),
        (dict(out=A + 63), b"d_out overlaps d_src"), (dict(out=A - 63), b"d_out overlaps d_src"),
        (dict(out=2 * A + 255), b"d_out overlaps d_ops"), (dict(out=8 * A - 1, out_cap=2), b"d_out overlaps d_ops_out"),
        (dict(ops_out=2 * A + 240), b"d_ops_out overlaps d_ops"),
    ]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in err(), (kw, err())
    # what may be NULL or touch: none of these fails its checks, so each reaches
    # the device context, which without a GPU is the runtime's error
    import torch
    if not torch.cuda.is_available():
        for kw in (dict(src=None, src_bytes=0), dict(ops=None, op_cap=0, ops_out=None, ws_bytes=WB.encode_workspace_bytes(8, 0)),
                   dict(out=None, out_cap=0), dict(ops_out=None), dict(out=A + 64), dict(out=A - 64),
                   dict(rec_off=None, rec_len=None, rec_cap=0)):
            assert call(**kw) not in (0, -1), (kw, err())


def test_constants_match_header():
    with open(HEADER) as f:
        text = f.read()
    d = {k: int(v) for k, v in re.findall(r"#define LV_WB_ENCODE_(\w+)\s+(\d+)u", text)}
    assert {v: k for k, v in d.items()} == WB.ENCODE_STATUS
    assert (E.UPSTREAM, E.REC_OVER, E.BAD_BOUNDS, E.BAD_OP, E.OUT_OVER) == tuple(sorted(d.values())) == (1, 2, 4, 8, 16)
    m = re.search(r"typedef struct lv_wb_encode_totals \{[^\n]*\n\s*uint64_t ([^;]+);", text)
    assert tuple(x.strip() for x in m.group(1).split(",")) == WB.ENCODE_TOTALS == E.TOTALS
    assert ctypes.sizeof(WB.EncodeTotals) == 9 * 8
    m = re.search(r"typedef struct lv_wb_encode_out \{(.*?)\} lv_wb_encode_out;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"\*?\b(d_\w+|out_cap)\b", body)
    assert fields == [n for n, _ in WB.EncodeOut._fields_] and ctypes.sizeof(WB.EncodeOut) == 6 * 8
    # the first struct the older test's pattern finds is still the decode's
    assert re.search(r"typedef struct lv_wb_totals \{", text).start() < text.index("lv_wb_encode_totals")
    assert "2^30" in text and WB.ENCODE_MAX_OP_CAP == 1 << 30 and WB.ENCODE_MAX_REC_CAP == (1 << 32) - 2


def test_we_constants_match_source():
    """lvgpu.write_batch.WE_* (the GPU tests sweep around them) are the
    kernels' named constants."""
    with open(SOURCE) as f:
        text = f.read()
    assert WB.WE_TILE == int(re.search(r"kWeTile = (\d+);", text).group(1))
    assert WB.WE_WAVE_COPY == int(re.search(r"kWeWaveCopy = (\d+);", text).group(1))
    assert WB.WE_COPY_LANES == int(re.search(r"kWeCopyLanes = (\d+);", text).group(1))
    threads = int(re.search(r"kWeThreads = (\d+);", text).group(1))
    assert WB.WE_TILE % threads == 0 and 64 % WB.WE_COPY_LANES == 0 and WB.WE_WAVE_COPY >= 16
    assert "group_copy<kWeCopyLanes, kWeWaveCopy>" in text
    # the grids are sized by the work: no capped grid, no name added to the debug grids
    assert "gridDim" not in text and "lv_debug_launch_grid" not in text


def test_symbols_declared_and_exported():
    names = lvgpu.declared_symbols()
    L = ctypes.CDLL(lvgpu.LIB_PATH)
    for n in ("lv_write_batch_encode_workspace_bytes", "lv_write_batch_encode_device", "lv_write_batch_encode_host"):
        assert n in names and hasattr(L, n), n
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for n in ("lv_write_batch_encode_workspace_bytes", "lv_write_batch_encode_device", "lv_write_batch_encode_host"):
        assert re.search(r"\bfn " + n + r"\s*\(", doc), n


def test_stress_trials_are_not_hollow():
    """At least one trial in five holds an empty record, a long copy and a
    record above one tile; d_rec_op[0] != 0 and a wrapping sequence occur."""
    flags, leads, firsts = [], [], []
    for seed in range(E.STRESS_TRIALS):
        _, ops, rec_op, first, lead, f = E.stress_trial(seed, WB.WE_TILE, WB.WE_WAVE_COPY)
        flags.append(f)
        leads.append(lead)
        firsts.append(first)
        if seed % 5 == 0:
            assert all(f), (seed, f)
    assert sum(all(f) for f in flags) * 5 >= E.STRESS_TRIALS
    assert any(leads) and any(f > M64 - 100 for f in firsts)
