"""Everything about the WriteBatch walk that needs no GPU: the host scalar twin
lv_write_batch_iterate against the model (tests/write_batch_cases.py) and the
reference's own tests (write_batch.rs:240-297), the constants, the workspace
size and the argument checks of lv_write_batch_decode_device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lvgpu
import lvgpu.write_batch as WB
import write_batch_cases as C

INVALID = -1  # LV_ERR_INVALID
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lvgpu", "write_batch.h")
SOURCE = os.path.join(ROOT, "leveldb-rs_amd", "csrc", "write_batch.hip")


def host_equals_model(rep, tag=""):
    """lv_write_batch_iterate == the model with an ample op_cap, with 0 and
    with found - 1; returns the model's (status, ops)."""
    rep = bytes(rep)
    st, ops, seq, cnt = C.iterate_ext(rep)
    got = WB.iterate_found(rep)
    assert got == (st, ops, seq, cnt, len(ops)), (tag, got[0], st, got[4], len(ops))
    none = WB.iterate_found(rep, 0)
    assert none == (st, [], seq, cnt, len(ops)), (tag, "op_cap 0")
    if ops:
        short = WB.iterate_found(rep, len(ops) - 1)
        assert short == (st, ops[:-1], seq, cnt, len(ops)), (tag, "op_cap found - 1")
    return st, ops


def test_symbols_declared_and_exported():
    names = lvgpu.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", lvgpu.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in ("lv_write_batch_iterate", "lv_write_batch_decode_workspace_bytes", "lv_write_batch_decode_device"):
        assert n in names and n in syms, n


def test_constants_match_header():
    with open(HEADER) as f:
        text = f.read()
    d = {k: int(v) for k, v in re.findall(r"#define LV_WB_(\w+)\s+(\d+)u", text)}
    assert d["HEADER_SIZE"] == WB.HEADER_SIZE == C.HEADER == 12
    assert (d["TYPE_DELETION"], d["TYPE_VALUE"]) == (WB.TYPE_DELETION, WB.TYPE_VALUE) == (C.DELETION, C.VALUE)
    names = ("OK", "TOO_SMALL", "BAD_VARINT", "BAD_LENGTH", "WRONG_COUNT", "BAD_TAG", "OUT_OF_RANGE")
    assert [d[n] for n in names] == [getattr(WB, n) for n in names] == [getattr(C, n) for n in names] == list(range(7))
    assert {d["DECODE_" + n]: n for n in ("UPSTREAM", "REC_OVER", "OP_OVER")} == WB.DECODE_STATUS
    assert (C.UPSTREAM, C.REC_OVER, C.OP_OVER) == (1, 2, 4)
    # the strings of the reference's error returns, as the header quotes them
    quoted = dict(re.findall(r'#define LV_WB_\w+\s+(\d)u\s+/\* "([^"]+)" \*/', text))
    assert {int(k): v for k, v in quoted.items()} == WB.STATUS_TEXT
    # the op and the totals: field order and size
    assert WB.OP_DTYPE.names == ("tag", "key_off", "val_off", "key_len", "val_len") and WB.OP_DTYPE.itemsize == 32
    m = re.search(r"typedef struct lv_wb_totals \{[^\n]*\n\s*uint64_t ([^;]+);", text)
    assert tuple(x.strip() for x in m.group(1).split(",")) == WB.TOTALS
    assert ctypes.sizeof(WB.DecodeOut) == 5 * 8


def test_wb_constants_match_source():
    """lvgpu.write_batch.WB_* (the GPU tests sweep around them) are the
    kernels' named constants."""
    with open(SOURCE) as f:
        text = f.read()
    threads = int(re.search(r"kWbThreads = (\d+);", text).group(1))
    per = int(re.search(r"kWbPer = (\d+);", text).group(1))
    assert "kWbTile = kWbThreads * kWbPer;" in text and WB.WB_TILE == threads * per
    assert WB.WB_SMALL == int(re.search(r"kWbSmall = (\d+);", text).group(1))
    assert WB.WB_WINDOW == int(re.search(r"kWbWindow = (\d+);", text).group(1))
    assert "kWbRound = 64 * 16;" in text and WB.WB_ROUND == 1024
    assert WB.WB_SMALL >= 12 and WB.WB_WINDOW % WB.WB_ROUND == 0 and WB.WB_WINDOW > WB.WB_ROUND


def test_workspace_bytes():
    L = WB._bind()
    prev = 0
    for cap in [0, 1, 2, 100, 1023, 1024, 1025, 4681, 65536, 1 << 20, (1 << 20) + 1]:
        w = L.lv_write_batch_decode_workspace_bytes(cap)
        assert w >= prev and w % 16 == 0 and w >= 12 * cap, cap
        prev = w
    assert WB.decode_workspace_bytes(1000) == L.lv_write_batch_decode_workspace_bytes(1000)


# ---- the reference's own tests (write_batch.rs:240-297) ----
def test_reference_empty():
    b = C.WriteBatch()
    assert C.print_contents(b.rep) == "" and b.count == 0
    assert host_equals_model(b.rep) == (C.OK, [])


def test_reference_multiple():
    b = C.ref_multiple()
    assert b.sequence == 100 and b.count == 3
    assert C.print_contents(b.rep) == "Put(baz, boo)@102Delete(box)@101Put(foo, bar)@100"
    st, ops = host_equals_model(b.rep)
    assert st == C.OK and [t >> 8 for t, *_ in ops] == [100, 101, 102]
    assert [t & 0xFF for t, *_ in ops] == [C.VALUE, C.DELETION, C.VALUE]
    rep = b.bytes()
    assert [rep[ko:ko + kl] for _, ko, kl, _, _ in ops] == [b"foo", b"box", b"baz"]
    assert [rep[vo:vo + vl] for _, _, _, vo, vl in ops] == [b"bar", b"", b"boo"]
    # DELETION: val_off = key_off + key_len, val_len = 0
    assert ops[1][3] == ops[1][1] + ops[1][2] and ops[1][4] == 0
    assert WB.iterate(rep) == (C.OK, ops, 100, 3)


def test_reference_corruption():
    b = C.ref_corruption()
    assert C.print_contents(b.rep) == "Put(foo, bar)@200ParseError()"
    st, ops = host_equals_model(b.rep)
    assert st == C.BAD_LENGTH and len(ops) == 1 and ops[0][0] == (200 << 8) | C.VALUE


def test_reference_append():
    for i, (rep, want) in enumerate(C.ref_append_stages()):
        assert C.print_contents(rep) == want, i
        st, ops = host_equals_model(rep, f"append{i}")
        assert st == C.OK and len(ops) == [0, 1, 2, 4][i]  # the last append brings b2's two entries
        assert [t >> 8 for t, *_ in ops] == list(range(200, 200 + len(ops)))


@pytest.mark.parametrize("name", [c[0] for c in C.status_cases()])
def test_every_status(name):
    _, rep, status, nops = next(c for c in C.status_cases() if c[0] == name)
    st, ops = host_equals_model(rep, name)
    assert (st, len(ops)) == (status, nops)


def test_every_status_is_covered():
    seen = {c[2] for c in C.status_cases()}
    assert seen == {C.OK, C.TOO_SMALL, C.BAD_VARINT, C.BAD_LENGTH, C.WRONG_COUNT, C.BAD_TAG}


def test_varint_top_bits_are_discarded():
    rep = next(c[1] for c in C.status_cases() if c[0] == "varint5_top_bits")
    st, ops = host_equals_model(rep)
    assert st == C.OK and ops == [((1 << 8) | C.DELETION, 18, 2, 20, 0)]


def test_sequence_wraps():
    b = C.WriteBatch().set_sequence((1 << 56) - 1).put(b"a", b"1").delete(b"b").put(b"c", b"3")
    st, ops = host_equals_model(b.rep)
    assert st == C.OK
    # (2^56 - 1) << 8 fills the top; the next sequence numbers wrap out of the 64-bit tag
    assert [o[0] for o in ops] == [(((1 << 56) - 1) << 8) | 1, 0 | 0, (1 << 8) | 1]
    b = C.WriteBatch().set_sequence((1 << 64) - 1).put(b"a", b"1").put(b"b", b"2")
    st, ops = host_equals_model(b.rep)
    assert st == C.OK and [o[0] for o in ops] == [(((1 << 64) - 1) << 8 | 1) & C.M64, 1]
    assert WB.iterate(b.rep)[2] == (1 << 64) - 1


def test_every_truncation_of_a_mixed_batch():
    rep = C.mixed_batch(20).bytes()
    full = C.iterate_ext(rep)
    assert full[0] == C.OK and len(full[1]) == 20
    seen = set()
    for n in range(len(rep) + 1):
        st, ops = host_equals_model(rep[:n], f"cut{n}")
        seen.add(st)
        assert ops == full[1][: len(ops)]
    assert seen == {C.OK, C.TOO_SMALL, C.BAD_VARINT, C.BAD_LENGTH, C.WRONG_COUNT}


def test_random_byte_strings():
    rng = np.random.default_rng(77)
    seen = set()
    for i in range(2000):
        n = int(rng.integers(0, 80))
        raw = bytearray(rng.integers(0, 256, size=n, dtype=np.uint8).tobytes())
        if i % 2 and n > 12:  # tags and lengths that parse further
            for j in range(12, n):
                raw[j] &= 0x83 if rng.random() < 0.1 else 0x07 if rng.random() < 0.7 else 0xFF
        st, _ = host_equals_model(raw, f"random{i}")
        seen.add(st)
    assert seen >= {C.TOO_SMALL, C.BAD_VARINT, C.BAD_LENGTH, C.WRONG_COUNT, C.BAD_TAG}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernels_do_not_spill():
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-munsafe-fp-atomics", "--cuda-device-only", "-c", "-o", os.devnull, SOURCE,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    spills, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name:
            spills[name] = int(m.group(1))
    for k in ("wb_count", "wb_tiles", "wb_emit"):
        hits = {n: v for n, v in spills.items() if k in n}
        assert hits and all(v == 0 for v in hits.values()), (k, hits)


def test_decode_device_argument_checks():
    """Every argument error of lv_write_batch_decode_device is found on the
    host, before any device call: LV_ERR_INVALID and a message, with pointers
    that are never dereferenced and no GPU in the machine."""
    L = WB._bind()
    vp = ctypes.c_void_p
    cap, nbytes = 100, 4096
    wsb = L.lv_write_batch_decode_workspace_bytes(cap)
    err = lambda: lvgpu.lib().lv_last_error()

    def out(**kw):
        o = WB.DecodeOut()
        o.d_ops, o.op_cap = 0x900000, nbytes // 2
        o.d_rec_op, o.d_rec_status, o.d_totals = 0xA00000, 0xA10000, 0xC00000
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(pay=vp(0x100000), n=nbytes, off=vp(0x200000), ln=vp(0x300000), recs=vp(0x500000), up=vp(0x600000),
             c=cap, o="default", flags=0, w=vp(0x4000000), wb=wsb):
        o = out() if o == "default" else o
        return L.lv_write_batch_decode_device(pay, n, off, ln, recs, up, c, ctypes.byref(o) if o is not None else None,
                                              flags, w, wb, None)

    # NULL pointers
    assert call(pay=None) == INVALID and b"null" in err()
    assert call(off=None) == INVALID and b"null" in err()
    assert call(ln=None) == INVALID and b"null" in err()
    assert call(recs=None) == INVALID and b"null" in err()
    assert call(o=None) == INVALID and b"null" in err()
    assert call(w=None) == INVALID and b"workspace" in err()
    for field in ("d_ops", "d_rec_op", "d_rec_status", "d_totals"):
        assert call(o=out(**{field: None})) == INVALID and b"null" in err(), field
    # alignment: d_ops 16, d_totals 8, workspace 16
    assert call(o=out(d_ops=0x900008)) == INVALID and b"d_ops" in err() and b"16-byte" in err()
    assert call(o=out(d_totals=0xC00004)) == INVALID and b"d_totals" in err()
    assert call(w=vp(0x4000008)) == INVALID and b"aligned" in err()
    # workspace one byte short
    assert call(wb=wsb - 1) == INVALID and b"workspace too small" in err()
    # no flag is defined
    assert call(flags=1) == INVALID and b"flag" in err()
    assert call(flags=0x80000000) == INVALID and b"flag" in err()
    # limits
    assert call(c=0xFFFFFFFF, wb=1 << 62) == INVALID and b"rec_cap" in err()
    assert call(o=out(op_cap=(1 << 58) + 1)) == INVALID and b"op_cap" in err()
    # d_ops[0, op_cap) inside / straddling the payload, at either end
    assert call(o=out(d_ops=0x100000 + nbytes - 16)) == INVALID and b"overlap" in err()
    assert call(o=out(d_ops=0x100000 - 32 * (nbytes // 2) + 16)) == INVALID and b"overlap" in err()
    assert call(o=out(d_ops=0x100000 + 16, op_cap=1)) == INVALID and b"overlap" in err()
    # What passes the checks goes on to the device: with no GPU that is an
    # error of another kind, never LV_ERR_INVALID.  (A NULL upstream status; a
    # table that ends where the payload starts; no payload, no records.)
    import torch
    if not torch.cuda.is_available():
        assert call(up=None) not in (0, INVALID)
        assert call(o=out(d_ops=0x100000 - 32 * (nbytes // 2))) not in (0, INVALID)
        assert call(pay=None, n=0, off=None, ln=None, c=0, o=out(d_ops=None, op_cap=0, d_rec_status=None),
                    wb=L.lv_write_batch_decode_workspace_bytes(0)) not in (0, INVALID)
        assert lvgpu.lib().lv_last_error()
