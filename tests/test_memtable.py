"""Everything about the memtable order that needs no GPU: the host twins
lv_internal_key_compare, lv_memtable_build_host and lv_memtable_get_host
against the model (tests/memtable_cases.py), the reference's own print tests
(write_batch.rs:240-297) under the reference's entry order and under the
product's, the constants, the workspace size and the argument checks of the
device entry points."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lvgpu
import lvgpu.memtable as MT
import memtable_cases as C
import write_batch_cases as W

INVALID = -1  # LV_ERR_INVALID
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lvgpu", "memtable.h")
SOURCE = os.path.join(ROOT, "leveldb-rs_amd", "csrc", "memtable.hip")
KNOBS = os.path.join(ROOT, "leveldb-rs_amd", "csrc", "lvk", "knobs.h")


def host_equals_model(payload, ops, tag=""):
    order, tot = MT.build_host(payload, ops)
    want_order, want_tot = C.model_totals(payload, ops)
    assert tot == want_tot, (tag, tot, want_tot)
    assert order.tolist() == want_order, (tag, order[:8], want_order[:8])
    return order, tot


def test_symbols_declared_and_exported():
    names = lvgpu.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", lvgpu.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in ("lv_internal_key_compare", "lv_memtable_build_workspace_bytes", "lv_memtable_build_device",
              "lv_memtable_get_device", "lv_memtable_build_host", "lv_memtable_get_host"):
        assert n in names and n in syms, n


def test_constants_match_header_and_knobs():
    with open(HEADER) as f:
        text = f.read()
    d = {k: int(v) for k, v in re.findall(r"#define LV_MT_(\w+)\s+(\d+)u", text)}
    assert {d["BUILD_" + n]: n for n in ("UPSTREAM", "OP_OVER", "BAD_OP")} == MT.BUILD_STATUS
    assert (C.UPSTREAM, C.OP_OVER, C.BAD_OP) == (1, 2, 4)
    names = ("ABSENT", "FOUND", "DELETED", "BAD_SEQ", "NO_TABLE", "BAD_QUERY")
    assert [d["GET_" + n] for n in names] == [getattr(MT, "GET_" + n) for n in names] == list(range(6))
    assert [getattr(C, n) for n in names] == list(range(6))
    assert "#define LV_MT_MAX_SEQUENCE ((1ull << 56) - 1)" in text and MT.MAX_SEQUENCE == C.MAX_SEQUENCE == 2**56 - 1
    m = re.search(r"typedef struct lv_mt_totals \{[^\n]*\n\s*uint64_t ([^;]+);", text)
    assert tuple(x.strip() for x in m.group(1).split(",")) == MT.TOTALS
    assert ctypes.sizeof(MT.Totals) == 24 and ctypes.sizeof(MT.GetResult) == 24 == MT.RESULT_DTYPE.itemsize
    assert MT.RESULT_DTYPE.names == ("val_off", "val_len", "op", "status", "reserved")
    # the tunables the GPU tests sweep around
    with open(KNOBS) as f:
        knobs = f.read()
    assert MT.MT_TILE == int(re.search(r"#define LVK_MT_TILE (\d+)", knobs).group(1))
    assert MT.MT_PREFIX == int(re.search(r"#define LVK_MT_PREFIX (\d+)", knobs).group(1))
    with open(SOURCE) as f:
        src = f.read()
    assert "kMtTile = LVK_MT_TILE;" in src and "kMtPrefix = LVK_MT_PREFIX;" in src
    # the header says where the order differs from the reference's MemTable
    assert "does NOT produce this order" in text and "write_batch.rs:293-296" in text


def test_workspace_bytes():
    L = MT._bind()
    prev = 0
    for cap in [0, 1, 2, 100, 1023, 1024, 1025, 4681, 65536, 1 << 20, (1 << 20) + 1]:
        w = L.lv_memtable_build_workspace_bytes(cap)
        assert w >= prev and w % 16 == 0 and w >= 32 * cap, cap
        prev = w
    assert MT.build_workspace_bytes(1000) == L.lv_memtable_build_workspace_bytes(1000)


# ---- the comparator ----
def model_compare(a, ta, b, tb):
    x, y = (a, -ta), (b, -tb)
    return -1 if x < y else 1 if x > y else 0


@pytest.mark.parametrize("group", list(C.corner_groups()))
def test_compare_corner_keys(group):
    keys = C.corner_groups()[group]
    tags = [C.tag(5), C.tag(5, 0), C.tag(6), C.tag(1 << 56), C.M64]
    for a in keys:
        for b in keys:
            for ta in tags:
                for tb in tags[:3] if len(a) > 100 else tags:
                    assert MT.compare(a, ta, b, tb) == model_compare(a, ta, b, tb), (a[:20], ta, b[:20], tb)


def test_compare_rules():
    assert MT.compare(b"", 0, b"", 0) == 0
    assert MT.compare(b"a", 0, b"a\x00", C.M64) == -1          # a proper prefix first, whatever the tags
    assert MT.compare(b"\x7f", 0, b"\x80", 0) == -1            # unsigned bytes
    assert MT.compare(b"ab", 0, b"ba", 0) == -1                # the first byte decides
    assert MT.compare(b"k", C.tag(9), b"k", C.tag(8)) == -1    # the newer sequence first
    assert MT.compare(b"k", C.tag(9, 1), b"k", C.tag(9, 0)) == -1   # VALUE before DELETION
    assert MT.compare(b"k", 1 << 63, b"k", (1 << 63) - 1) == -1     # the tag is unsigned
    assert MT.compare(b"k", C.tag(9), b"k", C.tag(9)) == 0


# ---- the build ----
def test_build_host_corner_and_tag_tables():
    payload, ops = C.make_table(C.corner_items() + C.tag_items())
    order, tot = host_equals_model(payload, ops, "corner")
    items = C.tag_items()
    payload, ops = C.make_table(items)
    order, tot = host_equals_model(payload, ops, "tags")
    printed = [(items[i][0], items[i][1], i) for i in order]
    dups = [i for k, t, i in printed if k == b"dup" and t == C.tag(42)]
    assert dups == sorted(dups, reverse=True) and len(dups) == 3     # later duplicates in front
    vers = [t >> 8 for k, t, i in printed if k == b"versions"]
    assert vers == [900, 900, 77, 77, 5, 1]
    tops = [t for k, t, i in printed if k == b"top"]
    assert tops == sorted(tops, reverse=True) and tops[0] == C.tag(C.M64 >> 8)  # full unsigned 64-bit tags
    for group, keys in C.corner_groups().items():                   # each group alone, in pairs
        for a in keys:
            for b in keys:
                payload, ops = C.make_table([(a, C.tag(1), b"x"), (b, C.tag(1), b"y")])
                host_equals_model(payload, ops, group)


def test_build_host_empty_and_single():
    payload, ops = C.make_table([])
    order, tot = MT.build_host(payload, ops)
    assert order.size == 0 and tot == dict(entries=0, user_keys=0, status=0)
    payload, ops = C.make_table([(b"", C.tag(1), b"")])
    assert MT.build_host(payload, ops)[1] == dict(entries=1, user_keys=1, status=0)


def test_build_host_random_tables():
    rng = np.random.default_rng(2024)
    for trial in range(200):
        n = int(rng.integers(0, 300))
        items = C.random_items(rng, n, alphabet=[2, 4, 26][trial % 3], seqs=[2, 50][trial % 2])
        gaps = rng.integers(0, 9, size=n) if trial % 2 else None
        payload, ops = C.make_table(items, gaps)
        host_equals_model(payload, ops, f"trial {trial}")


def test_build_host_bad_extents():
    payload, ops = C.make_table(C.random_items(np.random.default_rng(3), 20))
    P = len(payload)
    for field, off, ln in (("key", P - 3, 4), ("key", P + 1, 0), ("key", (1 << 64) - 2, 8), ("val", P, 1),
                           ("val", (1 << 64) - 1, 0xFFFFFFFF)):
        bad = ops.copy()
        bad[7][field + "_off"], bad[7][field + "_len"] = off, ln
        order, tot = MT.build_host(payload, bad)
        assert tot == dict(entries=20, user_keys=0, status=C.BAD_OP) and order.size == 0, (field, off, ln)
    ok = ops.copy()  # an empty extent at the very end is inside
    ok[7]["key_off"], ok[7]["key_len"] = P, 0
    assert MT.build_host(payload, ok)[1]["status"] == 0


# ---- get ----
def test_get_host_against_model():
    rng = np.random.default_rng(77)
    for items in (C.tag_items(), C.corner_items(), C.random_items(rng, 150, seqs=6), []):
        payload, ops = C.make_table(items)
        order, tot = MT.build_host(payload, ops)
        extra = [(b"", 0), (b"\xff" * 9, 5), (b"zzzz", C.MAX_SEQUENCE), (b"versions", 76), (b"versions", 0),
                 (b"versions", C.MAX_SEQUENCE + 1), (b"dup", 42), (b"dup", 41)]
        for key, seq in C.queries_for(payload, ops, extra=extra):
            got = MT.get_host(payload, ops, order, tot, key, seq)
            want = C.model_get(payload, ops, order.tolist(), key, seq)
            assert got == want, (key[:30], seq, got, want)


def test_get_host_rules():
    items = [(b"k", C.tag(10), b"ten"), (b"k", C.tag(20, 0), b""), (b"k", C.tag(30), b"thirty")]
    payload, ops = C.make_table(items)
    order, tot = MT.build_host(payload, ops)
    get = lambda key, seq: MT.get_host(payload, ops, order, tot, key, seq)
    assert get(b"k", 9)["status"] == C.ABSENT
    assert (get(b"k", 10)["status"], get(b"k", 10)["op"]) == (C.FOUND, 0)
    assert payload[get(b"k", 19)["val_off"]:][:get(b"k", 19)["val_len"]] == b"ten"
    assert (get(b"k", 20)["status"], get(b"k", 20)["op"]) == (C.DELETED, 1)   # a DELETION exactly at the snapshot
    assert get(b"k", 29)["status"] == C.DELETED
    assert (get(b"k", 30)["status"], get(b"k", C.MAX_SEQUENCE)["op"]) == (C.FOUND, 2)
    assert get(b"k", C.MAX_SEQUENCE + 1)["status"] == C.BAD_SEQ
    assert get(b"j", 30)["status"] == get(b"l", 30)["status"] == get(b"k\x00", 30)["status"] == C.ABSENT
    assert get(b"", 30)["status"] == C.ABSENT
    assert MT.get_host(payload, ops, order, dict(tot, status=C.BAD_OP), b"k", 30)["status"] == C.NO_TABLE


# ---- the reference's own tests, under both orders ----
def reference_strings():
    out = [(W.ref_multiple().bytes(), "Put(baz, boo)@102Delete(box)@101Put(foo, bar)@100"),
           (W.ref_corruption().bytes(), "Put(foo, bar)@200ParseError()")]
    return out + W.ref_append_stages()


def test_reference_memtable_order_reproduces_the_reference_strings():
    """The entry-compare restatement of the reference's MemTable yields every
    expected string of write_batch.rs:240-297 verbatim."""
    for rep, want in reference_strings():
        assert C.reference_memtable_print(rep) == want


def test_product_order_differs_only_in_the_last_append_string():
    """Internal-key order (C++ LevelDB's) yields the same strings except the
    one the reference marks "the order is different from cpp": the newer Put(b)
    comes first.  The model and the host twin agree on it."""
    cases = reference_strings()
    host = lambda payload, ops: MT.build_host(payload, ops)[0]
    for rep, want in cases[:-1]:
        assert C.product_print(rep) == want == C.product_print(rep, host)
    want = "Put(a, va)@200Put(b, vb)@202Put(b, vb)@201Delete(foo)@203"
    assert C.product_print(cases[-1][0]) == want == C.product_print(cases[-1][0], host)
    assert cases[-1][1] == "Put(a, va)@200Put(b, vb)@201Put(b, vb)@202Delete(foo)@203"


def test_reference_entry_order_depends_on_length_and_value_bytes():
    """Why the reference's entry order is not the product's: the length byte is
    compared first ("b" before "aa"), and a version's place depends on its
    value's last bytes."""
    b = W.WriteBatch().set_sequence(1).put(b"aa", b"v").put(b"b", b"v")
    assert C.reference_memtable_print(b.bytes()) == "Put(b, v)@2Put(aa, v)@1"
    assert C.product_print(b.bytes()) == "Put(aa, v)@1Put(b, v)@2"


# ---- the kernels ----
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernels_do_not_spill():
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-munsafe-fp-atomics", "--cuda-device-only", "-c", "-o", os.devnull, SOURCE,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    spills, scratch, name = {}, {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name:
            spills[name] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    for k in ("mt_tile_sort", "mt_merge", "mt_order", "mt_totals", "mt_get"):
        hits = {n: (spills[n], scratch[n]) for n in spills if k in n}
        assert hits and all(v == (0, 0) for v in hits.values()), (k, hits)


# ---- argument checks ----
def test_build_device_argument_checks():
    """Every argument error of lv_memtable_build_device is found on the host,
    before any device call: LV_ERR_INVALID and a message, with pointers that
    are never dereferenced and no GPU in the machine."""
    L = MT._bind()
    vp = ctypes.c_void_p
    cap, nbytes = 100, 4096
    wsb = L.lv_memtable_build_workspace_bytes(cap)
    err = lambda: lvgpu.lib().lv_last_error()

    def call(pay=vp(0x100000), n=nbytes, ops=vp(0x900000), nops=vp(0x500000), up=vp(0x600000), c=cap,
             order=vp(0xA00000), tot=vp(0xC00000), flags=0, w=vp(0x4000000), wb=wsb):
        return L.lv_memtable_build_device(pay, n, ops, nops, up, c, order, tot, flags, w, wb, None)

    # NULL pointers
    assert call(pay=None) == INVALID and b"null d_payload" in err()
    assert call(ops=None) == INVALID and b"null d_ops" in err()
    assert call(nops=None) == INVALID and b"null d_n_ops" in err()
    assert call(order=None) == INVALID and b"null d_order" in err()
    assert call(tot=None) == INVALID and b"null d_totals" in err()
    assert call(w=None) == INVALID and b"workspace" in err()
    # alignment: d_ops 16, d_order 4, d_totals 8, workspace 16
    assert call(ops=vp(0x900008)) == INVALID and b"d_ops" in err() and b"16-byte" in err()
    assert call(order=vp(0xA00002)) == INVALID and b"d_order" in err() and b"4-byte" in err()
    assert call(tot=vp(0xC00004)) == INVALID and b"d_totals" in err()
    assert call(nops=vp(0x500004)) == INVALID and b"d_n_ops" in err()
    assert call(w=vp(0x4000008)) == INVALID and b"aligned" in err()
    # workspace one byte short
    assert call(wb=wsb - 1) == INVALID and b"workspace too small" in err()
    # no flag is defined
    assert call(flags=1) == INVALID and b"flag" in err()
    assert call(flags=0x80000000) == INVALID and b"flag" in err()
    # indices are 32-bit
    assert call(c=0xFFFFFFFF, wb=1 << 62) == INVALID and b"op_cap" in err()
    # d_order[0, op_cap) inside / straddling d_ops or the payload, at either end
    assert call(order=vp(0x900000 + 32 * cap - 4)) == INVALID and b"overlaps d_ops" in err()
    assert call(order=vp(0x900000 - 4 * cap + 4)) == INVALID and b"overlaps d_ops" in err()
    assert call(order=vp(0x100000 + nbytes - 4)) == INVALID and b"overlaps d_payload" in err()
    assert call(order=vp(0x100000 - 4 * cap + 4)) == INVALID and b"overlaps d_payload" in err()
    # What passes the checks goes on to the device: with no GPU that is the
    # runtime's error, never LV_ERR_INVALID and never a host fallback.  (A NULL
    # upstream status; an order that ends where the ops start; nothing at all.)
    import torch
    if not torch.cuda.is_available():
        assert call() not in (0, INVALID)
        assert call(up=None) not in (0, INVALID)
        assert call(order=vp(0x900000 - 4 * cap)) not in (0, INVALID)
        assert call(pay=None, n=0, ops=None, c=0, order=None,
                    wb=L.lv_memtable_build_workspace_bytes(0)) not in (0, INVALID)
        assert lvgpu.lib().lv_last_error()


def test_get_device_argument_checks():
    L = MT._bind()
    vp = ctypes.c_void_p
    err = lambda: lvgpu.lib().lv_last_error()

    def call(pay=vp(0x100000), n=4096, ops=vp(0x900000), order=vp(0xA00000), tot=vp(0xC00000), qk=vp(0xD00000),
             qb=512, qo=vp(0xE00000), ql=vp(0xE10000), qs=vp(0xE20000), nq=10, res=vp(0xF00000), flags=0):
        return L.lv_memtable_get_device(pay, n, ops, order, tot, qk, qb, qo, ql, qs, nq, res, flags, None)

    assert call(pay=None) == INVALID and b"null d_payload" in err()
    assert call(tot=None) == INVALID and b"null d_totals" in err()
    assert call(qk=None) == INVALID and b"null d_qkeys" in err()
    assert call(ops=None) == INVALID and b"null" in err()
    assert call(order=None) == INVALID and b"null" in err()
    for k in ("qo", "ql", "qs"):
        assert call(**{k: None}) == INVALID and b"null query array" in err(), k
    assert call(res=None) == INVALID and b"null d_results" in err()
    assert call(ops=vp(0x900008)) == INVALID and b"d_ops" in err()
    assert call(order=vp(0xA00002)) == INVALID and b"d_order" in err()
    assert call(tot=vp(0xC00004)) == INVALID and b"d_totals" in err()
    assert call(qo=vp(0xE00004)) == INVALID and b"8-byte" in err()
    assert call(qs=vp(0xE20004)) == INVALID and b"8-byte" in err()
    assert call(ql=vp(0xE10002)) == INVALID and b"d_q_len" in err()
    assert call(res=vp(0xF00004)) == INVALID and b"d_results" in err()
    assert call(flags=2) == INVALID and b"flag" in err()
    assert call(nq=0xFFFFFFFF) == INVALID and b"nq" in err()
    import torch
    if not torch.cuda.is_available():
        assert call() not in (0, INVALID)
        assert call(nq=0, qo=None, ql=None, qs=None, res=None) not in (0, INVALID)
        assert lvgpu.lib().lv_last_error()
