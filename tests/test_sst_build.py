"""lv_sst_build_host, lv_sst_build_file_bound and the argument checks of
lv_sst_build_device, without a GPU: the hand-derived fixtures, the host twin
against the Python model (tests/sst_build_cases.py) byte for byte, the model
reader over the host twin's file, the index keys' ordering, the format
decoders over what was written, every status, the file bound."""
import ctypes
import json
import os

import numpy as np
import pytest

import lvgpu
import lvgpu.memtable as MT
import lvgpu.table as T
import memtable_cases as M
import sst_build_cases as C
from conftest import GOLDEN
from memtable_cases import make_table, tag

CASES = C.cases()


def host_build(items, bs=None, ri=None, **kw):
    payload, ops = make_table(items)
    order, tot = MT.build_host(payload, ops)
    return payload, ops, order, tot, T.build_host(payload, ops, order, tot, bs, ri, **kw)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "sst_build_one_entry.json")) as f:
        return json.load(f)


def hexb(s):
    return bytes.fromhex(s.replace(" ", ""))


def test_one_entry_fixture(golden):
    g = golden["one_entry"]
    want = b""
    for name in ("data_block", "metaindex_block", "index_block"):
        raw = hexb(g[name])
        want += raw + b"\x00" + lvgpu.mask(lvgpu.value(raw + b"\x00")).to_bytes(4, "little")
    want += hexb(g["footer"])
    lay = g["layout"]
    assert len(want) == lay["file_bytes"] == 114 and len(hexb(g["footer"])) == 48
    items = [(hexb(g["key"]), tag(g["sequence"], g["type"]), hexb(g["value"]))]
    payload, ops = make_table(items)
    file, handles, tot = C.model_build(payload, ops)
    assert file == want
    assert handles == [tuple(lay["data"]), tuple(lay["metaindex"]), tuple(lay["index"])]
    _, _, _, _, (hfile, hhandles, htot) = host_build(items)  # NULL opt: the defaults
    assert hfile == want and hhandles == handles and htot == tot
    _, _, _, _, (hfile, _, _) = host_build(items, g["block_size"], g["restart_interval"])
    assert hfile == want
    assert tot == dict(entries=1, data_blocks=1, file_bytes=114, metaindex_offset=26, metaindex_size=8,
                       index_offset=39, index_size=22, status=0)


def test_shortened_separator_fixture(golden):
    g = golden["shortened_separator"]
    a, b, want = hexb(g["last_user_key"]), hexb(g["next_user_key"]), hexb(g["index_key"])
    assert C.shortest_separator(C.ikey(a, tag(7)), C.ikey(b, tag(3))) == want
    items = [(a, tag(7), b"v"), (b, tag(3), b"w")]
    _, _, _, _, (file, handles, tot) = host_build(items, 1, 16)  # block_size 1: one entry per block
    assert tot["data_blocks"] == 2
    _, index, _ = C.read_table(file)
    assert index[0][0] == want and index[1][0] == b"b" + C.MAXTAG  # the last block: short_successor


@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_is_the_model(name):
    items, bs, ri = CASES[name]
    payload, ops, order, mt, (file, handles, tot) = host_build(items, bs, ri)
    want_file, want_handles, want_tot = C.model_build(payload, ops, bs, ri)
    assert tot == want_tot
    assert file == want_file
    assert handles == want_handles
    assert order.tolist() == M.model_order(payload, ops)
    # the bound
    assert T.file_bound(len(payload), len(ops), bs, ri) >= len(want_file)
    if not items:
        assert file == b"" and handles == [] and tot["file_bytes"] == 0 and tot["data_blocks"] == 0
        return
    # the reader returns exactly the memtable's entries in order
    entries, index, blocks = C.read_table(file)
    assert entries == C.entries_of(payload, ops)
    assert [h for _, h in index] == handles[:-2] and len(blocks) == tot["data_blocks"]
    # last key of b <= index key b < first key of b + 1
    cmp_ = lambda x, y: MT.compare(C.user(x), int.from_bytes(x[-8:], "little"), C.user(y),
                                   int.from_bytes(y[-8:], "little"))
    for b, ((key, _), ents) in enumerate(zip(index, blocks)):
        assert cmp_(ents[-1][0], key) <= 0, (b, ents[-1][0], key)
        if b + 1 < len(blocks):
            # strictly, unless an exact duplicate (same key, same tag: upstream never has one) straddles
            # the boundary: then the three keys are one and nothing can lie between them
            nxt = blocks[b + 1][0][0]
            assert cmp_(key, nxt) < 0 or ents[-1][0] == key == nxt, (b, key, nxt)
    # an index seek finds every entry (the first of its duplicates)
    for k, v in entries[:: max(len(entries) // 50, 1)]:
        assert C.index_seek(index, blocks, k)[0] == k
    # the project's decoders accept what was written
    foot = T.Footer.decode_from(file[-48:])
    assert (foot.metaindex_handle.offset, foot.metaindex_handle.size) == handles[-2]
    assert (foot.index_handle.offset, foot.index_handle.size) == handles[-1]
    raw = file[handles[-1][0]:handles[-1][0] + handles[-1][1]]
    idx_entries, _ = C.block_entries(raw)
    for (_, value), h in zip(idx_entries, handles):
        got, used = T.BlockHandle.decode_from(value)
        assert (got.offset, got.size) == h and used == len(value)


def test_cases_hit_what_they_name():
    """The case tables are not hollow: restart cadence, a block end on a
    restart, the three thresholds, prefixes across the key / tag edge."""
    def shape(name):
        items, bs, ri = CASES[name]
        payload, ops = make_table(items)
        file, handles, tot = C.model_build(payload, ops, bs, ri)
        blocks = [C.block_entries(file[o:o + s]) for o, s in handles[:-2]]
        return tot, blocks
    for n, restarts in ((1, 1), (15, 1), (16, 1), (17, 2), (32, 2), (33, 3)):
        tot, blocks = shape(f"count_{n}")
        assert tot["data_blocks"] == 1 and len(blocks[0][1]) == restarts
    tot, blocks = shape("end_on_restart")
    assert any(len(ents) % 4 == 0 for ents, _ in blocks[:-1]) and tot["data_blocks"] > 3
    assert shape("threshold_-1")[0]["data_blocks"] == 1
    assert shape("threshold_+0")[0]["data_blocks"] == 2 and shape("threshold_+1")[0]["data_blocks"] == 2
    for d in (-1, 0, 1):
        items, bs, ri = CASES[f"threshold_{d:+d}"]
        bb = C.BlockBuilder(ri)
        for k, t, v in items[:2]:
            bb.add(C.ikey(k, t), v)
        assert bb.estimate() == bs + d
    tot, blocks = shape("one_big_entry")
    assert tot["data_blocks"] == 2 and [len(e) for e, _ in blocks] == [2, 1]
    # the shared prefix runs into the tag (12 > 4 user bytes), and from a tag into user bytes
    payload, ops = make_table(CASES["tag_high_byte"][0])
    ents = C.entries_of(payload, ops)
    assert C.common_prefix(ents[0][0], ents[1][0]) > 4
    payload, ops = make_table(CASES["tag_into_key"][0])
    ents = C.entries_of(payload, ops)
    assert ents[0][0][:1] == b"a" and C.common_prefix(ents[0][0], ents[1][0]) >= 3 > len(C.user(ents[0][0]))
    # exact duplicates: non_shared = 0
    items, bs, ri = CASES["duplicates"]
    payload, ops = make_table(items)
    file, handles, _ = C.model_build(payload, ops, bs, ri)
    assert file[18:21] == bytes([11, 0, 4])  # the second entry, after 18 bytes: shared 11, non_shared 0, value 4
    # varint widths appear in the bytes
    for w in (127, 128, 16383, 16384):
        payload, ops = make_table(CASES[f"varint_shared_{w}"][0])
        ents = C.entries_of(payload, ops)
        assert C.common_prefix(ents[0][0], ents[1][0]) == w
    # successor branches
    S = C.short_successor
    assert S(C.ikey(b"", 5)) == C.ikey(b"", 5) and S(C.ikey(b"\xff\xff", 5)) == C.ikey(b"\xff\xff", 5)
    assert S(C.ikey(b"\xff\xff\x41\x42", 5)) == b"\xff\xff\x42" + C.MAXTAG and S(C.ikey(b"k", 5)) == C.ikey(b"k", 5)
    assert S(C.ikey(b"hello", 5)) == b"i" + C.MAXTAG
    # separator branches
    sep = lambda a, b: C.shortest_separator(C.ikey(a, 9), C.ikey(b, 8))
    assert sep(b"abc", b"abcd") == C.ikey(b"abc", 9) and sep(b"same", b"same") == C.ikey(b"same", 9)
    assert sep(b"ab\xffq", b"ac") == C.ikey(b"ab\xffq", 9) and sep(b"abc", b"abd") == C.ikey(b"abc", 9)
    assert sep(b"abcd", b"abz") == b"abd" + C.MAXTAG and sep(b"a", b"c") == b"b" + C.MAXTAG


def test_tile_structure_on_the_host():
    """The tile cases of the GPU suite, on the host twin: block chains that
    cross every tile edge of the device path."""
    for ri in (1, 2, 16):
        for n in (T.SB_TILE - 1, T.SB_TILE + 1):
            items = C.tile_items(n, seed=ri)
            payload, ops, order, mt, (file, handles, tot) = host_build(items, 32, ri)
            want_file, want_handles, want_tot = C.model_build(payload, ops, 32, ri)
            assert file == want_file and handles == want_handles and tot == want_tot
            assert tot["data_blocks"] > n // 4


def test_statuses():
    items, bs, ri = CASES["random_small_blocks"]
    payload, ops = make_table(items)
    order, mt = MT.build_host(payload, ops)
    file, handles, tot = C.model_build(payload, ops, bs, ri)
    nb, fb = tot["data_blocks"], tot["file_bytes"]
    untouched = lambda f, h: set(f) <= {0xA5} and bool((h == 0xA5A5A5A5A5A5A5A5).all())
    # a sizing pass: file == NULL, file_cap == 0; nothing written, the true totals, no FILE_OVER
    _, _, t = T.build_host(payload, ops, order, mt, bs, ri, sizing=True)
    assert t == tot
    # ... with a handle array too small: HANDLE_OVER, the array untouched
    _, h, t = T.build_host(payload, ops, order, mt, bs, ri, sizing=True, block_cap=nb - 1)
    assert t == dict(tot, status=C.HANDLE_OVER) and untouched(b"", h)
    # exact capacities work; one less of either does not
    f, h, t = T.build_host(payload, ops, order, mt, bs, ri, file_cap=fb, block_cap=nb)
    assert f == file and h == handles and t == tot
    f, h, t = T.build_host(payload, ops, order, mt, bs, ri, file_cap=fb - 1, block_cap=nb)
    assert t == dict(tot, status=C.FILE_OVER) and untouched(f, h)
    f, h, t = T.build_host(payload, ops, order, mt, bs, ri, file_cap=fb, block_cap=nb - 1)
    assert t == dict(tot, status=C.HANDLE_OVER) and untouched(f, h)
    f, h, t = T.build_host(payload, ops, order, mt, bs, ri, file_cap=10, block_cap=0)
    assert t == dict(tot, status=C.FILE_OVER | C.HANDLE_OVER) and untouched(f, h)
    # NO_TABLE: the memtable's status is not 0; entries = 0
    f, h, t = T.build_host(payload, ops, order, dict(mt, status=M.BAD_OP), bs, ri, file_cap=fb, block_cap=nb)
    assert t == dict(zip(C.TOTALS, [0] * 7 + [C.NO_TABLE])) and untouched(f, h)
    # ... or an extent is outside the payload (not the memtable build's arguments)
    bad = ops.copy()
    bad[3]["val_len"] = len(payload) + 1
    f, h, t = T.build_host(payload, bad, order, mt, bs, ri, file_cap=fb, block_cap=nb)
    assert t["status"] == C.NO_TABLE and t["entries"] == 0 and untouched(f, h)
    # the empty memtable: nothing written, no file
    payload0, ops0 = make_table([])
    order0, mt0 = MT.build_host(payload0, ops0)
    f, h, t = T.build_host(payload0, ops0, order0, mt0, file_cap=64, block_cap=4)
    assert t == dict(zip(C.TOTALS, [0] * 8)) and f == b"" and h == []


def test_block_large_through_the_sizing_pass():
    """A value extent of 2^32 - 1 bytes claimed inside a 2^32-byte payload that
    is not allocated: the sizing pass reads key bytes only, computes in u64 and
    reports BLOCK_LARGE with the true sizes.  Two such values overlap."""
    payload, ops = make_table([(b"a", tag(2), b"x"), (b"b", tag(1), b"y"), (b"c", tag(3), b"z")])
    ops = ops.copy()
    big = (1 << 32) - 1
    for i in (1, 2):
        ops[i]["val_off"], ops[i]["val_len"] = 0, big
    order, mt = MT.build_host(payload, ops[:0])  # (the memtable twin would check the extents)
    order = np.array([0, 1, 2], dtype=np.uint32)
    mt = dict(entries=3, user_keys=3, status=0)
    for bs, blocks in ((1 << 30, 2), (16, 3)):
        _, _, t = T.build_host(payload, ops, order, mt, bs, 16, sizing=True, payload_bytes=1 << 32)
        assert t["status"] == C.BLOCK_LARGE and t["entries"] == 3 and t["data_blocks"] == blocks
        assert t["file_bytes"] > 2 * big and t["index_offset"] > 2 * big
    # one byte less than the limit is not large: raw = 2^32 - 2
    ops[2]["val_len"] = 0
    ops[1]["val_len"] = big - 1 - (1 + 1 + 5 + 9) - 8
    ops[0]["val_len"] = 0
    ops[0]["key_len"] = 0
    _, _, t = T.build_host(payload, ops, np.array([1], dtype=np.uint32), dict(entries=1, user_keys=1, status=0),
                           1 << 30, 16, sizing=True, payload_bytes=1 << 32)
    assert t["status"] == 0 and t["metaindex_offset"] == big - 1 + 5
    ops[1]["val_len"] += 1
    _, _, t = T.build_host(payload, ops, np.array([1], dtype=np.uint32), dict(entries=1, user_keys=1, status=0),
                           1 << 30, 16, sizing=True, payload_bytes=1 << 32)
    assert t["status"] == C.BLOCK_LARGE


def test_file_bound_on_adversarial_tables():
    rng = np.random.default_rng(77)
    worst = 0.0
    for items, bs, ri in C.adversarial_tables(rng, 200):
        payload, ops = make_table(items)
        file, _, tot = C.model_build(payload, ops, bs, ri)
        bound = T.file_bound(len(payload), len(ops), bs, ri)
        assert bound >= len(file), (len(payload), len(ops), bs, ri, bound, len(file))
        worst = max(worst, len(file) / bound)
    assert worst > 0.5  # not vacuous: some table uses more than half of its bound
    assert T.file_bound(0, 0) == 0 and T.file_bound((1 << 64) - 1, 5) == (1 << 64) - 1  # saturates


def test_host_argument_checks():
    L = T._bind_build()
    payload, ops = make_table([(b"k", tag(1), b"v")])
    order, mt = MT.build_host(payload, ops)
    for bs, ri in ((0, 16), ((1 << 30) + 1, 16), (4096, 0), (4096, 1025)):
        with pytest.raises(lvgpu.LvError):
            T.build_host(payload, ops, order, mt, bs, ri)
    T.build_host(payload, ops, order, mt, 1 << 30, 1024)
    tot = T.BuildTotals()
    m = T.MtTotals(1, 1, 0)
    assert L.lv_sst_build_host(None, 0, None, None, ctypes.byref(m), None, None, 0, None, 0, None) == -1
    assert L.lv_sst_build_host(None, 0, None, None, None, None, None, 0, None, 0, ctypes.byref(tot)) == -1
    assert L.lv_sst_build_host(None, 0, None, None, ctypes.byref(m), None, None, 0, None, 0, ctypes.byref(tot)) == -1
    assert L.lv_sst_build_host(None, 0, None, None, ctypes.byref(m), None, None, 8, None, 0, ctypes.byref(tot)) == -1


def test_device_argument_checks_before_any_device_call():
    """Every check fails with LV_ERR_INVALID and a message before the GPU is
    touched; a well-formed call without a GPU fails with the runtime's error."""
    import torch
    L = T._bind_build()
    vp = ctypes.c_void_p
    ws = T.build_workspace_bytes(100, 10)
    assert ws > 0 and T.build_workspace_bytes(1 << 32, 1) == 0
    assert T.build_workspace_bytes(2000, 10) > ws and T.build_workspace_bytes(100, 1000) > ws
    good = dict(payload=vp(0x10000), pn=4096, ops=vp(0x20000), order=vp(0x30000), mt=vp(0x40000), cap=100, opt=None,
                file=vp(0x50000), fcap=4096, handles=vp(0x60000), bcap=10, tot=vp(0x70000), flags=0,
                ws=vp(0x100000), wsn=ws)

    def call(**kw):
        a = dict(good, **kw)
        return L.lv_sst_build_device(a["payload"], a["pn"], a["ops"], a["order"], a["mt"], a["cap"], a["opt"],
                                     a["file"], a["fcap"], a["handles"], a["bcap"], a["tot"], a["flags"], a["ws"],
                                     a["wsn"], None)

    def opt(bs, ri):
        return ctypes.byref(T.BuildOptions(bs, ri))
    bad = [(dict(flags=1), b"flag"), (dict(opt=opt(0, 16)), b"block_size"), (dict(opt=opt((1 << 30) + 1, 16)), b"block_size"),
           (dict(opt=opt(4096, 0)), b"restart_interval"), (dict(opt=opt(4096, 1025)), b"restart_interval"),
           (dict(tot=None), b"d_totals"), (dict(tot=vp(0x70004)), b"8-byte"), (dict(mt=None), b"d_mt_totals"),
           (dict(mt=vp(0x40004)), b"8-byte"), (dict(payload=None), b"d_payload"), (dict(cap=1 << 32), b"op_cap"),
           (dict(ops=None), b"d_ops"), (dict(ops=vp(0x20008)), b"16-byte"), (dict(order=None), b"d_order"),
           (dict(order=vp(0x30002)), b"4-byte"), (dict(file=None), b"d_file"), (dict(file=vp(0x50008)), b"16-byte"),
           (dict(handles=None), b"d_handles"), (dict(handles=vp(0x60004)), b"8-byte"), (dict(ws=None), b"workspace"),
           (dict(ws=vp(0x100008)), b"16-byte"), (dict(wsn=ws - 1), b"workspace too small"),
           (dict(file=vp(0x10010)), b"d_file overlaps d_payload"), (dict(file=vp(0x20000 - 16)), b"d_file overlaps d_ops"),
           (dict(file=vp(0x30010)), b"d_file overlaps d_order"), (dict(handles=vp(0x10ff8)), b"d_handles overlaps d_payload"),
           (dict(handles=vp(0x50100)), b"d_file overlaps d_handles"), (dict(bcap=(1 << 32) - 3, wsn=1 << 62), b"block_cap")]
    for kw, msg in bad:
        assert call(**kw) == -1, kw
        assert msg in L.lv_last_error(), (kw, L.lv_last_error())
    if not torch.cuda.is_available():  # no host fallback: the runtime's error, loudly
        assert call() != 0 and L.lv_last_error()
        assert call(opt=opt(1, 1), cap=0, ops=None, order=None, fcap=0, file=None, wsn=1 << 20) != 0


def test_constants_match_the_header_and_the_knobs():
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "lvgpu", "table.h")).read()
    knobs = open(os.path.join(ROOT, "leveldb-rs_amd", "csrc", "lvk", "knobs.h")).read()
    define = lambda text, name: int(re.search(r"#define %s\s+\(?(\d+)" % name, text).group(1))
    assert T.SB_TILE == define(knobs, "LVK_SB_TILE") and T.SB_WAVE_COPY == define(knobs, "LVK_SB_WAVE_COPY")
    assert T.SB_COPY_LANES == define(knobs, "LVK_SB_COPY_LANES")
    assert (T.DEFAULT_BLOCK_SIZE, T.DEFAULT_RESTART_INTERVAL) == (define(hdr, "LV_SST_DEFAULT_BLOCK_SIZE"),
                                                                 define(hdr, "LV_SST_DEFAULT_RESTART_INTERVAL"))
    for bit, name in T.BUILD_STATUS.items():
        assert bit == define(hdr, "LV_SST_BUILD_" + name)
    assert ctypes.sizeof(T.BuildTotals) == 64 and ctypes.sizeof(T.BuildOptions) == 8
