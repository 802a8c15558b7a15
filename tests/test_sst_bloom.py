"""Bloom filter blocks without a GPU: the hand-derived fixture, the host
scalars and the host twins (lv_sst_build_bloom_host, lv_sst_bloom_open_host,
lv_sst_get_bloom_host) against the Python model (tests/sst_bloom_cases.py)
byte for byte, the upstream hash KAT, the k rule, the closed form of the
filter count against the serial builder, the file bound, every `why`, the
damaged images, the argument checks of the device entry points."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import lvgpu
import lvgpu.memtable as MT
import lvgpu.table as T
import memtable_cases as M
import sst_bloom_cases as B
import sst_build_cases as S
import sst_get_cases as G
from conftest import GOLDEN, ROOT
from memtable_cases import MAX_SEQUENCE, make_table, tag

CASES = B.cases()


def host_build(items, bpk=10, bs=None, ri=None, **kw):
    payload, ops = make_table(items)
    order, tot = MT.build_host(payload, ops)
    return payload, ops, order, tot, T.build_bloom_host(payload, ops, order, tot, bpk, bs, ri, **kw)


def hexb(s):
    return bytes.fromhex(s.replace(" ", ""))


def test_one_entry_fixture():
    with open(os.path.join(GOLDEN, "sst_bloom_one_entry.json")) as f:
        g = json.load(f)["one_entry"]
    meta = hexb(g["metaindex_head"]) + g["metaindex_name_ascii"].encode() + hexb(g["metaindex_tail"])
    assert g["metaindex_name_ascii"].encode() == B.NAME == T.BLOOM_NAME and len(B.NAME) == 34
    want = b""
    for raw in (hexb(g["data_block"]), hexb(g["filter_block"]), meta, hexb(g["index_block"])):
        want += raw + b"\x00" + lvgpu.mask(lvgpu.value(raw + b"\x00")).to_bytes(4, "little")
    want += hexb(g["footer"])
    lay = g["layout"]
    assert len(want) == lay["file_bytes"] == 176
    key = hexb(g["key"])
    assert B.bloom_hash(key) == T.bloom_hash(key) == int(g["bloom_hash"], 16) and B.bloom_k(g["bits_per_key"]) == g["k"]
    items = [(key, tag(g["sequence"], g["type"]), hexb(g["value"]))]
    payload, ops = make_table(items)
    file, handles, tot, btot = B.model_build(payload, ops, g["bits_per_key"])
    assert file == want
    assert handles == [tuple(lay[n]) for n in ("data", "filter", "metaindex", "index")]
    assert btot == dict(filter_offset=26, filter_size=18, filters=1, filter_keys=1)
    _, _, _, _, (hfile, hhandles, htot, hbtot) = host_build(items, g["bits_per_key"])  # NULL opt: the defaults
    assert hfile == want and hhandles == handles and htot == tot and hbtot == btot
    assert T.Footer.decode_from(file[-48:]) == T.Footer(T.BlockHandle(49, 47), T.BlockHandle(101, 22))
    # the filter holds the key; with 6 of 64 bits set it rejects most others
    filt = hexb(g["filter_block"])[:9]
    assert B.key_may_match(b"k", filt) and T.bloom_key_may_match(b"k", filt)
    others = [b"key%d" % i for i in range(50)]
    assert [T.bloom_key_may_match(o, filt) for o in others] == [B.key_may_match(o, filt) for o in others]
    assert sum(B.key_may_match(o, filt) for o in others) < 5


def test_upstream_hash_kat():
    """The reference's own KAT of the hash at the Bloom seed (util/hash.rs)."""
    assert T.bloom_hash(b"\x62") == 0xEF1345C4 == B.bloom_hash(b"\x62")
    from lvgpu.hash import hash as lv_hash
    rng = np.random.default_rng(2)
    for n in list(range(0, 20)) + [63, 64, 65, 1000]:
        key = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        assert T.bloom_hash(key) == B.bloom_hash(key) == lv_hash(key, B.SEED), n


def test_k_rule():
    """k = bpk * 69 / 100 in integers, clamped to [1, 30]: upstream's
    (size_t)(bpk * 0.69) for every bpk the call takes (and up to 299)."""
    for bpk in range(1, 300):
        want = min(30, max(1, int(bpk * 0.69)))
        assert B.bloom_k(bpk) == want, bpk
    for bpk in range(1, 65):
        f = T.bloom_create_filter([b"a", b"b"], bpk)
        assert f[-1] == B.bloom_k(bpk) and len(f) == T.bloom_filter_bytes(2, bpk) == max(8, (2 * bpk + 7) // 8) + 1


@pytest.mark.parametrize("bpk", [1, 10, 64])
def test_create_filter_is_the_model(bpk):
    rng = np.random.default_rng(bpk)
    for n in (0, 1, 6, 7, 63, 64, 65, 300):
        keys = [rng.integers(0, 256, size=int(rng.integers(0, 12)), dtype=np.uint8).tobytes() for _ in range(n)]
        f = T.bloom_create_filter(keys, bpk)
        assert f == B.create_filter(keys, bpk), (n, bpk)
        for k in keys:
            assert T.bloom_key_may_match(k, f)
        for k in (b"", b"x", b"other", b"\xff" * 9):
            assert T.bloom_key_may_match(k, f) == B.key_may_match(k, f)
    # short filters, and a k byte above 30
    assert not T.bloom_key_may_match(b"a", b"") and not T.bloom_key_may_match(b"a", b"\x06")
    assert T.bloom_key_may_match(b"a", bytes(8) + b"\x1f") and not T.bloom_key_may_match(b"a", bytes(8) + b"\x1e")


@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_is_the_model(name):
    items, bs, ri, bpk = CASES[name]
    payload, ops, order, mt, (file, handles, tot, btot) = host_build(items, bpk, bs, ri)
    want = B.model_build(payload, ops, bpk, bs, ri)
    assert (tot, btot) == want[2:], name
    assert file == want[0] and handles == want[1], name
    bound = T.bloom_file_bound(len(payload), len(ops), bpk)
    assert len(file) <= bound, (name, len(file), bound)
    if not items:
        return
    # a reader without a filter policy reads the same entries; the sizing pass reports the same totals
    assert read_entries(file) == S.entries_of(payload, ops)
    _, _, stot, sbtot = T.build_bloom_host(payload, ops, order, mt, bpk, bs, ri, sizing=True)
    assert (stot, sbtot) == (tot, btot)
    # the closed form of the filter count against the serial builder's
    last = handles[-4][0]
    data_end = handles[-3][0]
    assert btot["filters"] == max((last >> 11) + 1, data_end >> 11)


def read_entries(file):
    """The entries of a bloom image by the open's handles (the model reader of
    sst_build_cases insists on an empty metaindex block)."""
    table, handles = G.model_open(file)
    assert table["status"] == 0
    entries = []
    for o, s in handles[:-2]:
        entries += S.block_entries(S.read_block(file, o, s))[0]
    return entries


def test_both_arms_of_the_filter_count():
    """The cases reach F = (last offset >> 11) + 1 above, at and below
    data_end >> 11, through the host twin's handles and count (which
    test_host_twin_is_the_model holds equal to the serial model's)."""
    seen = set()
    for name, (items, bs, ri, bpk) in CASES.items():
        if not items:
            continue
        _, _, _, _, (_, handles, _, btot) = host_build(items, bpk, bs, ri)
        a, b = (handles[-4][0] >> 11) + 1, handles[-3][0] >> 11
        seen.add((a > b) - (a < b))
        assert btot["filters"] == max(a, b), name
    assert seen == {-1, 0, 1}


def test_statuses_write_nothing():
    items, bs, ri, bpk = CASES["random_small_blocks"]
    payload, ops, order, mt, (file, handles, tot, btot) = host_build(items, bpk, bs, ri)
    nb, fb = tot["data_blocks"], tot["file_bytes"]
    zero = dict.fromkeys(B.BLOOM_TOTALS, 0)
    f, h, t, bt = T.build_bloom_host(payload, ops, order, mt, bpk, bs, ri, file_cap=fb - 1, block_cap=nb)
    assert t == dict(tot, status=S.FILE_OVER) and bt == zero and set(f) == {0xA5} and (h == T.HANDLE_CANARY).all()
    f, h, t, bt = T.build_bloom_host(payload, ops, order, mt, bpk, bs, ri, file_cap=fb, block_cap=nb - 1)
    assert t == dict(tot, status=S.HANDLE_OVER) and bt == zero and set(f) == {0xA5} and (h == T.HANDLE_CANARY).all()
    f, h, t, bt = T.build_bloom_host(payload, ops, order, dict(mt, status=1), bpk, bs, ri, file_cap=fb, block_cap=nb)
    assert t == dict(zip(S.TOTALS, [0] * 7 + [S.NO_TABLE])) and bt == zero and set(f) == {0xA5}
    for bad_bpk, reserved in ((0, 0), (65, 0), (10, 1)):
        with pytest.raises(lvgpu.LvError):
            T.build_bloom_host(payload, ops, order, mt, bad_bpk, bs, ri, reserved=reserved)


def test_file_bound_holds():
    rng = np.random.default_rng(17)
    for items, bs, ri in S.adversarial_tables(rng, 120):
        for bpk in (1, 10, 64):
            payload, ops = make_table(items)
            order, mt = MT.build_host(payload, ops)
            _, _, tot, _ = T.build_bloom_host(payload, ops, order, mt, bpk, bs, ri, sizing=True)
            assert tot["file_bytes"] <= T.bloom_file_bound(len(payload), len(ops), bpk), (bs, ri, bpk)
    assert T.bloom_file_bound(100, 0, 10) == 0 and T.bloom_file_bound(1 << 63, 1 << 32, 64) == (1 << 64) - 1


def test_every_why_and_the_reader():
    wc, queries = B.why_cases()
    base = wc["ok"][0]
    queries = queries[::3]
    seen = set()
    for name, (image, why) in wc.items():
        table, bloom, wants = B.model_answers(image, queries)
        assert bloom["why"] == why and bloom["present"] == (why == 0), (name, bloom)
        htable, hbloom, got = B.host_answers(image, queries)
        assert htable == table and hbloom == bloom, (name, hbloom, bloom)
        assert got == wants, name
        seen.add(why)
        if not bloom["present"]:  # no filter: byte for byte the plain get
            assert got == [T.get_host(image, table, k, s) for k, s in queries], name
    assert seen == set(range(9))
    # a well-formed image: the filter never rejects a stored key, and what it rejects is absent
    table, bloom, wants = B.model_answers(base, queries)
    plain = [G.model_get(base, table, k, s) for k, s in queries]
    nf = 0
    for w, p in zip(wants, plain):
        if w["reserved"]:
            assert p["status"] == G.ABSENT and w == dict(p, reserved=1)
            nf += 1
        else:
            assert w == p
    assert nf > 0


def test_damaged_images_host_twin_is_the_model():
    for name, image, queries in B.damaged_cases(150):
        table, bloom, wants = B.model_answers(image, queries)
        htable, hbloom, got = B.host_answers(image, queries)
        assert hbloom == bloom, (name, hbloom, bloom)
        assert got == wants, name


def test_dump_for_the_host_check_program(tmp_path):
    """The file tools/sst_bloom_host_check.cc replays can be written (it holds
    the model's answers only; the program and the GPU suite compare the
    product with them)."""
    n = B.dump(str(tmp_path / "cases.bin"))
    assert n > 300 and os.path.getsize(tmp_path / "cases.bin") > 1000000


def test_absent_keys_are_filtered():
    """The guard against a vacuous read test: of 2,000 keys the table does not
    hold the model's filter rejects at least 90 % at 10 bits per key (about
    99 % is expected); the host twin rejects exactly the same ones."""
    items, bs, ri, bpk, absent = B.absent_source()
    payload, ops = make_table(items)
    image = B.model_build(payload, ops, bpk, bs, ri)[0]
    queries = [(k, MAX_SEQUENCE) for k in absent]
    _, _, wants = B.model_answers(image, queries)
    filtered = sum(w["reserved"] for w in wants)
    print("filtered", filtered, "of", len(absent))
    assert filtered >= 0.9 * len(absent) and all(w["status"] == G.ABSENT for w in wants)
    assert B.host_answers(image, queries)[2] == wants
    stored = [(k, MAX_SEQUENCE) for k, _, _ in items]
    assert all(w["status"] == G.FOUND and not w["reserved"] for w in B.model_answers(image, stored)[2])


def test_a_bloom_struct_of_another_file_reads_nothing_outside():
    """lv_sst_get_bloom_host with a bloom that was not written for this file:
    offsets beyond the file mean no filter."""
    items, bs, ri, bpk = CASES["block_256"]
    payload, ops = make_table(items)
    image = B.model_build(payload, ops, bpk, bs, ri)[0]
    table, bloom, _ = B.model_answers(image, [])
    queries = B.queries_for(payload, ops, bs, ri)[::11]
    for patch in (dict(filter_offset=len(image)), dict(filter_size=len(image)), dict(filter_size=4),
                  dict(array_offset=bloom["filter_size"]), dict(num=bloom["num"] + 1), dict(num=1 << 62),
                  dict(filter_offset=(1 << 64) - 3), dict(base_lg=64), dict(base_lg=1 << 40), dict(present=2)):
        b = dict(bloom, **patch)
        for k, s in queries:
            assert T.get_bloom_host(image, table, b, k, s) == B.model_get(image, table, b, k, s), patch


def test_device_argument_checks_before_any_device_call():
    import torch
    L = T._bind_bloom()
    vp = ctypes.c_void_p
    ws = T.build_bloom_workspace_bytes(100, 10)
    assert ws > T.build_workspace_bytes(100, 10) and T.build_bloom_workspace_bytes(1 << 32, 1) == 0
    assert T.build_bloom_workspace_bytes(0, (1 << 32) - 3) == 0
    good = dict(payload=vp(0x10000), pn=4096, ops=vp(0x20000), order=vp(0x30000), mt=vp(0x40000), cap=100, opt=None,
                bloom=ctypes.byref(T.BloomOptions(10, 0)), file=vp(0x50000), fcap=4096, handles=vp(0x60000), bcap=10,
                tot=vp(0x70000), btot=vp(0x80000), flags=0, ws=vp(0x100000), wsn=ws)

    def call(**kw):
        a = dict(good, **kw)
        return L.lv_sst_build_bloom_device(a["payload"], a["pn"], a["ops"], a["order"], a["mt"], a["cap"], a["opt"],
                                           a["bloom"], a["file"], a["fcap"], a["handles"], a["bcap"], a["tot"],
                                           a["btot"], a["flags"], a["ws"], a["wsn"], None)

    def bo(bpk, r=0):
        return ctypes.byref(T.BloomOptions(bpk, r))
    bad = [(dict(bloom=None), b"null bloom options"), (dict(bloom=bo(0)), b"bits_per_key"), (dict(bloom=bo(65)), b"bits_per_key"),
           (dict(bloom=bo(10, 1)), b"reserved"), (dict(btot=None), b"d_bloom_totals"), (dict(btot=vp(0x80004)), b"8-byte"),
           (dict(flags=1), b"flag"), (dict(tot=None), b"d_totals"), (dict(file=vp(0x50008)), b"16-byte"),
           (dict(wsn=ws - 1), b"workspace too small"), (dict(wsn=T.build_workspace_bytes(100, 10)), b"workspace too small"),
           # the handle array is block_cap + 3 pairs: its last pair reaches d_file
           (dict(handles=vp(0x50000 - 16 * 13 + 8)), b"d_file overlaps d_handles")]
    for kw, msg in bad:
        assert call(**kw) == -1, kw
        assert msg in L.lv_last_error(), (kw, L.lv_last_error())
    assert call(handles=vp(0x50000 - 16 * 13)) != -1 or b"overlaps" not in L.lv_last_error()

    def opn(**kw):
        a = dict(dict(file=vp(0x50000), fcap=4096, table=vp(0x70000), bloom=vp(0x80000), flags=0), **kw)
        return L.lv_sst_bloom_open_device(a["file"], a["fcap"], a["table"], a["bloom"], a["flags"], None)
    for kw, msg in [(dict(flags=1), b"flag"), (dict(table=None), b"d_table"), (dict(table=vp(0x70004)), b"8-byte"),
                    (dict(bloom=None), b"d_bloom"), (dict(bloom=vp(0x80004)), b"8-byte"), (dict(file=None), b"d_file")]:
        assert opn(**kw) == -1, kw
        assert msg in L.lv_last_error(), (kw, L.lv_last_error())

    def get(**kw):
        a = dict(dict(file=vp(0x50000), fcap=4096, table=vp(0x70000), bloom=vp(0x80000), qk=vp(0x90000), qn=64,
                      off=vp(0xa0000), ln=vp(0xb0000), seq=vp(0xc0000), nq=4, res=vp(0xd0000), flags=0), **kw)
        return L.lv_sst_get_bloom_device(a["file"], a["fcap"], a["table"], a["bloom"], a["qk"], a["qn"], a["off"],
                                         a["ln"], a["seq"], a["nq"], a["res"], a["flags"], None)
    for kw, msg in [(dict(flags=1), b"flag"), (dict(table=None), b"d_table"), (dict(bloom=None), b"null d_bloom"),
                    (dict(bloom=vp(0x80004)), b"d_bloom must be 8-byte"), (dict(res=None), b"d_results"),
                    (dict(off=None), b"query array"), (dict(res=vp(0x50010)), b"d_results overlaps d_file")]:
        assert get(**kw) == -1, kw
        assert msg in L.lv_last_error(), (kw, L.lv_last_error())
    if not torch.cuda.is_available():  # no host fallback: the runtime's error, loudly
        assert call() != 0 and L.lv_last_error()
        assert opn() != 0 and get() != 0


def test_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "lvgpu", "table.h")).read()
    define = lambda name: int(re.search(r"#define %s\s+\(?(\d+)" % name, hdr).group(1))
    assert T.FILTER_BASE_LG == define("LV_SST_FILTER_BASE_LG") == B.BASE_LG
    assert re.search(r'#define LV_SST_BLOOM_NAME "([^"]+)"', hdr).group(1).encode() == T.BLOOM_NAME
    assert T.GET_FILTERED == define("LV_SST_GET_FILTERED") == B.FILTERED
    for v, name in T.BLOOM_WHY.items():
        if v:
            assert v == define("LV_SST_BLOOM_" + name)
    assert ctypes.sizeof(T.SstBloom) == 64 and ctypes.sizeof(T.BloomTotals) == 32 and ctypes.sizeof(T.BloomOptions) == 8
    src = open(os.path.join(ROOT, "leveldb-rs_amd", "csrc", "sst_build.hip")).read()
    assert T.SB_BLOOM_LDS == int(re.search(r"kSbBloomLds = (\d+)", src).group(1))
