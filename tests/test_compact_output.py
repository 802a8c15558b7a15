"""lv_compact_output_host against the serial model (tests/compact_output_cases.py)
and against the twins that define it: the slice rule (lv_sst_build_host /
lv_sst_build_bloom_host over the order slice), the records (lv_sst_open_host,
lv_sst_bloom_open_host, lv_version_file_host), the run as a level of a version
(lv_version_open_host, lv_version_get_host against lv_memtable_get_host), the
arena bound, the statuses, the golden example and every argument refusal of
the host and device calls.  No GPU."""
import ctypes
import json

import numpy as np
import pytest

import compact_output_cases as CO
import lvgpu.compact as C
import lvgpu.memtable as MT
import lvgpu.table as T
import lvgpu.version as LV
import memtable_cases as M
import sst_bloom_cases as B
import sst_build_cases as S
from memtable_cases import MAX_SEQUENCE, make_table, tag

CASES = CO.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_matches_the_model(name):
    items, bs, ri, bpk, mf = CASES[name]
    payload, ops = make_table(items)
    w = CO.model_output(payload, ops, mf, bpk, bs, ri, bound_used=3, first_number=9, level=4, images_off=4096)
    out = CO.host_output(payload, ops, mf, bpk, bs, ri, bound_used=3, first_number=9, level=4, images_off=4096)
    CO.compare_host(out, w, name)
    sized = CO.host_output(payload, ops, mf, bpk, bs, ri, sizing=True)
    assert sized.totals == w.totals


def test_the_cases_have_the_shapes_they_claim():
    def model(name):
        items, bs, ri, bpk, mf = CASES[name]
        payload, ops = make_table(items)
        return CO.model_output(payload, ops, mf, bpk, bs, ri), mf
    assert model("one_file_10")[0].totals["files"] == 1
    assert model("small_files_10")[0].totals["files"] >= 8
    blocks = [model(f"cut_{d:+d}")[0].files[0]["data_blocks"] for d in (-1, 0, 1)]
    assert blocks == [2, 2, 3]
    w, mf = model("end_on_flush")
    assert w.last_by_cut and len(w.files) >= 2 and w.flushed(len(w.files) - 1) >= mf
    w, mf = model("end_open")
    assert not w.last_by_cut and w.flushed(len(w.files) - 1) < mf
    w, _ = model("filter_windows")
    assert len(w.files) >= 3 and all(b["num"] >= 3 for b in w.blooms[:-1])
    w, _ = model("duplicates")
    assert w.totals["files"] == w.totals["entries"]


def test_golden_example():
    """The header's worked example: file 0 is table.h's one-entry table, file
    1 lies at 128, and the first index key is the successor, not the
    separator the one-file build writes."""
    g = CO.load_golden()
    assert g == json.loads(json.dumps(CO.golden_dict()))
    items = [(k.encode(), tag(s), v.encode()) for k, s, v in g["entries"]]
    payload, ops = make_table(items)
    out = CO.host_output(payload, ops, g["max_file_bytes"], None, g["block_size"], g["restart_interval"])
    assert [out.image(k).hex() for k in range(2)] == g["images"]
    assert [int(f["file_off"]) for f in out.files[:2]] == [0, 128] and out.totals["arena_bytes"] == 242
    one = S.model_build(*make_table(items[:1]), g["block_size"], g["restart_interval"])[0]
    assert out.image(0) == one and len(one) == 114
    whole = S.model_build(payload, ops, g["block_size"], g["restart_interval"])[0]
    assert b"l" + S.MAXTAG in whole and b"l" + S.MAXTAG not in out.image(0) + out.image(1)
    assert S.ikey(b"k", tag(1)) in out.image(0)[39:61]


def _random_cases(trials):
    rng = np.random.default_rng(77)
    for t, (items, bs, ri) in enumerate(S.adversarial_tables(rng, trials)):
        payload, ops = make_table(items)
        sizes = [sz + 5 for _, sz in S.model_build(payload, ops, bs, ri)[1][:-2]]
        mf = [1, max(sizes[0] - 1, 1), sizes[0] + 1, sum(sizes[:3]), 1 << 63][t % 5]
        yield t, payload, ops, bs, ri, (10 if t % 3 else None), mf


def test_random_tables():
    """Adversarial tables with max_file_bytes of 1, a block's size - 1 and + 1,
    three blocks and 2^63: the model, the slice rule, the records, and the run
    as a level that answers every key as the memtable does."""
    files = 0
    for t, payload, ops, bs, ri, bpk, mf in _random_cases(120):
        w = CO.model_output(payload, ops, mf, bpk, bs, ri)
        out = CO.host_output(payload, ops, mf, bpk, bs, ri)
        CO.compare_host(out, w, f"trial {t}")
        order, mt = M.model_totals(payload, ops)
        nf = w.totals["files"]
        files += nf
        bounds = np.full(out.bounds.size, 0xA5, dtype=np.uint8)
        used = 0
        for k in range(nf):
            f = out.files[k]
            sl = order[int(f["first_entry"]): int(f["first_entry"] + f["entries"])]
            smt = dict(entries=len(sl), user_keys=0, status=0)
            if bpk:
                img, hs, _, bt = T.build_bloom_host(payload, ops, sl, smt, bpk, bs, ri)
                assert bt["filter_keys"] == int(f["filter_keys"])
            else:
                img, hs, _ = T.build_host(payload, ops, sl, smt, bs, ri)
            assert img == out.image(k) and list(hs) == out.file_handles(k, w.extra), (t, k)
            table = T.open_host(img, handles=False)[0]
            assert [int(table[n]) for n in T.TABLE_FIELDS] == [int(x) for x in out.tables[k]], (t, k)
            bl = T.bloom_open_host(img, table)
            assert [int(bl[n]) for n in B.BLOOM_FIELDS] == [int(x) for x in out.blooms[k]], (t, k)
            vf, used = LV.file_host(out.arena[:out.arena_cap], int(f["file_off"]), int(f["file_bytes"]), table, 1 + k, 1,
                                    bounds, used, bound_cap=out.bound_cap)
            assert vf == {n: int(out.version_files[k][n]) for n in LV.FILE_DTYPE.names}, (t, k)
        assert bounds.tobytes() == out.bounds.tobytes() and used == out.bound_used
        hv = LV.HostVersion(out.arena[:out.arena_cap], out.version_files[:nf], out.tables[:nf], out.blooms[:nf],
                            out.bounds[:out.bound_cap])
        state = hv.open()
        ents = S.entries_of(payload, ops)
        strictly = all(ents[i][0] != ents[i + 1][0] for i in range(len(ents) - 1))
        assert state["status"] == (0 if strictly else state["status"]) and state["status"] in (0, 16), (t, state)
        if state["status"]:
            continue
        for key in {M.key_of(payload, o) for o in ops}:
            for seq in (MAX_SEQUENCE, 2, 0):
                a = MT.get_host(payload, ops, order, mt, key, seq)
                b = hv.get(key, seq)
                assert a["status"] == b["status"], (t, key, seq, a, b)
                if a["status"] == 1:
                    assert payload[a["val_off"]:a["val_off"] + a["val_len"]] == \
                        out.arena[b["val_off"]:b["val_off"] + b["val_len"]].tobytes(), (t, key, seq)
    assert files > 600


@pytest.mark.parametrize("bpk", [None, 10])
def test_arena_bound_holds_at_one_file_per_block(bpk):
    """max_file_bytes = 1 closes a file behind every block: the worst case."""
    rng = np.random.default_rng(3)
    tight = 0.0
    for items, bs, ri in S.adversarial_tables(rng, 120):
        payload, ops = make_table(items)
        t = CO.host_output(payload, ops, 1, bpk, bs, ri, sizing=True).totals
        bound = C.output_arena_bound(len(payload), len(ops), bpk)
        assert t["arena_bytes"] <= bound, (t, bound)
        tight = max(tight, t["arena_bytes"] / bound)
    assert tight > 0.3
    assert C.output_arena_bound(100, 0, bpk) == 0 and C.output_arena_bound(1 << 63, 1 << 31, bpk) == (1 << 64) - 1
    assert C.output_arena_bound(100, 10, 65) == 0 and C.output_arena_bound(100, 10, 0) == 0
    assert C.output_arena_bound(100, 10, bpk) >= (T.bloom_file_bound(100, 10, bpk) if bpk else T.file_bound(100, 10))


def test_statuses_report_the_true_totals_and_write_nothing():
    items, bs, ri, bpk, mf = CASES["small_files_10"]
    payload, ops = make_table(items)
    t = CO.model_output(payload, ops, mf, bpk, bs, ri).totals
    full = dict(arena_cap=t["arena_bytes"], block_cap=t["data_blocks"], files_cap=t["files"], bound_cap=3 + t["bound_bytes"])
    bits = dict(arena_cap=CO.ARENA_OVER, block_cap=CO.HANDLE_OVER, files_cap=CO.FILES_OVER, bound_cap=CO.BOUND_OVER)
    for cap, bit in bits.items():
        out = CO.host_output(payload, ops, mf, bpk, bs, ri, bound_used=3, **dict(full, **{cap: full[cap] - 1}))
        assert out.totals == dict(t, status=bit), (cap, out.totals)
        CO.untouched_host(out, 3)
    out = CO.host_output(payload, ops, mf, bpk, bs, ri, bound_used=3, arena_cap=1, block_cap=0, files_cap=0, bound_cap=0)
    assert out.totals == dict(t, status=CO.ARENA_OVER | CO.HANDLE_OVER | CO.FILES_OVER | CO.BOUND_OVER)
    CO.untouched_host(out, 3)
    none = dict.fromkeys(CO.TOTALS, 0) | dict(status=CO.NO_TABLE)
    order, mt = M.model_totals(payload, ops)
    kw = dict(bits_per_key=bpk, block_size=bs, restart_interval=ri, **full)
    assert C.output_host(payload, ops, order, dict(mt, status=1), mf, **kw).totals == none
    assert C.output_host(payload, ops, order, dict(mt, entries=len(ops) + 1), mf, **kw).totals == none
    for field, val in (("key_off", len(payload) + 1), ("val_len", 0xFFFFFFFF), ("val_off", (1 << 64) - 1)):
        bad = ops.copy()
        bad[7][field] = val
        out = C.output_host(payload, bad, order, mt, mf, **kw)
        assert out.totals == none, field
        CO.untouched_host(out)
    out = C.output_host(payload, ops, [len(ops)] + list(order[1:]), mt, mf, **kw)
    assert out.totals == none
    # no version files: no bound keys, and the cursor stays
    out = CO.host_output(payload, ops, mf, bpk, bs, ri, version_files=False, blooms=False, bound_used=3)
    assert out.totals == dict(t, bound_bytes=0) and out.bound_used == 3 and (out.bounds == 0xA5).all()
    assert (out.blooms == 0xA5A5A5A5A5A5A5A5).all() and set(out.version_files.tobytes()) == {0xA5}


@pytest.mark.parametrize("bpk", [None, 10])
def test_block_large(bpk):
    """A value extent of 2^32 - 1 bytes claimed inside a payload that is not
    allocated: the status comes from sizes alone, in u64, with the true totals
    and nothing written.  The large block also closes its file, so a second
    file follows; alone through the sizing pass, with ARENA_OVER through a call
    with an arena; raw = 2^32 - 2 is not large, 2^32 - 1 is."""
    payload, ops, order, mt, claimed, bs, ri, mf = CO.block_large_case()
    kw = dict(bits_per_key=bpk, block_size=bs, restart_interval=ri, payload_bytes=claimed)
    t = C.output_host(payload, ops, order, mt, mf, sizing=True, **kw).totals
    assert t["status"] == CO.BLOCK_LARGE and (t["entries"], t["files"], t["data_blocks"]) == (3, 2, 2)
    assert t["handle_pairs"] == 2 + 2 * (3 if bpk else 2) and t["bound_bytes"] == 4 * 9
    # the slice rule for the sizes: file 0 is {a, b}, file 1 is {c}
    sizes = [T.build_host(payload, ops, sl, dict(entries=len(sl), user_keys=0, status=0), bs, ri, sizing=True,
                          payload_bytes=claimed)[2] for sl in ([0, 1], [2])]
    assert sizes[0]["status"] == CO.BLOCK_LARGE == S.BLOCK_LARGE and sizes[1]["status"] == 0
    plain = CO.align16(sizes[0]["file_bytes"]) + sizes[1]["file_bytes"]
    if bpk is None:
        assert t["arena_bytes"] == plain > (1 << 32)
    else:  # 2^21 windows of 4 bytes in file 0's filter block, and a filter per file
        assert plain + 4 * (1 << 21) < t["arena_bytes"] < plain + 4 * (1 << 21) + 200
    # with an arena: the capacities are judged too, the totals stay, nothing is written
    caps = dict(arena_cap=64, block_cap=2, files_cap=2, bound_cap=3 + 36)
    out = C.output_host(payload, ops, order, mt, mf, bound_used=3, **kw, **caps)
    assert out.totals == dict(t, status=CO.BLOCK_LARGE | CO.ARENA_OVER)
    CO.untouched_host(out, 3)
    out = C.output_host(payload, ops, order, mt, mf, bound_used=3, **kw, **dict(caps, files_cap=1, bound_cap=3 + 35))
    assert out.totals == dict(t, status=CO.BLOCK_LARGE | CO.ARENA_OVER | CO.FILES_OVER | CO.BOUND_OVER)
    CO.untouched_host(out, 3)
    # a small value instead: one block, one file; the large block moved the cut
    small = CO.block_large_case(vlen=1)
    t1 = C.output_host(small[0], small[1], order, mt, mf, sizing=True, **kw).totals
    assert (t1["status"], t1["files"], t1["data_blocks"]) == (0, 1, 1)
    # the boundary: entry b alone, 1 + 1 + 5 bytes of varints, 9 of key, the value, 4 + 4 of restarts
    one, omt = np.array([1], dtype=np.uint32), dict(entries=1, user_keys=1, status=0)
    for raw, status in ((CO.BIG - 1, 0), (CO.BIG, CO.BLOCK_LARGE)):
        edge = CO.block_large_case(vlen=raw - (1 + 1 + 5 + 9) - 8)
        t2 = C.output_host(edge[0], edge[1], one, omt, mf, sizing=True, **kw).totals
        assert t2["status"] == status and (t2["files"], t2["data_blocks"]) == (1, 1), (raw, t2)
        assert t2["arena_bytes"] > raw + 5


def test_empty_memtable():
    out = CO.host_output(b"", np.zeros(0, dtype=M.op_dtype()), 100, 10, arena_cap=64, block_cap=4, files_cap=4, bound_cap=8)
    assert out.totals == dict.fromkeys(CO.TOTALS, 0)
    CO.untouched_host(out)


def test_host_argument_checks():
    items, bs, ri, bpk, mf = CASES["example"]
    payload, ops = make_table(items)
    order, mt = M.model_totals(payload, ops)
    for kw in (dict(max_file_bytes=0), dict(level=0), dict(level=7), dict(files_cap=(1 << 20) + 1),
               dict(first_number=(1 << 64) - 1), dict(block_size=0), dict(restart_interval=1025), dict(bits_per_key=0),
               dict(bits_per_key=65), dict(bits_per_key=10, bloom_reserved=1), dict(op_cap=(1 << 32) - 1)):
        a = dict(dict(max_file_bytes=1, arena_cap=512, block_cap=4, files_cap=4, bound_cap=64), **kw)
        with pytest.raises(C.LvError):
            C.output_host(payload, ops, order, mt, a.pop("max_file_bytes"), **a)


def test_device_argument_checks_before_any_device_call():
    L = C._bind_output()
    vp = ctypes.c_void_p
    ws = C.output_workspace_bytes(100, 10, 4)
    assert ws > T.build_bloom_workspace_bytes(100, 10)
    assert C.output_workspace_bytes(1 << 32, 1, 1) == 0 and C.output_workspace_bytes(1, 1, (1 << 20) + 1) == 0
    bo = ctypes.byref(T.BloomOptions(10, 0))
    good = dict(payload=vp(0x10000), pn=4096, ops=vp(0x20000), order=vp(0x30000), mt=vp(0x40000), cap=100, opt=None,
                bloom=bo, mf=1000, number=1, level=1, ioff=0, arena=vp(0x50000), acap=4096, handles=vp(0x60000), bcap=10,
                files=vp(0x70000), tables=vp(0x71000), blooms=vp(0x72000), vfiles=vp(0x73000), fcap=4, keys=vp(0x80000),
                kcap=256, used=vp(0x81000), tot=vp(0x82000), flags=0, ws=vp(0x100000), wsn=ws)
    names = list(good)

    def call(**kw):
        a = dict(good, **kw)
        return L.lv_compact_output_device(*[a[n] for n in names], None)

    def opt(bs, ri):
        return ctypes.byref(T.BuildOptions(bs, ri))
    bad = [(dict(flags=1), b"flag"), (dict(opt=opt(0, 16)), b"block_size"), (dict(opt=opt(64, 0)), b"restart_interval"),
           (dict(bloom=ctypes.byref(T.BloomOptions(0, 0))), b"bits_per_key"),
           (dict(bloom=ctypes.byref(T.BloomOptions(10, 1))), b"reserved"), (dict(mf=0), b"max_file_bytes"),
           (dict(level=0), b"level"), (dict(level=7), b"level"), (dict(fcap=(1 << 20) + 1), b"LV_VERSION_MAX_FILES"),
           (dict(number=(1 << 64) - 2), b"wraps"), (dict(tot=None), b"d_totals"), (dict(tot=vp(0x82004)), b"8-byte"),
           (dict(mt=None), b"d_mt_totals"), (dict(payload=None), b"d_payload"), (dict(cap=(1 << 32) - 1), b"op_cap"),
           (dict(bcap=(1 << 32) - 3), b"block_cap"), (dict(ops=None), b"d_ops"), (dict(ops=vp(0x20008)), b"16-byte"),
           (dict(order=None), b"d_order"), (dict(order=vp(0x30002)), b"4-byte"), (dict(arena=None), b"d_arena"),
           (dict(arena=vp(0x50008)), b"16-byte"), (dict(handles=None), b"d_handles"),
           (dict(handles=vp(0x60004)), b"8-byte"), (dict(files=None), b"d_files"), (dict(tables=None), b"d_tables"),
           (dict(vfiles=vp(0x73004)), b"8-byte"), (dict(used=None), b"d_bound_used"), (dict(keys=None), b"d_bound_keys"),
           (dict(used=vp(0x81004)), b"8-byte"), (dict(ws=None), b"null workspace"), (dict(ws=vp(0x100008)), b"16-byte"),
           (dict(wsn=ws - 1), b"workspace too small"),
           # the handle array is block_cap + 3 files_cap pairs: its last pair reaches the arena
           (dict(handles=vp(0x50000 - 16 * 22 + 8)), b"d_arena overlaps d_handles"),
           (dict(arena=vp(0x10800)), b"d_arena overlaps d_payload"), (dict(files=vp(0x20000 + 32 * 99)), b"d_files overlaps d_ops"),
           (dict(tables=vp(0x70000 + 64 * 3)), b"d_files overlaps d_tables"),
           (dict(keys=vp(0x30000 + 4 * 99)), b"d_bound_keys overlaps d_order"),
           (dict(tot=vp(0x73000 + 64 * 3)), b"d_version_files overlaps d_totals"),
           (dict(used=vp(0x40000)), b"d_bound_used overlaps d_mt_totals")]
    for kw, msg in bad:
        assert call(**kw) == -1, kw
        assert msg in L.lv_last_error(), (kw, L.lv_last_error())
    # optional outputs may be NULL, and a neighbour that only touches is no overlap: what follows a well-formed
    # call is the runtime's answer, not LV_ERR_INVALID (no host fallback).  Only without a GPU: with one the
    # call would run over these made-up addresses.
    import torch
    if not torch.cuda.is_available():
        for kw in ({}, dict(blooms=None), dict(vfiles=None, keys=None, used=None), dict(bloom=None),
                   dict(handles=vp(0x50000 - 16 * 22))):
            assert call(**kw) == -2, (kw, L.lv_last_error())  # LV_ERR_NO_DEVICE
            assert b"hipGetDevice" in L.lv_last_error(), (kw, L.lv_last_error())
