"""lv_compact_filter_host against the Python model (tests/compact_cases.py),
field for field: snapshot thresholds, exact duplicates, deletions with and
without the base-level flag, unparsed type bytes, key lengths and alignments,
ranges, every status and every LV_ERR_INVALID rule of both entry points (the
device call checks its arguments before it touches a GPU).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import compact_cases as C
import lvgpu
import lvgpu.compact as CP
from compact_cases import BASE_LEVEL, MAX_SEQUENCE
from conftest import ROOT

CASES = C.cases()


def _seqs(payload, ops, kept, key):
    return [(int(ops[i]["tag"]) >> 8, int(ops[i]["tag"]) & 0xFF) for i in kept if C.make_key(payload, ops[i]) == key]


@pytest.mark.parametrize("name", list(CASES))
def test_cases_against_the_model(name):
    items, gaps, settings = CASES[name]
    payload, ops, order, mt = C.table_of(items, gaps)
    for S, flags, ranges in settings:
        want = C.check_host(payload, ops, order, mt, S, ranges, flags, tag_=(name, S, flags))
        assert want[0]["status"] == 0
        assert want[0]["kept"] + want[0]["dropped_hidden"] + want[0]["dropped_deletions"] == len(ops)


def test_snapshot_thresholds_explicitly():
    """One key at sequences 6..1: the newest is always kept, and below it
    exactly the versions at or above S (the version at S is the one every
    snapshot sees; it hides the next)."""
    items, gaps, _ = CASES["thresholds"]
    payload, ops, order, mt = C.table_of(items, gaps)
    for S in C.THRESHOLD_S:
        got = CP.filter_host(payload, ops, order, mt, S)
        kept = [s for s, _ in _seqs(payload, ops, got.order().tolist(), b"k")]
        assert kept == [s for s in range(6, 0, -1) if s == 6 or s >= S], (S, kept)
        assert got.totals["user_keys"] == 3 and got.mt_totals["user_keys"] == 3
    for S, want in ((3, [6, 5, 4, 3]), (2, [6, 5, 4, 3, 2]), (4, [6, 5, 4])):  # seq == S, S + 1, S - 1 around 3
        got = CP.filter_host(payload, ops, order, mt, S)
        assert [s for s, _ in _seqs(payload, ops, got.order().tolist(), b"k")] == want


def test_exact_duplicates_both_sides_of_the_snapshot():
    items, gaps, _ = CASES["duplicates"]
    payload, ops, order, mt = C.table_of(items, gaps)
    kept = lambda S, f=0: _seqs(payload, ops, CP.filter_host(payload, ops, order, mt, S, None, f).order().tolist(), b"d")
    assert kept(4) == [(9, 1), (9, 1), (5, 1), (5, 1), (5, 1), (5, 0), (5, 0)]  # nothing at or below 4
    assert kept(5) == [(9, 1), (9, 1), (5, 1)]      # the first of the duplicates at 5 hides the rest
    assert kept(8) == [(9, 1), (9, 1), (5, 1)]
    assert kept(9) == [(9, 1)]                      # the duplicate at 9 is hidden by its twin
    assert kept(10) == [(9, 1)]


def test_deletions_explicitly():
    items, gaps, _ = CASES["deletions"]
    payload, ops, order, mt = C.table_of(items, gaps)

    def kept(S, flags):
        got = CP.filter_host(payload, ops, order, mt, S, None, flags)
        return {k: _seqs(payload, ops, got.order().tolist(), k) for k in
                (b"first", b"shadowed", b"shadowing", b"at_s", b"above_s")}, got.totals
    k, t = kept(5, 0)  # without the flag a deletion is dropped only as hidden
    assert k == {b"first": [(5, 0)], b"shadowed": [(7, 1), (5, 0)], b"shadowing": [(6, 0), (4, 1)],
                 b"at_s": [(5, 0)], b"above_s": [(6, 0)]}
    assert t["dropped_deletions"] == 0 and t["dropped_hidden"] == 2
    k, t = kept(5, BASE_LEVEL)  # seq == S goes, S + 1 stays; what a dropped deletion hid stays hidden
    assert k == {b"first": [], b"shadowed": [(7, 1)], b"shadowing": [(6, 0), (4, 1)], b"at_s": [], b"above_s": [(6, 0)]}
    assert t["dropped_deletions"] == 3 and t["dropped_hidden"] == 2 and t["user_keys"] == 3
    k, t = kept(6, BASE_LEVEL)
    assert k[b"above_s"] == [] and k[b"shadowing"] == [] and k[b"shadowed"] == [(7, 1)]


def test_unparsed_type_bytes_are_kept_and_reset_the_state():
    items, gaps, _ = CASES["unparsed"]
    payload, ops, order, mt = C.table_of(items, gaps)
    got = CP.filter_host(payload, ops, order, mt, 9, None, BASE_LEVEL)
    kept = got.order().tolist()
    # u: 6 kept, 5 hidden, (4, type 2) kept, 3 the first of its key again, 2 hidden
    assert _seqs(payload, ops, kept, b"u") == [(6, 1), (4, 2), (3, 1)]
    # v: 9 kept, (8, 0xff) kept, the deletion at 7 is a first entry and base level: dropped; 6 hidden behind it
    assert _seqs(payload, ops, kept, b"v") == [(9, 1), (8, 0xFF)]
    assert _seqs(payload, ops, kept, b"w") == [(1, 2)]
    assert got.totals["unparsed"] == 3


def test_ranges_explicitly():
    items, gaps, _ = CASES["ranges"]
    payload, ops, order, mt = C.table_of(items, gaps)
    for name, ranges in C.range_lists().items():
        got = CP.filter_host(payload, ops, order, mt, 5, C.for_binding(ranges), BASE_LEVEL)
        kept = got.order().tolist()
        dels = {C.make_key(payload, ops[i]) for i in kept if int(ops[i]["tag"]) & 0xFF == 0}
        inside = {C.RANGE_LO, C.RANGE_HI, b"ccc"} if ranges else set()
        if name == "4096":
            inside |= {b"r0007", b"r0007~"}
        assert dels == inside, (name, dels)  # lo and hi are inside; bba, bb (a prefix of lo), ddd\0 and dde are not
        assert got.totals["dropped_deletions"] == 11 - len(inside)


@pytest.mark.parametrize("name", list(C.status_cases()))
def test_statuses(name):
    kw, status = C.status_cases()[name]
    kw = dict(kw)
    want = C.check_host(kw.pop("payload"), kw.pop("ops"), kw.pop("order"), kw.pop("mt"), kw.pop("S"), kw.pop("ranges"),
                        kw.pop("flags"), tag_=name, **kw)
    assert want[0]["status"] == status and (status == 0 or want[1] == C.NO_TABLE)


def test_op_cap_above_the_entries_and_the_empty_table():
    items, gaps, _ = CASES["deletions"]
    payload, ops, order, mt = C.table_of(items, gaps)
    pad = np.zeros(5, dtype=ops.dtype)
    C.check_host(payload, np.concatenate([ops, pad]), order, mt, 5, None, BASE_LEVEL, op_cap=len(ops) + 5)
    empty = C.table_of([])
    for cap in (0, 3):
        want = C.check_host(empty[0], np.zeros(cap, dtype=ops.dtype), empty[2], empty[3], 5, None, BASE_LEVEL, op_cap=cap)
        assert want[0] == dict.fromkeys(C.TOTALS, 0) and want[1] == dict(entries=0, user_keys=0, status=0)


def test_an_unsorted_order_yields_what_the_loop_yields():
    items, gaps, _ = CASES["key_lengths"]
    payload, ops, order, mt = C.table_of(items, gaps)
    rng = np.random.default_rng(5)
    for _ in range(5):
        C.check_host(payload, ops, rng.permutation(order), mt, 5, None, BASE_LEVEL)
    C.check_host(payload, ops, np.zeros(len(ops), dtype=np.uint32), mt, 5)  # one op, many times


def _host_rc(S=5, flags=0, n_ranges=0, op_cap=1, null=None):
    L = CP._bind()
    mt, mto, tot = CP.MtTotals(0, 0, 0), CP.MtTotals(), CP.CompactTotals()
    buf = ctypes.create_string_buffer(64)
    p = {k: buf for k in ("payload", "ops", "order", "ranges", "range_keys", "order_out")}
    p.update(mt=ctypes.byref(mt), mto=ctypes.byref(mto), tot=ctypes.byref(tot))
    if null:
        p[null] = None
    return L.lv_compact_filter_host(p["payload"], 1, p["ops"], p["order"], p["mt"], op_cap, S, p["ranges"], n_ranges,
                                    p["range_keys"], 1, p["order_out"], p["mto"], p["tot"], flags)


def test_host_invalid_arguments():
    assert _host_rc() == 0
    assert _host_rc(S=MAX_SEQUENCE) == -1 and _host_rc(S=MAX_SEQUENCE - 1) == 0 and _host_rc(S=2 ** 64 - 1) == -1
    assert _host_rc(flags=2) == -1 and _host_rc(flags=BASE_LEVEL) == 0
    assert _host_rc(n_ranges=1) == -1  # ranges without the flag
    assert _host_rc(n_ranges=4097, flags=BASE_LEVEL) == -1
    assert _host_rc(op_cap=2 ** 32 - 1) == -1
    for null in ("payload", "ops", "order", "order_out", "range_keys", "mt", "mto", "tot"):
        assert _host_rc(null=null) == -1, null
    assert _host_rc(null="ranges", n_ranges=1, flags=BASE_LEVEL) == -1


def _dev_rc(**kw):
    """lv_compact_filter_device with fake pointers: every call here fails its
    checks before anything is dereferenced."""
    L = CP._bind()
    vp = ctypes.c_void_p
    a = dict(payload=0x10000, payload_bytes=64, ops=0x20000, order=0x30000, mt=0x40000, op_cap=8, S=5, ranges=0x50000,
             n_ranges=0, range_keys=0x60000, range_keys_bytes=8, order_out=0x70000, mto=0x80000, tot=0x90000, flags=0,
             ws=0xA0000, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = CP.filter_workspace_bytes(a["op_cap"])
    ptr = lambda v: vp(v) if v else None
    rc = L.lv_compact_filter_device(ptr(a["payload"]), a["payload_bytes"], ptr(a["ops"]), ptr(a["order"]), ptr(a["mt"]),
                                    a["op_cap"], a["S"], ptr(a["ranges"]), a["n_ranges"], ptr(a["range_keys"]),
                                    a["range_keys_bytes"], ptr(a["order_out"]), ptr(a["mto"]), ptr(a["tot"]), a["flags"],
                                    ptr(a["ws"]), a["ws_bytes"], None)
    return rc, lvgpu.lib().lv_last_error()


def test_device_invalid_arguments():
    bad = {
        b"flag": dict(flags=2), b"smallest_snapshot": dict(S=MAX_SEQUENCE), b"n_ranges": dict(n_ranges=4097, flags=1),
        b"LV_COMPACT_BASE_LEVEL": dict(n_ranges=1), b"d_mt_totals": dict(mt=0), b"d_mt_totals_out": dict(mto=0),
        b"d_totals": dict(tot=0), b"8-byte": dict(tot=0x90004), b"d_payload": dict(payload=0), b"2^32": dict(op_cap=2 ** 32 - 1),
        b"d_ops": dict(ops=0), b"16-byte": dict(ops=0x20008), b"d_order": dict(order_out=0), b"4-byte": dict(order=0x30002),
        b"d_ranges": dict(ranges=0, n_ranges=1, flags=1), b"d_range_keys": dict(range_keys=0), b"null workspace": dict(ws=0),
        b"workspace must": dict(ws=0xA0008), b"too small": dict(ws_bytes=CP.filter_workspace_bytes(8) - 1),
        b"overlaps d_order": dict(order_out=0x30000 + 28), b"overlaps d_ops": dict(order_out=0x20000 + 252),
        b"overlaps d_payload": dict(order_out=0x10000 + 60),
    }
    for word, kw in bad.items():
        rc, err = _dev_rc(**kw)
        assert rc == -1 and word in err, (word, rc, err)
    for kw in (dict(mt=0x40004), dict(mto=0x80004), dict(ranges=0x50004, n_ranges=1, flags=1), dict(order_out=0x70002)):
        assert _dev_rc(**kw)[0] == -1, kw
    # adjacent is not overlapping; what follows a well-formed call is the runtime's answer, not LV_ERR_INVALID
    import torch
    if not torch.cuda.is_available():
        assert _dev_rc(order_out=0x30000 + 32)[0] not in (0, -1)  # no host fallback


def test_workspace_bytes():
    assert CP.filter_workspace_bytes(2 ** 32 - 1) == 0
    small, big = CP.filter_workspace_bytes(0), CP.filter_workspace_bytes(1 << 20)
    assert small > 0 and big - small == (1 << 20) * 4 + ((1 << 20) // CP.CF_TILE) * 8


def test_tile_constant_matches_the_knob():
    text = open(os.path.join(ROOT, "leveldb-rs_amd", "csrc", "lvk", "knobs.h")).read()
    assert int(re.search(r"#define LVK_CF_TILE (\d+)", text).group(1)) == CP.CF_TILE


def test_stress_trials_are_not_hollow():
    """The stress trials hold tables of more than two tiles, both kinds of
    drop, unparsed entries, ranges that hold keys and every flag."""
    import test_gpu_compact_stress as TS
    big = hidden = dels = unparsed = ranged = 0
    for seed in range(C.STRESS_TRIALS):
        payload, ops, order, mt, S, ranges, flags = C.stress_trial(seed)
        want = C.model_filter(payload, ops, order, mt, S, ranges, flags)[0]
        assert want["status"] == 0
        big += len(ops) > 2 * CP.CF_TILE
        hidden += want["dropped_hidden"] > 0
        dels += want["dropped_deletions"] > 0
        unparsed += want["unparsed"] > 0
        if ranges:
            free = C.model_filter(payload, ops, order, mt, S, None, flags)[0]
            ranged += free["dropped_deletions"] > want["dropped_deletions"]
    assert big >= 10 and hidden >= 33 and dels >= 25 and unparsed >= 5 and ranged >= 10, (big, hidden, dels, unparsed, ranged)
    assert TS.CHUNK * len(range(0, C.STRESS_TRIALS, TS.CHUNK)) == C.STRESS_TRIALS
