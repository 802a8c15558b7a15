"""lv_sst_scan_host (include/lvgpu/table.h, "Scan") against the Python model of
sst_scan_cases.py, the model against sst_build_cases.read_table, the scan
against the build (scan -> build reproduces the image) and against the two
gets; every status, appending, the block rules, damaged and foreign tables,
the argument checks of lv_sst_scan_device.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lvgpu
import lvgpu.memtable as MT
import lvgpu.table as T
import memtable_cases as M
import sst_build_cases as S
import sst_get_cases as G
import sst_scan_cases as C
from memtable_cases import make_table, tag

CASES = S.cases()
INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "leveldb-rs_amd", "csrc", "sst_scan.hip")
FILL = 0xA5


def scan_both(image, table, prev=None, *, prev_out=None, order=None, tag_="", **caps):
    """scan_host against model_scan, field for field and byte for byte, with
    the untouched parts of the arena and the ops checked: the host's result."""
    order = prev is None if order is None else order
    want_t, want_ops, want_arena, want_mt = C.model_scan(image, table, prev, order=order, **caps)
    kw = {k: v for k, v in caps.items() if k in ("arena_cap", "op_cap")}
    if prev_out is not None:
        kw.update(arena=prev_out[2], ops=prev_out[1])
        kw.setdefault("arena_cap", want_t["arena_bytes"] if not want_t["status"] else len(prev_out[2]))
        kw.setdefault("op_cap", want_t["entries"] if not want_t["status"] else len(prev_out[1]))
    if want_t["status"] & (C.OP_OVER | C.ARENA_OVER) == 0 and want_t["status"]:
        kw.setdefault("arena_cap", 64)  # a status: room that must stay untouched
        kw.setdefault("op_cap", 4)
    got_t, ops, arena, mt = T.scan_host(image, table, prev, order=order, fill=FILL, **kw)
    assert got_t == want_t, (tag_, got_t, want_t)
    base_e, base_b = (prev["entries"], prev["arena_bytes"]) if prev else (0, 0)
    if want_t["status"]:
        base_e = base_b = 0 if prev_out is None else None
    if base_e is not None:
        n = len(want_ops)
        assert (ops[base_e:base_e + n] == C.ops_array(want_ops)).all(), (tag_, "ops differ")
        assert arena[base_b:base_b + len(want_arena)].tobytes() == want_arena, (tag_, "arena differs")
        assert (arena[base_b + len(want_arena):] == FILL).all(), (tag_, "arena written beyond the entries")
        assert (ops[base_e + n:].view(np.uint8) == FILL).all(), (tag_, "ops written beyond the entries")
    else:  # appended and refused: what the earlier scans left is unchanged
        assert arena.tobytes()[: len(prev_out[2])] == prev_out[2].tobytes()[: len(arena)], (tag_, "arena changed on a status")
        assert (ops[: len(prev_out[1])] == prev_out[1][: len(ops)]).all(), (tag_, "ops changed on a status")
    if order:
        o = mt.pop("order")
        assert mt == want_mt, (tag_, mt, want_mt)
        n = 0 if want_t["status"] else want_t["table_entries"]
        assert (o[:n] == np.arange(n)).all() and (o[n:] == 0xA5A5A5A5).all(), (tag_, "order")
        mt["order"] = o
    return got_t, ops, arena, mt


def built(name, bs=None, ri=None):
    items, cbs, cri = CASES[name]
    bs, ri = cbs if bs is None else bs, cri if ri is None else ri
    payload, ops = make_table(items)
    image, _, _ = S.model_build(payload, ops, bs, ri)
    return payload, ops, image, bs, ri


# ---- exports and constants ----
def test_exports_and_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "lvgpu", "table.h")).read()
    define = lambda text, n: int(re.search(r"#define\s+%s\s+(\d+)u?\b" % n, text).group(1))
    for bit, name in T.SCAN_STATUS.items():
        assert define(src, "LV_SST_SCAN_" + name) == bit
    assert define(src, "LV_SST_SCAN_MT_UNORDERED") == T.SCAN_MT_UNORDERED == C.MT_UNORDERED
    assert T.SCAN_MT_UNORDERED not in MT.BUILD_STATUS
    assert (C.UPSTREAM, C.NO_TABLE, C.CORRUPT, C.BLOCK_OVER, C.OP_OVER, C.ARENA_OVER) == tuple(T.SCAN_STATUS)
    body = re.search(r"typedef struct lv_sst_scan_totals \{(.*?)\} lv_sst_scan_totals;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert tuple(re.findall(r"\b([a-z_]+)\s*[,;]", body)) == T.SCAN_TOTALS == C.TOTALS
    assert ctypes.sizeof(T.ScanTotals) == 64
    knobs = open(os.path.join(ROOT, "leveldb-rs_amd", "csrc", "lvk", "knobs.h")).read()
    assert T.SS_TILE == define(knobs, "LVK_SS_TILE") and T.SS_WAVE_COPY == define(knobs, "LVK_SS_WAVE_COPY")
    for n in ("lv_sst_scan_workspace_bytes", "lv_sst_scan_device", "lv_sst_scan_host"):
        assert n in lvgpu.declared_symbols() and hasattr(lvgpu.lib(), n)
    # the workspace holds op_cap + block_cap runs and block_cap blocks
    w = T.scan_workspace_bytes
    assert w(2000, 16) - w(1000, 16) == 1000 * 16 and w(0, 2016) - w(0, 1016) == 1000 * (24 + 16)
    assert w(1 << 32, 1) == 0 and w(1, 1 << 32) == 0 and w(0, 0) > 0


# ---- well-formed tables ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_model_and_reader(name):
    for bs in (None, 1):
        payload, ops, image, bs_, ri = built(name, bs)
        table = T.open_host(image)[0]
        assert table == C.open_table(image)
        got_t, gops, garena, mt = scan_both(image, table, tag_=(name, bs))
        # the model against the reader written for the build
        _, mops, marena, mmt = C.model_scan(image, table, order=True)
        want = S.read_table(image)[0] if image else []
        assert C.model_entries(mops, marena) == want == S.entries_of(payload, ops)
        assert got_t["table_entries"] == len(ops) and mt["status"] == 0
        assert got_t["table_bytes"] == int(ops["key_len"].sum()) + int(ops["val_len"].sum())
        assert mt["user_keys"] == M.model_totals(payload, ops)[1]["user_keys"]
        assert got_t["data_blocks"] == table["data_blocks"] and (got_t["runs"] >= got_t["data_blocks"])
        # scan -> build with the same options reproduces the image; with others the model's build of the source
        mtd = {k: mt[k] for k in ("entries", "user_keys", "status")}
        for obs, ori in ((bs_, ri), (97, 3)):
            file2, _, tot2 = T.build_host(garena.tobytes(), gops, mt["order"], mtd, obs, ori)
            assert file2 == S.model_build(payload, ops, obs, ori)[0], (name, bs, obs, ori)
        assert T.build_host(garena.tobytes(), gops, mt["order"], mtd, bs_, ri)[0] == image


@pytest.mark.parametrize("name", ["random_small_blocks", "tags", "corner_keys", "empty_and_deleted", "count_0"])
def test_memtable_get_over_the_scan_agrees_with_table_get(name):
    payload, ops, image, _, _ = built(name)
    table = T.open_host(image)[0]
    _, gops, garena, mt = scan_both(image, table)
    mtd = {k: mt[k] for k in ("entries", "user_keys", "status")}
    for key, seq in G.queries_for(image, payload, ops):
        a = MT.get_host(garena.tobytes(), gops, mt["order"], mtd, key, seq)
        b = T.get_host(image, table, key, seq)
        assert a["status"] == b["status"], (key, seq, a, b)
        if a["status"] in (G.FOUND, G.DELETED):
            assert int(gops[a["op"]]["tag"]) == b["tag"]


# ---- statuses ----
def test_every_status_and_the_retry():
    payload, ops, image, _, _ = built("random_small_blocks")
    table = C.open_table(image)
    full = C.model_scan(image, table)[0]
    ne, nb = full["table_entries"], full["table_bytes"]
    t = scan_both(image, table, op_cap=ne - 1, arena_cap=nb)[0]
    assert t["status"] == C.OP_OVER and (t["entries"], t["arena_bytes"], t["runs"]) == (ne, nb, full["runs"])
    t = scan_both(image, table, op_cap=ne, arena_cap=nb - 1)[0]
    assert t["status"] == C.ARENA_OVER
    t = scan_both(image, table, op_cap=0, arena_cap=0)[0]
    assert t["status"] == C.OP_OVER | C.ARENA_OVER
    assert scan_both(image, table, op_cap=t["entries"], arena_cap=t["arena_bytes"])[0]["status"] == 0  # the retry
    # BLOCK_OVER is the device's (the host twin has no block_cap): the model's rule here
    m = C.model_scan(image, table, block_cap=table["data_blocks"] - 1)[0]
    assert m["status"] == C.BLOCK_OVER and m["data_blocks"] == table["data_blocks"] and m["runs"] == 0
    assert C.model_scan(image, table, block_cap=table["data_blocks"])[0]["status"] == 0
    for name, (bad, kw, st) in G.open_cases().items():  # NO_TABLE from each open status
        tab = G.model_open(bad, **kw)[0]
        if tab["status"]:
            t = scan_both(bad, tab, tag_=name)[0]
            assert t["status"] == C.NO_TABLE and t["data_blocks"] == 0
    up = dict.fromkeys(C.TOTALS, 0)
    up.update(entries=3, arena_bytes=40, status=C.OP_OVER)
    t = scan_both(image, table, up, prev_out=(None, np.zeros(3, dtype=M.op_dtype()), np.zeros(40, dtype=np.uint8)))[0]
    assert t["status"] == C.UPSTREAM and (t["entries"], t["arena_bytes"], t["table_entries"]) == (3, 40, 0)
    t = scan_both(image, dict(table, status=G.BAD_INDEX), up,
                  prev_out=(None, np.zeros(3, dtype=M.op_dtype()), np.zeros(40, dtype=np.uint8)))[0]
    assert t["status"] == C.UPSTREAM | C.NO_TABLE
    assert scan_both(b"", C.open_table(b""))[0] == dict.fromkeys(C.TOTALS, 0)  # the empty table


def test_appending_two_and_three_tables():
    # (no table holds exact duplicates that differ in their values: the scan hands them on in table order, the
    # later op first, and a second sort would turn them round again)
    names = ["tags", "corner_keys", "duplicates"]
    parts = [built(n) for n in names]
    for k in (2, 3):
        prev, out, items = None, None, []
        for i in range(k):
            payload, ops, image, _, _ = parts[i]
            res = scan_both(image, C.open_table(image), prev, prev_out=out, tag_=(k, i))
            prev, out = res[0], res
            items += CASES[names[i]][0]
            assert prev["entries"] == len(items) and prev["table_entries"] == len(ops)
        _, gops, garena, _ = out
        order, mt = MT.build_host(garena.tobytes(), gops)
        file2 = T.build_host(garena.tobytes(), gops, order, mt, 256, 8)[0]
        payload, ops = make_table(items)
        assert file2 == S.model_build(payload, ops, 256, 8)[0], k
    # an append that does not fit leaves the first table's entries alone
    payload, ops, image, _, _ = parts[1]
    first = scan_both(parts[0][2], C.open_table(parts[0][2]))
    t = scan_both(image, C.open_table(image), first[0], prev_out=first, op_cap=first[0]["entries"] + len(ops) - 1,
                  arena_cap=1 << 20)[0]
    assert t["status"] == C.OP_OVER and t["entries"] == first[0]["entries"] + len(ops)


def test_unordered_and_a_block_named_twice():
    image = C.swapped_table()
    t, _, _, mt = scan_both(image, C.open_table(image))
    assert t["status"] == 0 and t["table_entries"] == 4 and mt["status"] == C.MT_UNORDERED and mt["user_keys"] == 0
    image = C.twice_table()
    t, ops, _, mt = scan_both(image, C.open_table(image))
    assert t["status"] == 0 and t["table_entries"] == 10 and t["data_blocks"] == 2 and mt["status"] == C.MT_UNORDERED
    assert (ops["tag"][:5] == ops["tag"][5:]).all()


@pytest.mark.parametrize("name", sorted(C.block_rule_cases()))
def test_block_rules(name):
    image, want = C.block_rule_cases()[name]
    table = C.open_table(image)
    assert table["status"] == 0
    t = scan_both(image, table, tag_=name)[0]
    assert t["status"] == want, (name, t)
    if name in ("n_0", "empty_block", "n_1_arr_0_restart_7"):
        assert (t["table_entries"], t["runs"]) == (0, 0 if name == "n_0" else 1)
    if name == "good":
        assert (t["table_entries"], t["runs"]) == (12, 3)


def test_varint_corner_cases_and_damaged_images():
    seen = set()
    for name, image, _, use, _ in G.damaged_cases(0):
        seen.add(scan_both(image, use, tag_=name)[0]["status"])
    assert seen == {0, C.NO_TABLE, C.CORRUPT}
    by = {name: scan_both(image, C.open_table(image))[0] for name, (image, _, _) in G.get_corruption_cases().items()
          if name != "index_handles"}
    assert by["good"]["status"] == 0 and by["varint_5_bytes_high_bits"]["status"] == 0
    assert by["entry_type_2"]["status"] == 0 and by["entry_type_2"]["table_entries"] == 22  # tags pass through
    assert by["n_0"]["status"] == 0 and by["n_0"]["table_entries"] == 10
    for name in ("type_byte_1", "n_large", "size_3", "restart_at_arr", "restart_beyond_arr", "restart_huge",
                 "shared_on_probed_restart", "shared_beyond_previous_key", "value_len_overruns", "non_shared_overruns",
                 "varint_6_bytes", "varint_runs_into_limit", "key_shorter_than_8", "scanned_key_shorter_than_8"):
        assert by[name]["status"] == C.CORRUPT, name


def test_random_flips_in_the_data_blocks():
    ok = bad = 0
    for i, (image, table) in enumerate(C.flip_cases()):
        st = scan_both(image, table, tag_=("flip", i))[0]["status"]
        assert st in (0, C.CORRUPT)
        ok += st == 0
        bad += st == C.CORRUPT
    assert ok >= 20 and bad >= 20, (ok, bad)


def test_foreign_tables_never_read_outside_the_file():
    """Each is CORRUPT or NO_TABLE (or, the index block intact, sound); the
    image sits in a heap block of exactly the table's file_bytes, so a read
    outside it is the host check program's to find (it replays these)."""
    image = G.base_image()[2]
    sts = []
    for t in C.foreign_tables(image):
        m = C.model_scan(image, t, file_cap=len(image))[0]
        sts.append(m["status"])
        if C.host_usable(image, t):
            assert scan_both(image[: t["file_bytes"]], t)[0]["status"] == m["status"]
    assert sts == [C.NO_TABLE, C.CORRUPT, C.CORRUPT, C.CORRUPT, C.CORRUPT, 0, C.CORRUPT, C.CORRUPT]


def test_dump_for_the_host_check_program(tmp_path):
    n = C.dump(str(tmp_path / "cases.bin"))
    assert n > 250 and os.path.getsize(tmp_path / "cases.bin") > 100000


# ---- argument checks ----
def test_scan_device_argument_checks():
    L = T._bind_scan()
    vp = ctypes.c_void_p
    cap, bc = 100, 10
    wsb = L.lv_sst_scan_workspace_bytes(cap, bc)
    err = lambda: lvgpu.lib().lv_last_error()

    def call(file=vp(0x100000), fcap=4096, tab=vp(0x200000), prev=None, arena=vp(0x300000), acap=4096, ops=vp(0x400000),
             c=cap, b=bc, order=None, mt=None, tot=vp(0x600000), flags=0, w=vp(0x4000000), wb=wsb):
        return L.lv_sst_scan_device(file, fcap, tab, prev, arena, acap, ops, c, b, order, mt, tot, flags, w, wb, None)

    assert call(file=None) == INVALID and b"null d_file" in err()
    assert call(tab=None) == INVALID and b"null d_table" in err()
    assert call(arena=None) == INVALID and b"null d_arena" in err()
    assert call(ops=None) == INVALID and b"null d_ops" in err()
    assert call(tot=None) == INVALID and b"null d_totals" in err()
    assert call(w=None) == INVALID and b"workspace" in err()
    assert call(ops=vp(0x400008)) == INVALID and b"d_ops must be 16-byte" in err()
    assert call(tab=vp(0x200004)) == INVALID and b"d_table must be 8-byte" in err()
    assert call(prev=vp(0x700004)) == INVALID and b"d_prev must be 8-byte" in err()
    assert call(tot=vp(0x600004)) == INVALID and b"d_totals must be 8-byte" in err()
    assert call(order=vp(0x800000), mt=vp(0x900004)) == INVALID and b"d_mt_totals must be 8-byte" in err()
    assert call(order=vp(0x800002), mt=vp(0x900000)) == INVALID and b"d_order must be 4-byte" in err()
    assert call(w=vp(0x4000008)) == INVALID and b"workspace must be 16-byte" in err()
    assert call(wb=wsb - 1) == INVALID and b"workspace too small" in err()
    assert call(flags=1) == INVALID and b"flag" in err()
    assert call(c=(1 << 32) - 1) == INVALID and b"op_cap too large" in err()
    assert call(b=(1 << 32) - 3) == INVALID and b"block_cap too large" in err()
    assert call(order=vp(0x800000)) == INVALID and b"go together" in err()
    assert call(mt=vp(0x900000)) == INVALID and b"go together" in err()
    assert call(order=vp(0x800000), mt=vp(0x900000), prev=vp(0x700000)) == INVALID and b"NULL d_prev" in err()
    assert call(prev=vp(0x600000)) == INVALID and b"d_prev must not be d_totals" in err()
    assert call(arena=vp(0x100800)) == INVALID and b"d_arena overlaps d_file" in err()
    assert call(ops=vp(0x100ff0)) == INVALID and b"d_ops overlaps d_file" in err()
    assert call(ops=vp(0x300ff0)) == INVALID and b"d_ops overlaps d_arena" in err()
    assert call(order=vp(0x100ffc), mt=vp(0x900000)) == INVALID and b"d_order overlaps d_file" in err()
    assert call(order=vp(0x300ffc), mt=vp(0x900000)) == INVALID and b"d_order overlaps d_arena" in err()
    assert call(order=vp(0x400c7c), mt=vp(0x900000)) == INVALID and b"d_order overlaps d_ops" in err()
    # the host twin's
    H = lambda *a: L.lv_sst_scan_host(*a)
    t, tot, mt = T.SstTable(), T.ScanTotals(), T.MtTotals()
    order = (ctypes.c_uint32 * 4)()
    assert H(None, None, None, None, 0, None, 0, None, None, ctypes.byref(tot)) == INVALID
    assert H(None, ctypes.byref(t), None, None, 0, None, 0, None, None, None) == INVALID
    assert H(None, ctypes.byref(t), ctypes.byref(tot), None, 0, None, 0, None, None, ctypes.byref(tot)) == INVALID
    assert H(None, ctypes.byref(t), None, None, 8, None, 0, None, None, ctypes.byref(tot)) == INVALID
    assert H(None, ctypes.byref(t), None, None, 0, None, 8, None, None, ctypes.byref(tot)) == INVALID
    assert H(None, ctypes.byref(t), None, None, 0, None, 0, order, None, ctypes.byref(tot)) == INVALID
    assert H(None, ctypes.byref(t), None, None, 0, None, 0, None, ctypes.byref(mt), ctypes.byref(tot)) == INVALID
    prev = T.ScanTotals()
    assert H(None, ctypes.byref(t), ctypes.byref(prev), None, 0, None, 0, order, ctypes.byref(mt), ctypes.byref(tot)) == INVALID
    assert H(None, ctypes.byref(t), None, None, 0, None, 0, order, ctypes.byref(mt), ctypes.byref(tot)) == 0


def test_without_a_gpu_a_well_formed_call_fails_with_the_runtimes_error():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = T._bind_scan()
    vp = ctypes.c_void_p
    wsb = L.lv_sst_scan_workspace_bytes(8, 8)
    rc = L.lv_sst_scan_device(vp(0x100000), 64, vp(0x200000), None, vp(0x300000), 64, vp(0x400000), 8, 8, None, None,
                              vp(0x600000), 0, vp(0x4000000), wsb, None)
    assert rc not in (0, -1)
    assert L.lv_last_error()


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
    for k in ("ss_header", "ss_blocks", "ss_carry", "ss_count", "ss_plan", "ss_emit", "ss_order", "ss_finish"):
        hits = {n: (spills[n], scratch[n]) for n in spills if k in n}
        assert hits and all(v == (0, 0) for v in hits.values()), (k, hits)
