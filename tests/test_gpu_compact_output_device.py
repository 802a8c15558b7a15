"""lv_compact_output_device on the GPU against the serial model
(tests/compact_output_cases.py): every byte of the arena with the gaps between
the files, the handles, the four record arrays, the bound keys, the cursor and
the totals, all between canaries, at the smallest shapes at which the kernels
can go wrong; every file's handles through lv_sst_verify_blocks_device.  Each
test first asserts on the model's own output that the shape is what it claims."""
import numpy as np
import pytest

import compact_output_cases as CO
import lvgpu.compact as C
import lvgpu.table as T
import lvgpu.version as LV
import memtable_cases as M
import sst_bloom_cases as B
import sst_build_cases as S
import sst_get_cases as G
import version_cases as V
from memtable_cases import MAX_SEQUENCE, make_table, tag

pytestmark = pytest.mark.gpu

TILE = CO.TILE
CASES = CO.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_cases(gpu, name):
    import torch
    items, bs, ri, bpk, mf = CASES[name]
    CO.check_device(torch, gpu, items, bs, ri, bpk, mf, shift=3, tag_=name)


@pytest.mark.parametrize("bpk", [None, 10])
def test_one_file_is_the_existing_build(gpu, bpk):
    """max_file_bytes = 2^63: one file, whose arena bytes and handles are those
    of lv_sst_build_device / lv_sst_build_bloom_device over the same input."""
    import torch
    items, bs, ri = S.cases()["random_small_blocks"]
    payload, ops = make_table(items)
    out, w = CO.run_device(torch, gpu, payload, ops, CO.NO_LIMIT, bpk, bs, ri)
    assert w.totals["files"] == 1 and w.totals["data_blocks"] > 20
    CO.compare_device(out, w)
    built = (B.run_device(torch, gpu, payload, ops, bpk, bs, ri) if bpk else S.run_device(torch, gpu, payload, ops, bs, ri))
    t = built.sync_totals()
    assert t["file_bytes"] == w.totals["arena_bytes"]
    assert built.file() == out.image(0)
    assert built.handles() == w.handles


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1])
def test_an_entry_per_file_around_the_tile(gpu, n):
    """block_size 1 and max_file_bytes 1: every entry is a block and a file, so
    the scans by block and by file cross a tile edge."""
    import torch
    w = CO.check_device(torch, gpu, S.seq_items(n), 1, 16, 10 if n == TILE else None, 1, tag_=f"files={n}")[1]
    assert w.totals["files"] == n == w.totals["data_blocks"]


def test_the_example(gpu):
    import torch
    g = CO.load_golden()
    items = [(k.encode(), tag(s), v.encode()) for k, s, v in g["entries"]]
    out, w = CO.check_device(torch, gpu, items, g["block_size"], g["restart_interval"], None, g["max_file_bytes"])
    assert [out.image(k).hex() for k in range(2)] == g["images"]
    assert w.offs == [0, 128] and w.totals == g["totals"]


def test_the_cut_moves_by_one_block_at_the_threshold(gpu):
    import torch
    blocks = []
    for d in (-1, 0, 1):
        items, bs, ri, bpk, mf = CASES[f"cut_{d:+d}"]
        w = CO.check_device(torch, gpu, items, bs, ri, bpk, mf, tag_=f"cut {d:+d}")[1]
        blocks.append(w.files[0]["data_blocks"])
        assert w.flushed(0) >= mf
    assert blocks == [2, 2, 3]


def test_ending_on_a_flushed_and_on_an_open_block(gpu):
    import torch
    items, bs, ri, bpk, mf = CASES["end_on_flush"]
    w = CO.check_device(torch, gpu, items, bs, ri, bpk, mf, tag_="flushed")[1]
    assert w.last_by_cut and len(w.files) >= 2 and w.flushed(len(w.files) - 1) >= mf
    items, bs, ri, bpk, mf = CASES["end_open"]
    w = CO.check_device(torch, gpu, items, bs, ri, bpk, mf, tag_="open")[1]
    assert not w.last_by_cut and len(w.files) >= 2 and w.flushed(len(w.files) - 1) < mf


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1])
def test_entry_counts_around_the_tile(gpu, n):
    """A few entries per block and a few blocks per file; then every capacity
    well above the counts: surplus tiles and waves run and exit."""
    import torch
    items = S.tile_items(n, seed=2)
    w = CO.check_device(torch, gpu, items, 32, 2, 10, 100, tag_=f"n={n}")[1]
    assert w.totals["files"] >= 8 and w.totals["data_blocks"] > 2 * w.totals["files"] and n > w.totals["data_blocks"]
    CO.check_device(torch, gpu, items, 32, 2, 10, 100, op_cap=4 * n, block_cap=n + 5, files_cap=n + 9,
                    arena_cap=1 << 20, bound_cap=1 << 16, tag_=f"n={n}, larger caps")


def windows_of(w, k):
    """The 2 KiB windows of file k's offsets in which a data block starts."""
    f = w.files[k]
    return sorted({off >> 11 for off, _ in w.handles[f["first_handle"]: f["first_handle"] + f["data_blocks"]]})


def test_filters_per_file(gpu):
    """max_file_bytes 5,000: every file, the last one (closed by the end of the
    input) included, spans three 2 KiB windows of its own offsets, window 0
    starts again in every file, and the first file has a window without a
    block start (its filter is zero bytes)."""
    import torch
    items = [(b"000000", tag(1), b"B" * 4500)] + B.window_items(1030, start=1)
    payload, ops = make_table(items)
    w = CO.model_output(payload, ops, 5000, 10, 32, 16, bound_used=5)
    assert len(w.files) >= 5 and not w.last_by_cut
    for k in range(len(w.files)):
        assert windows_of(w, k)[0] == 0 and w.blooms[k]["num"] >= 3, k
    assert windows_of(w, 0)[:2] == [0, 2] and w.files[0]["data_blocks"] > 3
    assert all(windows_of(w, k)[:3] == [0, 1, 2] for k in range(1, len(w.files)))
    out, _ = CO.run_device(torch, gpu, payload, ops, 5000, 10, 32, 16, want=w)
    CO.compare_device(out, w, "windows")


def test_a_filter_beyond_the_lds_budget_next_to_a_small_file(gpu):
    import torch
    big = B.large_items(20000)
    payload, ops = make_table(big)
    raw = S.model_build(payload, ops, 1 << 30, 16)[1][0][1]  # the one block's size = its last estimate
    items = big + [(b"z%d" % i, tag(1), b"v") for i in range(5)]
    payload, ops = make_table(items)
    w = CO.model_output(payload, ops, 1, 10, raw, 16, bound_used=5)
    assert [f["entries"] for f in w.files] == [20000, 5] and w.blooms[0]["array_offset"] > T.SB_BLOOM_LDS
    out, _ = CO.run_device(torch, gpu, payload, ops, 1, 10, raw, 16, want=w)
    CO.compare_device(out, w, "large filter")


@pytest.mark.parametrize("shift", range(8))
def test_alignment_and_long_copies(gpu, shift):
    """The payload shifted by 0 .. 7 bytes with gaps between the items; a key
    suffix and a value of at least the wave-copy threshold directly before and
    behind a cut, so the files' bound keys are long copies too."""
    import torch
    long_ = T.SB_WAVE_COPY + 9
    items = [(bytes(range(97, 97 + n)) + b"!", tag(50 + n), b"v" * n) for n in range(10)]
    items += [(b"m" + b"K" * long_, tag(3), b"V" * (long_ + shift)), (b"n" + b"Q" * (long_ + 5), tag(4), b"W" * long_),
              (b"o", tag(5), b"")]
    gaps = [(3 * i + shift) % 5 for i in range(len(items))]
    payload, ops = make_table(items, gaps)
    ents = S.entries_of(payload, ops)
    at = next(i for i, (k, _) in enumerate(ents) if k.startswith(b"m"))
    w = CO.model_output(payload, ops, 150, 10, 64, 2, bound_used=5)
    cut = [f["first_entry"] for f in w.files]
    assert len(cut) >= 3 and any(c in (at, at + 1, at + 2) for c in cut[1:]), cut
    assert max(v["largest_len"] for v in w.vfiles) >= T.SB_WAVE_COPY
    out, _ = CO.run_device(torch, gpu, payload, ops, 150, 10, 64, 2, want=w, shift=shift)
    CO.compare_device(out, w, f"shift {shift}")


def test_statuses_leave_everything_untouched(gpu):
    """Each capacity one short of the model's count: its bit alone, the true
    totals, and no byte of any output but the totals."""
    import torch
    items, bs, ri, bpk, mf = CASES["small_files_10"]
    payload, ops = make_table(items)
    w = CO.model_output(payload, ops, mf, bpk, bs, ri, bound_used=5)
    t = w.totals
    shorts = {"arena_cap": (t["arena_bytes"] - 1, CO.ARENA_OVER), "block_cap": (t["data_blocks"] - 1, CO.HANDLE_OVER),
              "files_cap": (t["files"] - 1, CO.FILES_OVER), "bound_cap": (w.used - 1, CO.BOUND_OVER)}
    for cap, (val, bit) in shorts.items():
        out, _ = CO.run_device(torch, gpu, payload, ops, mf, bpk, bs, ri, want=w, **{cap: val})
        got = out.sync(check=False)
        assert got == dict(t, status=bit), (cap, got)
        CO.untouched_device(out)
    out, _ = CO.run_device(torch, gpu, payload, ops, mf, bpk, bs, ri, want=w, arena_cap=0, block_cap=0, files_cap=0,
                           bound_cap=0)
    assert out.sync(check=False) == dict(t, status=CO.ARENA_OVER | CO.HANDLE_OVER | CO.FILES_OVER | CO.BOUND_OVER)
    CO.untouched_device(out)
    out, _ = CO.run_device(torch, gpu, payload, ops, mf, bpk, bs, ri, want=w, mt_status=1)
    assert out.sync(check=False) == dict.fromkeys(CO.TOTALS, 0) | dict(status=CO.NO_TABLE)
    CO.untouched_device(out)


@pytest.mark.parametrize("bpk", [None, 10])
def test_block_large(gpu, bpk):
    """A data block of 2^32 - 1 bytes or more: BLOCK_LARGE with the true u64
    totals of the host twin's sizing pass (two files: the large block closes
    the first), beside ARENA_OVER, and every output untouched.  The value's
    extent lies in a 4 GiB tensor that is allocated but never filled; no byte
    of it is read, because nothing is emitted."""
    import torch
    import lvgpu.memtable as MT
    payload, ops, order, mt, claimed, bs, ri, mf = CO.block_large_case()
    want = C.output_host(payload, ops, order, mt, mf, bits_per_key=bpk, block_size=bs, restart_interval=ri,
                         payload_bytes=claimed, sizing=True).totals
    assert want["status"] == CO.BLOCK_LARGE and want["files"] == 2 and want["arena_bytes"] > 1 << 32
    d_pay = torch.empty(claimed, dtype=torch.uint8, device=gpu)
    d_pay[: len(payload)].copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
    table = MT.build_device(d_pay, M.dev_bytes(torch, gpu, ops), M.dev_i64(torch, gpu, [3]), op_cap=3)
    assert table.sync_totals()["entries"] == 3
    for caps, bits in ((dict(arena_cap=1 << 20, block_cap=2, files_cap=2, bound_cap=5 + 36), CO.ARENA_OVER),
                       (dict(arena_cap=1 << 20, block_cap=1, files_cap=1, bound_cap=5 + 35),
                        CO.ARENA_OVER | CO.HANDLE_OVER | CO.FILES_OVER | CO.BOUND_OVER)):
        out = C.output_device(table, mf, bits_per_key=bpk, block_size=bs, restart_interval=ri,
                              used_t=M.dev_i64(torch, gpu, [5]), fill=CO.CANARY, guard=CO.GUARD, **caps)
        assert out.sync(check=False) == dict(want, status=CO.BLOCK_LARGE | bits), caps
        CO.untouched_device(out)
    del d_pay, table
    torch.cuda.empty_cache()


def test_hostile_ops_are_no_table(gpu):
    import torch
    items, bs, ri, bpk, mf = CASES["small_files_10"]
    payload, ops = make_table(items)
    w = CO.model_output(payload, ops, mf, bpk, bs, ri, bound_used=5)
    table, buf = M.run_build(torch, gpu, payload, ops)
    table.sync_totals()
    bad = ops.copy()
    bad[len(bad) // 2]["val_len"] = 0xFFFFFFFF
    table.ops_t[: 32 * len(bad)].copy_(torch.from_numpy(np.frombuffer(bad.tobytes(), dtype=np.uint8).copy()))
    out = C.output_device(table, mf, bits_per_key=bpk, block_size=bs, restart_interval=ri,
                           arena_cap=w.totals["arena_bytes"], block_cap=w.totals["data_blocks"],
                           files_cap=w.totals["files"], bound_cap=w.used, used_t=M.dev_i64(torch, gpu, [5]),
                           fill=CO.CANARY, guard=CO.GUARD)
    assert out.sync(check=False) == dict.fromkeys(CO.TOTALS, 0) | dict(status=CO.NO_TABLE)
    CO.untouched_device(out)


def test_no_records_asked_for(gpu):
    """d_blooms and d_version_files NULL: no bound keys, bound_bytes 0, the
    cursor stays."""
    import torch
    items, bs, ri, bpk, mf = CASES["small_files_10"]
    payload, ops = make_table(items)
    w = CO.model_output(payload, ops, mf, bpk, bs, ri, version_files=False)
    table, buf = M.run_build(torch, gpu, payload, ops)
    out = C.output_device(table, mf, bits_per_key=bpk, block_size=bs, restart_interval=ri, blooms=False,
                          version_files=False, used_t=M.dev_i64(torch, gpu, [7]), fill=CO.CANARY, guard=CO.GUARD)
    assert out.sync() == w.totals and w.totals["bound_bytes"] == 0
    assert [out.image(k) for k in range(len(w.images))] == w.images
    assert CO.tail_is_canary(out.bounds_t, 0) and int(out.used_t.cpu()[0]) == 7


def test_the_run_opens_as_a_level_and_answers(gpu):
    """The chain on the device: the output's records go to
    lv_version_open_device as they are, and every key of the input is answered
    as the model of Version::Get answers over the same arrays."""
    import torch
    items, bs, ri, bpk, mf = S.seq_items(600, klen=5, vlen=7), 48, 3, 10, 300
    payload, ops = make_table(items)
    out, w = CO.run_device(torch, gpu, payload, ops, mf, bpk, bs, ri, level=2, first_number=40)
    t = out.sync()
    assert t["files"] >= 8
    opened = LV.open_device(out.arena_t, out.version_files_t, out.tables_t.view(torch.int64), t["files"], out.bounds_t,
                            blooms_t=out.blooms_t.view(torch.int64), images_bytes=t["arena_bytes"], bounds_bytes=w.used)
    state = opened.sync(check=False)
    ver = V.ver_from_device(torch, opened)
    assert state == V.model_open(ver) and state["status"] == 0 and state["level_start"][2:4] == [0, t["files"]]
    queries = sorted({(k, MAX_SEQUENCE) for k, _, _ in items} | {(k, t_ >> 8) for k, t_, _ in items} |
                     {(k + b"x", MAX_SEQUENCE) for k, _, _ in items[::7]})
    qk, off, ln, sq, bad = G.pack_queries(queries)
    qs = queries + [(b"", 1)] * (len(bad) - len(queries))
    got = LV.get_device(opened, *G.dev_queries(torch, gpu, qk, off, ln, sq), nq=len(off)).sync()
    wants = [V.model_get(ver, state, k, s, bad_query=b) for (k, s), b in zip(qs, bad)]
    seen = V.compare_results(got, wants, "run")
    assert {G.FOUND, G.ABSENT} <= seen
    found = [w_ for w_ in wants if w_["status"] == G.FOUND]
    assert len(found) >= 2 * len(items) and len({w_["file"] for w_ in found}) == t["files"]


def test_graph_replay(gpu):
    """The call captured into a HIP graph and replayed over other inputs of the
    same capacities."""
    import torch
    import lvgpu.memtable as MT
    sets = []
    for seed in (0, 1, 2):
        items = S.tile_items(500 + 40 * seed, seed=seed)
        payload, ops = make_table(items)
        sets.append((payload, ops, CO.model_output(payload, ops, 100, 10, 32, 2, bound_used=5)))
    cap, pcap = 700, max(len(s[0]) for s in sets) + 64
    d_pay = torch.zeros(pcap, dtype=torch.uint8, device=gpu)
    d_ops = torch.zeros(32 * cap, dtype=torch.uint8, device=gpu)
    d_n = torch.zeros(1, dtype=torch.int64, device=gpu)
    used_t = torch.zeros(1, dtype=torch.int64, device=gpu)
    mws = torch.empty(MT.build_workspace_bytes(cap), dtype=torch.uint8, device=gpu)
    ows = torch.empty(C.output_workspace_bytes(cap, cap, cap), dtype=torch.uint8, device=gpu)

    def load(k):
        payload, ops, _ = sets[k]
        d_pay[: len(payload)].copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
        d_ops[: 32 * len(ops)].copy_(torch.from_numpy(np.frombuffer(ops.tobytes(), dtype=np.uint8).copy()))
        d_n.fill_(len(ops))
        used_t.fill_(5)

    def run(stream=None):
        table = MT.build_device(d_pay, d_ops, d_n, op_cap=cap, workspace=mws, stream=stream)
        return C.output_device(table, 100, bits_per_key=10, block_size=32, restart_interval=2, arena_cap=1 << 17,
                               block_cap=cap, files_cap=cap, bound_cap=1 << 15, used_t=used_t, workspace=ows,
                               stream=stream, fill=CO.CANARY, guard=CO.GUARD)

    load(0)
    out = run()
    CO.compare_device(out, sets[0][2], "warm")
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = run(s)
    torch.cuda.synchronize()
    for k in (1, 2, 0):
        load(k)
        for t_ in (out.arena_t, out.handles_t, out.files_t, out.tables_t, out.blooms_t, out.version_files_t, out.bounds_t):
            t_.view(torch.uint8).fill_(CO.CANARY)
        ows.fill_(0x33)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        out._tot = None
        CO.compare_device(out, sets[k][2], f"replay of set {k}")
