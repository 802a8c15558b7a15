"""lv_sst_build_bloom_device, lv_sst_bloom_open_device and
lv_sst_get_bloom_device on the GPU against the Python model
(tests/sst_bloom_cases.py): every byte of the image, the handles and both
totals with canaries around them at the smallest shapes at which the kernels can
go wrong; the filtered get against lv_sst_get_device and the model's exact list
of rejected keys; damaged images against the host twin; the plain reader over
a bloom image; the device chain on one stream; graph capture."""
import numpy as np
import pytest

import lvgpu.compact as CP
import lvgpu.memtable as MT
import lvgpu.table as T
import memtable_cases as M
import sst_bloom_cases as B
import sst_build_cases as S
import sst_get_cases as G
import sst_scan_cases as SC
from memtable_cases import MAX_SEQUENCE, make_table, tag

pytestmark = pytest.mark.gpu

TILE = T.SB_TILE
CASES = B.cases()


def verify_all(built):
    t = built.sync_totals()
    st = T.verify_blocks(built.file_t[: t["file_bytes"]], built.handles_view())
    assert st.cpu().tolist() == [T.BLOCK_OK] * (t["data_blocks"] + 3)


@pytest.mark.parametrize("name", list(CASES))
def test_cases(gpu, name):
    import torch
    items, bs, ri, bpk = CASES[name]
    built, _, _, _ = B.check_device(torch, gpu, items, bs, ri, bpk, shift=3, tag_=name)
    if items:
        verify_all(built)


@pytest.mark.parametrize("shift", range(8))
def test_key_lengths_at_every_alignment(gpu, shift):
    """User keys of 0 .. 9 bytes, the payload shifted by 0 .. 7 bytes and gaps
    between the items: the hash's 4-byte steps and its tail at every alignment."""
    import torch
    items = CASES["key_lengths"][0] + [(bytes(range(97, 97 + n)) + b"!", tag(50 + n), b"") for n in range(10)]
    gaps = [(3 * i + shift) % 5 for i in range(len(items))]
    B.check_device(torch, gpu, items, 64, 2, 10, shift=shift, gaps=gaps, tag_=f"shift {shift}")


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1])
def test_entry_counts_around_the_tile(gpu, n):
    """block_size 32: a block holds one to three entries, so there are more
    than TILE / 3 blocks, some sixty to a window; op_cap and block_cap above
    the counts: surplus tiles and waves run and exit."""
    import torch
    items = S.tile_items(n, seed=1)
    B.check_device(torch, gpu, items, 32, 2, 10, tag_=f"n={n}")
    built, _, _, want = B.check_device(torch, gpu, items, 32, 2, 10, op_cap=4 * n, block_cap=n + 5, file_cap=1 << 20,
                                       tag_=f"n={n}, larger caps")
    assert want[2]["data_blocks"] > n // 4 and want[3]["filters"] > 8


def test_block_counts_around_the_tile(gpu):
    """The filter sizes are scanned by block id: TILE - 1, TILE and TILE + 1
    blocks (block_size 1: an entry per block)."""
    import torch
    for nb in (TILE - 1, TILE, TILE + 1):
        _, _, _, want = B.check_device(torch, gpu, S.seq_items(nb), 1, 16, 10, tag_=f"blocks={nb}")
        assert want[2]["data_blocks"] == nb


def test_one_filter_beyond_the_lds_budget(gpu):
    """60,000 entries with 8-byte keys under block_size 2^30: one block, one
    window, a filter of 75,000 bytes, set by atomic ORs on d_file."""
    import torch
    items = B.large_items()
    built, _, _, want = B.check_device(torch, gpu, items, 1 << 30, 16, 10, tag_="large")
    assert want[2]["data_blocks"] == 1 and want[3]["filter_size"] > 70000 > T.SB_BLOOM_LDS
    verify_all(built)


def test_large_filters_beside_each_other_and_a_small_one(gpu):
    """7,500 such entries under block_size 40,000: filters beyond the budget
    that share dwords with each other, and a last one inside it."""
    import torch
    items = B.large_items(7500)
    for shift in (0, 1):
        _, _, _, want = B.check_device(torch, gpu, items, 40000, 16, 10, shift=shift, tag_="large neighbours")
    fo, fs = want[1][-3]
    arr = fo + fs - 5 - 4 * want[3]["filters"]
    starts = sorted({G.le32(want[0], arr + 4 * i) for i in range(want[3]["filters"])} | {G.le32(want[0], fo + fs - 5)})
    sizes = [b - a for a, b in zip(starts, starts[1:])]
    assert max(sizes) > T.SB_BLOOM_LDS + 1 and 8 < min(sizes) <= T.SB_BLOOM_LDS + 1, sizes
    assert any(s % 4 for s in starts[1:-1])


def test_status_paths(gpu):
    import torch
    items, bs, ri, bpk = CASES["random_small_blocks"]
    payload, ops = make_table(items)
    want = B.model_build(payload, ops, bpk, bs, ri)
    tot = want[2]
    nb, fb = tot["data_blocks"], tot["file_bytes"]
    zero = dict.fromkeys(B.BLOOM_TOTALS, 0)

    def untouched(b):
        return B.tail_is_canary(b.file_t, 0) and B.tail_is_canary(b.handles_t, 0)

    def run(**kw):
        return B.run_device(torch, gpu, payload, ops, bpk, bs, ri, want=want, **kw)
    b = run(file_cap=fb - 1)
    assert b.sync_totals(check=False) == dict(tot, status=S.FILE_OVER) and untouched(b) and b.sync_bloom_totals() == zero
    with pytest.raises(T.LvError, match="lv_sst_build_bloom_device: status FILE_OVER"):
        b.sync_totals()
    b = run(block_cap=nb - 1)
    assert b.sync_totals(check=False) == dict(tot, status=S.HANDLE_OVER) and untouched(b) and b.sync_bloom_totals() == zero
    b = run(file_cap=0, block_cap=0)
    assert b.sync_totals(check=False) == dict(tot, status=S.FILE_OVER | S.HANDLE_OVER) and untouched(b)
    b = run(file_cap=fb + 100, block_cap=nb + 7, op_cap=len(ops) + 9)
    B.compare_device(b, want, "larger caps")
    b = run(mt_status=M.BAD_OP)
    assert b.sync_totals(check=False) == dict(zip(S.TOTALS, [0] * 7 + [S.NO_TABLE])) and untouched(b)
    assert b.sync_bloom_totals() == zero
    payload0, ops0 = make_table([])
    b = B.run_device(torch, gpu, payload0, ops0, file_cap=64, block_cap=4)
    assert b.sync_totals() == dict(zip(S.TOTALS, [0] * 8)) and untouched(b) and b.sync_bloom_totals() == zero


def test_block_large_from_a_data_block(gpu):
    """BLOCK_LARGE with the true u64 sizes of a table whose filter block lies
    beyond 4 GiB; nothing is written, no byte of the huge value is read."""
    import torch
    payload, ops = make_table([(b"a", tag(2), b"x"), (b"b", tag(1), b"y")])
    ops = ops.copy()
    ops[1]["val_off"], ops[1]["val_len"] = 16, (1 << 32) - 1
    d_pay = torch.empty((1 << 32) + 16, dtype=torch.uint8, device=gpu)
    d_pay[: len(payload)].copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
    table = MT.build_device(d_pay, M.dev_bytes(torch, gpu, ops), M.dev_i64(torch, gpu, [2]), op_cap=2)
    b = T.build_bloom_device(table, 10, file_cap=1 << 20, block_cap=4, fill=B.CANARY, guard=B.GUARD)
    t = b.sync_totals(check=False)
    assert t["status"] == S.BLOCK_LARGE | S.FILE_OVER and t["entries"] == 2 and t["data_blocks"] == 1
    # one block at offset 0 that ends beyond 2^32: more than 2^21 windows, 4 bytes of offset each
    assert t["file_bytes"] > (1 << 32) + 4 * (1 << 21) and t["metaindex_offset"] > (1 << 32) + 4 * (1 << 21)
    assert B.tail_is_canary(b.file_t, 0) and B.tail_is_canary(b.handles_t, 0)
    assert b.sync_bloom_totals() == dict.fromkeys(B.BLOOM_TOTALS, 0)


# ---- the read side ----
@pytest.fixture(scope="module")
def absent_table():
    items, bs, ri, bpk, absent = B.absent_source()
    payload, ops = make_table(items)
    return items, payload, ops, bs, ri, bpk, absent, B.model_build(payload, ops, bpk, bs, ri)


def test_filtered_get(gpu, absent_table):
    """The image built on the device, opened, its filter found, and gets: every
    stored key at and around its snapshot equals lv_sst_get_device in every
    field; for absent keys the model says exactly which are filtered, and at
    least 90 % of them are."""
    import torch
    items, payload, ops, bs, ri, bpk, absent, want = absent_table
    built = B.run_device(torch, gpu, payload, ops, bpk, bs, ri, want=want)
    B.compare_device(built, want, "absent_source")
    op = T.open_device(built.file_t[: built.file_cap], built.totals[2:3], built.totals[7:8], block_cap=built.block_cap)
    bloom_t = T.bloom_open_device(op)
    image = want[0]
    table = G.model_open(image)[0]
    bloom = B.model_bloom_open(image, table)
    assert op.sync() == table and T.bloom_dict(bloom_t) == bloom and bloom["present"] == 1
    assert (bloom["filter_offset"], bloom["filter_size"]) == want[1][-3]
    st = T.verify_blocks(built.file_t[: len(image)], bloom_t[:2].view(1, 2))
    assert st.cpu().tolist() == [T.BLOCK_OK]
    stored = B.queries_for(payload, ops, bs, ri)
    queries = stored + [(k, MAX_SEQUENCE) for k in absent]
    qk, off, ln, sq, bad = G.pack_queries(queries)
    got = B.run_get(torch, gpu, op, bloom_t, qk, off, ln, sq)
    plain = G.run_get(torch, gpu, op, qk, off, ln, sq)
    wants = [B.model_get(image, table, bloom, k, s, bad_query=b)
             for (k, s), b in zip(queries + [(b"", 1)], bad)]
    assert B.result_dicts(got) == wants
    nf = 0
    for i, (g, p) in enumerate(zip(B.result_dicts(got), B.result_dicts(plain))):
        if g["reserved"]:
            assert p["status"] == G.ABSENT and g == dict(p, reserved=B.FILTERED), i
            nf += i >= len(stored)
        else:
            assert g == p, i
    # a stored version is never filtered at or above its own snapshot (below it the seek may land in
    # the next block, whose filter need not hold the key)
    seq_of = {k: t >> 8 for k, t, _ in items}
    for (k, s), g in zip(stored, B.result_dicts(got)):
        if k in seq_of and seq_of[k] <= s <= MAX_SEQUENCE:
            assert not g["reserved"] and g["status"] == G.FOUND, (k, s)
    assert {G.FOUND, G.ABSENT, G.BAD_SEQ, G.BAD_QUERY} <= {w["status"] for w in wants}
    print("filtered", nf, "of", len(absent))
    assert nf >= 0.9 * len(absent)


def test_an_image_without_a_filter(gpu):
    """lv_sst_build_device's image: present == 0, NO_ENTRY, and the results of
    lv_sst_get_bloom_device are lv_sst_get_device's byte for byte."""
    import torch
    items, bs, ri, bpk = CASES["block_256"]
    payload, ops = make_table(items)
    image = S.model_build(payload, ops, bs, ri)[0]
    op, bloom_t, owner = B.open_both(torch, gpu, image, shift=5)
    assert T.bloom_dict(bloom_t) == dict(dict.fromkeys(B.BLOOM_FIELDS, 0), why=B.WHY_NO_ENTRY)
    qk, off, ln, sq, _ = G.pack_queries(G.queries_for(image, payload, ops))
    got = B.run_get(torch, gpu, op, bloom_t, qk, off, ln, sq)
    assert got.tobytes() == G.run_get(torch, gpu, op, qk, off, ln, sq).tobytes()


def test_damaged_images_equal_the_host_twin(gpu):
    """Every `why` (the empty table, a NULL d_file with file_cap 0, among them)
    and the random flips inside the filter block, the metaindex block and the
    footer that tools/sst_bloom_host_check.cc replays from the dump: the
    device's lv_sst_bloom and results are the host twin's (and the model's);
    with no filter they are the plain get's."""
    import torch
    seen = set()
    for i, (name, image, queries) in enumerate(B.damaged_cases()):
        table, bloom, wants = B.host_answers(image, queries)
        assert (bloom, wants) == B.model_answers(image, queries)[1:], name
        op, bloom_t, owner = B.open_both(torch, gpu, image, shift=i % 8)
        qk, off, ln, sq, _ = G.pack_queries(queries, bad_query=False)
        got = B.run_get(torch, gpu, op, bloom_t, qk, off, ln, sq)
        assert op.sync(check=False) == table and T.bloom_dict(bloom_t) == bloom, (name, T.bloom_dict(bloom_t), bloom)
        assert B.result_dicts(got) == wants, name
        if not bloom["present"]:
            assert got.tobytes() == G.run_get(torch, gpu, op, qk, off, ln, sq).tobytes(), name
        seen.add(bloom["why"])
    assert seen == set(range(9))


def test_a_table_that_does_not_fit_file_cap(gpu):
    """A d_table the open did not write for this buffer: its file_bytes is one
    beyond file_cap.  lv_sst_bloom_open_device says TABLE and reads nothing of
    the image; every get is NO_TABLE."""
    import torch
    items, bs, ri, bpk = CASES["block_256"]
    payload, ops = make_table(items)
    image = B.model_build(payload, ops, bpk, bs, ri)[0]
    op, bloom_t, owner = B.open_both(torch, gpu, image, shift=2)
    assert T.bloom_dict(bloom_t)["present"] == 1
    cap = len(image) - 1
    small = T.Opened(op.file_t[:cap], cap, op.table, None, 0, None)
    bloom_t = T.bloom_open_device(small)
    table = G.model_open(image)[0]
    want = B.model_bloom_open(image, table, file_cap=cap)
    assert T.bloom_dict(bloom_t) == want == dict(dict.fromkeys(B.BLOOM_FIELDS, 0), why=B.WHY_TABLE)
    queries = B.queries_for(payload, ops, bs, ri)[::9]
    qk, off, ln, sq, _ = G.pack_queries(queries, bad_query=False)
    got = B.run_get(torch, gpu, small, bloom_t, qk, off, ln, sq)
    assert B.result_dicts(got) == [B.model_get(image, table, want, k, s, file_cap=cap) for k, s in queries]
    assert set(got["status"].tolist()) <= {G.NO_TABLE, G.BAD_SEQ}


def test_a_bloom_struct_of_another_file(gpu):
    """A d_bloom that was not written for this file: every offset is checked
    against file_bytes again; the image sits between canaries at the end of
    its allocation's used part, and the answers are the model's."""
    import torch
    items, bs, ri, bpk = CASES["block_256"]
    payload, ops = make_table(items)
    image = B.model_build(payload, ops, bpk, bs, ri)[0]
    op, bloom_t, owner = B.open_both(torch, gpu, image)
    table, bloom, _ = B.model_answers(image, [])
    queries = B.queries_for(payload, ops, bs, ri)[::7]
    qk, off, ln, sq, _ = G.pack_queries(queries, bad_query=False)
    for patch in (dict(filter_offset=len(image)), dict(filter_size=len(image)), dict(filter_size=4),
                  dict(array_offset=bloom["filter_size"]), dict(num=bloom["num"] + 1), dict(num=1 << 62),
                  dict(filter_offset=(1 << 64) - 3), dict(base_lg=64), dict(base_lg=1 << 40), dict(present=2)):
        b = dict(bloom, **patch)
        vals = np.array([b[f] for f in B.BLOOM_FIELDS], dtype=np.uint64)
        bloom_t.copy_(torch.from_numpy(vals.view(np.int64).copy()))
        got = B.run_get(torch, gpu, op, bloom_t, qk, off, ln, sq)
        assert B.result_dicts(got) == [B.model_get(image, table, b, k, s) for k, s in queries], patch


def test_the_plain_reader_takes_a_bloom_image(gpu):
    """lv_sst_open_device, lv_sst_scan_device and lv_sst_verify_blocks_device
    over a bloom image: the open's handles are the data blocks, the metaindex
    and the index; the scan equals the scan of the plain image."""
    import torch
    items, bs, ri, bpk = CASES["block_5000"]
    payload, ops = make_table(items)
    want = B.model_build(payload, ops, bpk, bs, ri)
    plain = S.model_build(payload, ops, bs, ri)[0]
    outs = []
    for image in (want[0], plain):
        op, owner, table = G.check_open(torch, gpu, image, shift=1)
        full = SC.model_scan(image, table)[0]
        sc = SC.run_scan(torch, gpu, op, arena_cap=full["table_bytes"], op_cap=full["table_entries"],
                         block_cap=table["data_blocks"])
        outs.append((sc.sync(), sc.ops().tobytes(), sc.arena()))
    assert outs[0][1:] == outs[1][1:] and outs[0][0] == outs[1][0]
    assert outs[0][0]["table_entries"] == len(items)


def test_chain_with_no_host_sync(gpu):
    """scan -> sort -> compaction filter -> bloom build -> open -> bloom open
    -> bloom get on one stream, one synchronisation at the end."""
    import torch
    rng = np.random.default_rng(4)
    items = M.random_items(rng, 1500, alphabet=4, maxlen=10, seqs=30)
    payload, ops = make_table(items)
    source = S.model_build(payload, ops, 512, 8)[0]
    tab = SC.open_table(source)
    full = SC.model_scan(source, tab)[0]
    queries = M.queries_for(payload, ops)[::2] + [(b"absent%d" % i, MAX_SEQUENCE) for i in range(300)]
    qk, off, ln, sq = M.pack_queries(queries)
    dq = G.dev_queries(torch, gpu, qk, off, ln, sq)
    s = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        op0, owner = SC.open_on(torch, gpu, source, shift=2, stream=s)
        sc = SC.run_scan(torch, gpu, op0, arena_cap=full["table_bytes"], op_cap=full["table_entries"],
                         block_cap=tab["data_blocks"], stream=s)
        table = MT.build_device(sc.arena_t[: sc.arena_cap], sc.ops_t, sc.totals[0:1], sc.totals[7:8], op_cap=sc.op_cap,
                                stream=s)
        f = CP.filter_device(table, 40, None, 0, stream=s)  # above every sequence: shadowed versions go
        built = T.build_bloom_device(f, 10, block_size=1024, stream=s, fill=B.CANARY, guard=B.GUARD)
        op = T.open_device(built.file_t[: built.file_cap], built.totals[2:3], built.totals[7:8],
                           block_cap=built.block_cap, stream=s)
        bloom_t = T.bloom_open_device(op, stream=s)
        st = T.verify_blocks(built.file_t[: built.file_cap], built.handles_t[: 2 * (built.block_cap + 3)], stream=s)
        gets = T.get_bloom_device(op, bloom_t, *dq, nq=len(queries), stream=s)
        plain = T.get_device(op, *dq, nq=len(queries), stream=s)
    s.synchronize()
    kept = f.sync()["kept"]
    t, bt = built.sync_totals(), built.sync_bloom_totals()
    assert t["entries"] == kept == bt["filter_keys"] and 0 < kept < len(items)
    image = built.file()
    mt, mb, _ = B.model_answers(image, [])
    assert op.sync() == mt and T.bloom_dict(bloom_t) == mb and mb["present"] == 1
    assert (mb["filter_offset"], mb["filter_size"]) == (bt["filter_offset"], bt["filter_size"])
    nh = t["data_blocks"] + 3
    st = st.cpu().tolist()
    assert st[:nh] == [T.BLOCK_OK] * nh and set(st[nh:]) <= {T.BLOCK_OUT_OF_RANGE}
    got, base = gets.sync(), plain.sync()
    assert B.result_dicts(got) == [B.model_get(image, mt, mb, k, q) for k, q in queries]
    nf = 0
    for g, p in zip(B.result_dicts(got), B.result_dicts(base)):
        nf += g["reserved"]
        assert g == (dict(dict.fromkeys(G.RESULT_FIELDS, 0), reserved=1) if g["reserved"] else p)
    assert nf >= 250 and {G.FOUND, G.DELETED, G.ABSENT} <= set(got["status"].tolist())


def test_graph_capture(gpu):
    """Memtable build + bloom build + open + bloom open + bloom get captured
    into one graph after a warm-up; replays over other tables of one capacity."""
    import torch
    sets = []
    for seed, n in ((1, TILE + 7), (2, TILE // 2), (3, 2000)):
        items = S.tile_items(n, seed=seed)
        payload, ops = make_table(items)
        want = B.model_build(payload, ops, 10, 200, 4)
        queries = (B.queries_for(payload, ops, 200, 4)[::9] + [(b"none%d" % i, MAX_SEQUENCE) for i in range(200)])[:500]
        table, bloom, wants = B.model_answers(want[0], queries)
        sets.append((payload, ops, want, G.pack_queries(queries, bad_query=False), wants))
    size = max(len(x[0]) for x in sets)
    cap = max(len(x[1]) for x in sets)
    nq = min(len(x[4]) for x in sets)
    qbytes = max(len(x[3][0]) for x in sets)
    fcap = T.bloom_file_bound(size, cap, 10)
    d_pay = torch.zeros(size, dtype=torch.uint8, device=gpu)
    d_ops = torch.zeros(cap * 32, dtype=torch.uint8, device=gpu)
    d_n = torch.zeros(1, dtype=torch.int64, device=gpu)
    d_qk = torch.zeros(qbytes, dtype=torch.uint8, device=gpu)
    d_off = torch.zeros(nq, dtype=torch.int64, device=gpu)
    d_len = torch.zeros(nq, dtype=torch.int32, device=gpu)
    d_seq = torch.zeros(nq, dtype=torch.int64, device=gpu)
    mws = torch.empty(MT.build_workspace_bytes(cap), dtype=torch.uint8, device=gpu)
    sws = torch.empty(T.build_bloom_workspace_bytes(cap, cap), dtype=torch.uint8, device=gpu)

    def load(k):
        payload, ops, _, (qk, off, ln, sq, _), _ = sets[k]
        d_pay.zero_()
        d_pay[: len(payload)].copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
        d_ops[: len(ops) * 32].copy_(torch.frombuffer(bytearray(ops.tobytes()), dtype=torch.uint8))
        d_n.fill_(len(ops))
        d_qk.zero_()
        d_qk[: len(qk)].copy_(torch.frombuffer(bytearray(qk), dtype=torch.uint8))
        d_off.copy_(torch.from_numpy(off[:nq].view(np.int64).copy()))
        d_len.copy_(torch.from_numpy(np.ascontiguousarray(ln[:nq]).view(np.int32).copy()))
        d_seq.copy_(torch.from_numpy(sq[:nq].view(np.int64).copy()))

    def run(stream=None):
        table = MT.build_device(d_pay, d_ops, d_n, op_cap=cap, workspace=mws, stream=stream)
        built = T.build_bloom_device(table, 10, block_size=200, restart_interval=4, file_cap=fcap, block_cap=cap,
                                     workspace=sws, stream=stream, fill=B.CANARY, guard=B.GUARD)
        op = T.open_device(built.file_t[:fcap], built.totals[2:3], built.totals[7:8], handles=False, stream=stream)
        bloom_t = T.bloom_open_device(op, stream=stream)
        gets = T.get_bloom_device(op, bloom_t, d_qk, d_off, d_len, d_seq, nq=nq, stream=stream, fill=B.CANARY,
                                  guard=B.GUARD)
        return built, op, bloom_t, gets

    def verify(k, out, what):
        built, op, bloom_t, gets = out
        torch.cuda.synchronize()
        fresh = T.BuiltBloom(built.file_t, built.file_cap, built.handles_t, built.block_cap, built.totals, None,
                             built.bloom_totals)
        B.compare_device(fresh, sets[k][2], what)
        assert T.bloom_dict(bloom_t)["present"] == 1, what
        assert B.result_dicts(T.Gets(gets.res, nq, None).sync()) == sets[k][4][:nq], what
        assert B.tail_is_canary(gets.res, 32 * nq), what

    load(0)
    verify(0, run(), "warm")
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = run(s)
    torch.cuda.synchronize()
    for k in (1, 2, 0):
        load(k)
        out[0].file_t.fill_(B.CANARY)
        out[0].handles_t.view(torch.uint8).fill_(B.CANARY)
        out[3].res.fill_(B.CANARY)
        sws.fill_(0x33)
        torch.cuda.synchronize()
        g.replay()
        verify(k, out, f"replay of set {k}")
