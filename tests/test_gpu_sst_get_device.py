"""lv_sst_open_device / lv_sst_get_device on the GPU against the Python model
(tests/sst_get_cases.py), field for field: every case of the build's suite
with the image at several byte alignments, query counts around the wave and
the workgroup, a deep index, default options, long keys, every open status
and get corruption the CPU suite lists, the device chain from the memtable
build to the table get on one stream, graph capture."""
import numpy as np
import pytest

import lvgpu.memtable as MT
import lvgpu.table as T
import memtable_cases as M
import sst_build_cases as S
import sst_get_cases as G
from memtable_cases import MAX_SEQUENCE, make_table, tag

pytestmark = pytest.mark.gpu

CASES = S.cases()
SHIFTS = (0, 1, 5, 8, 15)


@pytest.mark.parametrize("name", list(CASES))
def test_cases(gpu, name):
    import torch
    items, bs, ri = CASES[name]
    payload, ops = make_table(items)
    image, _, _ = S.model_build(payload, ops, bs, ri)
    seen = G.check_image(torch, gpu, image, G.queries_for(image, payload, ops), shifts=SHIFTS, tag_=name)
    assert G.BAD_SEQ in seen and G.BAD_QUERY in seen and (not items or G.FOUND in seen or G.DELETED in seen)


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_query_counts(gpu, nq):
    import torch
    items, bs, ri = CASES["random_small_blocks"]
    payload, ops = make_table(items)
    image, _, _ = S.model_build(payload, ops, bs, ri)
    qs = G.queries_for(image, payload, ops)
    qs = [qs[(i * 7) % len(qs)] for i in range(nq)]
    op, owner, table = G.check_open(torch, gpu, image, shift=3)
    qk, off, ln, sq, bad = G.pack_queries(qs, bad_query=False)
    got = G.run_get(torch, gpu, op, qk, off, ln, sq)
    G.compare_results(got, G.model_results(image, table, qs, bad), f"nq={nq}")


def test_deep_index(gpu):
    """block_size 32 over 5 * SB_TILE + 3 entries: thousands of blocks, so the
    index binary search is deep and most probes of a wave differ."""
    import torch
    items = S.tile_items(5 * T.SB_TILE + 3)
    payload, ops = make_table(items)
    image, handles, _ = S.model_build(payload, ops, 32, 16)
    assert len(handles) > 2000
    qs = [(k, s) for k, t, _ in items for s in (t >> 8, MAX_SEQUENCE)]
    seen = G.check_image(torch, gpu, image, qs, shifts=(7,), tag_="deep index")
    assert seen >= {G.FOUND, G.DELETED}


def test_default_options_many_blocks(gpu):
    """The build suite's default-options table: ~6,000 entries, some 90 blocks
    of ~70 entries, restart runs of 16: all keys plus absent neighbours."""
    import torch
    rng = np.random.default_rng(3)
    items = [(k, t, v * 6) for k, t, v in M.random_items(rng, 6000, alphabet=4, maxlen=30, seqs=50)]
    payload, ops = make_table(items)
    image, handles, _ = S.model_build(payload, ops)
    assert len(handles) > 40
    qs = [(k, t >> 8) for k, t, _ in items]
    qs += [(k + b"\x00", MAX_SEQUENCE) for k, _, _ in items[::3]] + [(G.bump(k, 1), 40) for k, _, _ in items[::3] if k]
    seen = G.check_image(torch, gpu, image, qs, shifts=(2,), tag_="defaults")
    assert seen >= {G.FOUND, G.DELETED, G.ABSENT}


@pytest.mark.parametrize("bs", [4096, 1 << 16])
def test_one_long_key_for_every_entry(gpu, bs):
    """300 versions of one 4 KiB user key: every comparison runs 4,096 bytes
    into the tag; with 64 KiB blocks the scan shares all of them."""
    import torch
    key = bytes(range(256)) * 16
    items = [(key, tag(1000 - i, i % 2), b"v%d" % i) for i in range(300)]
    payload, ops = make_table(items)
    image, _, _ = S.model_build(payload, ops, bs, 16)
    qs = [(key, s) for s in range(695, 1003)] + [(key[:-1], 900), (key + b"\x00", 900), (key[:-1] + b"\x00", 900)]
    seen = G.check_image(torch, gpu, image, qs, shifts=(0, 3), tag_=f"long key bs={bs}")
    assert seen >= {G.FOUND, G.DELETED, G.ABSENT}


def test_long_shared_stem(gpu):
    import torch
    stem = (bytes(range(256)) * 20)[:4999]
    items = [(stem + bytes([c]), tag(10 + c), b"v%d" % c) for c in range(1, 40)] + [(stem, tag(5), b"stem")]
    payload, ops = make_table(items)
    for opt in ((4096, 16), (1 << 20, 1024)):
        image, _, _ = S.model_build(payload, ops, *opt)
        qs = [(k, s) for k, t, _ in items for s in ((t >> 8) - 1, t >> 8)] + [(stem[:2500] + b"\xff" + stem[2501:], 99)]
        G.check_image(torch, gpu, image, qs, shifts=(0, 9), tag_=f"stem {opt}")


DAMAGED = G.damaged_cases(200)


@pytest.mark.parametrize("group", ["open", "get", "flip"])
def test_damaged_images(gpu, group):
    """Every open status, every deterministic get corruption and 200 random
    flips: the inputs tools/sst_get_host_check.cc replays on the CPU under a
    sanitizer (python tests/sst_get_cases.py dump) before they run here.  Each
    image sits inside a larger tensor this test owns."""
    import torch
    seen, opens = set(), set()
    for name, image, kw, use, queries in DAMAGED:
        if not name.startswith(group + "/"):
            continue
        op, owner, table = G.check_open(torch, gpu, image, shift=5, tag_=name, **kw)
        opens.add(table["status"])
        if use != table:
            G.set_table(torch, op, use)
        seen |= G.Packed(image, use, queries).check(torch, gpu, op, name)
    if group == "open":
        assert opens >= {0, G.NOT_A_TABLE, G.BAD_FOOTER, G.BAD_INDEX, G.INDEX_SHAPE, G.HANDLE_OVER} and G.NO_TABLE in seen
    else:
        assert G.CORRUPT in seen and G.FOUND in seen


def test_upstream_file_cap_and_foreign_tables(gpu):
    import torch
    payload, ops, image, _ = G.base_image()
    queries = G.queries_for(image, payload, ops)[:40]
    _, _, t = G.check_open(torch, gpu, image, upstream=8, tag_="upstream")
    assert t["status"] == G.UPSTREAM and t["file_bytes"] == 0
    op, owner, t = G.check_open(torch, gpu, image, file_cap=len(image) - 1, tag_="file_cap")
    assert t["status"] == G.NOT_A_TABLE
    assert G.Packed(image, t, queries, file_cap=len(image) - 1).check(torch, gpu, op) == {G.NO_TABLE}
    # tables the open did not write for this file
    op, owner, sound = G.check_open(torch, gpu, image, shift=1)
    for patch in (dict(file_bytes=len(image) + 1), dict(index_offset=len(image)), dict(index_size=1 << 40),
                  dict(index_offset=(1 << 64) - 3), dict(index_offset=0, index_size=sound["index_offset"]),
                  dict(file_bytes=len(image) - 48)):
        use = dict(sound, **patch)
        G.set_table(torch, op, use)
        seen = G.Packed(image, use, queries, file_cap=len(image)).check(torch, gpu, op, str(patch))
        if "file_bytes" not in patch or patch["file_bytes"] > len(image):  # (a shorter file still holds the index)
            assert seen <= {G.NO_TABLE, G.CORRUPT, G.ABSENT, G.BAD_SEQ, G.BAD_QUERY}, (patch, seen)


def _table_against_memtable(payload, ops, file_host, got, mgot, queries):
    for i, (key, seq) in enumerate(queries):
        r, m = got[i], mgot[i]
        assert int(r["status"]) == int(m["status"]), (i, key, seq, r, m)
        if int(r["status"]) in (G.FOUND, G.DELETED):
            assert int(r["tag"]) == int(ops[int(m["op"])]["tag"]), (i, key, seq)
            vo, vl, mo = int(r["val_off"]), int(r["val_len"]), int(m["val_off"])
            assert vl == int(m["val_len"]) and file_host[vo:vo + vl] == payload[mo:mo + vl], (i, key, seq)


def test_chain_with_no_host_sync(gpu):
    """Memtable build -> SSTable build -> open -> verify -> table get ->
    memtable get on one stream, one synchronisation at the end.  The open reads
    file_bytes and the upstream status from the build's totals on the device."""
    import torch
    rng = np.random.default_rng(9)
    items = M.random_items(rng, 3000, alphabet=4, maxlen=20, seqs=30)
    payload, ops = make_table(items)
    queries = M.queries_for(payload, ops)[::3]
    qk, off, ln, sq = M.pack_queries(queries)
    d_pay = M.dev_bytes(torch, gpu, payload)[: len(payload)]
    d_ops = M.dev_bytes(torch, gpu, ops)
    d_n = M.dev_i64(torch, gpu, [len(ops)])
    dq = G.dev_queries(torch, gpu, qk, off, ln, sq)
    s = torch.cuda.Stream(device=gpu)
    for fail in (False, True):
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            table = MT.build_device(d_pay, d_ops, d_n, stream=s)
            built = T.build_device(table, block_size=512, stream=s, fill=G.CANARY, guard=G.GUARD,
                                   file_cap=100 if fail else None)
            op = T.open_device(built.file_t[: built.file_cap], built.totals[2:3], built.totals[7:8],
                               block_cap=built.block_cap, stream=s, fill=G.CANARY, guard=G.GUARD)
            st = T.verify_blocks(built.file_t[: built.file_cap], op.handles_t[: 2 * (op.block_cap + 2)], stream=s)
            gets = T.get_device(op, *dq, nq=len(queries), stream=s, fill=G.CANARY, guard=G.GUARD)
            mres = MT.get_device(table, *dq, nq=len(queries), stream=s)
        s.synchronize()
        got = gets.sync()
        if fail:
            assert built.sync_totals(check=False)["status"] == S.FILE_OVER
            t = op.sync(check=False)
            assert t == dict(dict.fromkeys(G.TABLE_FIELDS, 0), status=G.UPSTREAM)
            assert G.tail_is_canary(op.handles_t, 0)
            assert set(got["status"].tolist()) == {G.NO_TABLE} and not got["val_off"].any() and not got["tag"].any()
            continue
        want_file, want_handles = S.compare_device(built, payload, ops, 512, 16, "chain")
        assert op.sync() == G.model_open(want_file)[0]
        assert op.handles() == want_handles
        assert G.tail_is_canary(op.handles_t, 16 * len(want_handles))
        st = st.cpu().tolist()
        assert st[: len(want_handles)] == [T.BLOCK_OK] * len(want_handles)
        assert set(st[len(want_handles):]) <= {T.BLOCK_OUT_OF_RANGE}
        _table_against_memtable(payload, ops, want_file, got, MT.results(mres, len(queries)), queries)
        assert {G.FOUND, G.DELETED, G.ABSENT} <= set(got["status"].tolist())


def test_graph_capture(gpu):
    """Open + get captured into one graph after a warm-up call; three replays
    over different images of one capacity, the results and the handles filled
    with the canary again between replays."""
    import torch
    sets = []
    for seed, n in ((1, 700), (2, 90), (3, 400)):
        items = S.tile_items(n, seed=seed)
        payload, ops = make_table(items)
        image, _, _ = S.model_build(payload, ops, 64, 4)
        table, handles = G.model_open(image)
        queries = G.queries_for(image, payload, ops)[:1200]
        sets.append((image, table, handles, G.Packed(image, table, queries)))
    fcap = max(len(s[0]) for s in sets) + 13
    bcap = max(s[1]["data_blocks"] for s in sets)
    nq = min(len(s[3].wants) for s in sets) - 1  # without the BAD_QUERY one: qkeys_bytes is the capacity here
    qbytes = max(len(s[3].arrays[0]) for s in sets)
    buf = torch.full((fcap + 32,), G.CANARY, dtype=torch.uint8, device=gpu)
    file_t = buf[3:3 + fcap]
    d_fb = torch.zeros(1, dtype=torch.int64, device=gpu)
    d_qk = torch.zeros(qbytes, dtype=torch.uint8, device=gpu)
    d_off = torch.zeros(nq, dtype=torch.int64, device=gpu)
    d_len = torch.zeros(nq, dtype=torch.int32, device=gpu)
    d_seq = torch.zeros(nq, dtype=torch.int64, device=gpu)

    def load(k):
        image, _, _, packed = sets[k]
        qk, off, ln, sq, _ = packed.arrays
        buf.fill_(G.CANARY)
        file_t[: len(image)].copy_(torch.frombuffer(bytearray(image), dtype=torch.uint8))
        d_fb.fill_(len(image))
        d_qk[: len(qk)].copy_(torch.frombuffer(bytearray(qk), dtype=torch.uint8))
        d_off.copy_(torch.from_numpy(off[:nq].view(np.int64).copy()))
        d_len.copy_(torch.from_numpy(np.ascontiguousarray(ln[:nq]).view(np.int32).copy()))
        d_seq.copy_(torch.from_numpy(sq[:nq].view(np.int64).copy()))

    def run(stream=None, op=None, gets=None):
        op = T.open_device(file_t, d_fb, block_cap=bcap, stream=stream, fill=G.CANARY, guard=G.GUARD,
                           table=op.table if op else None, handles_t=op.handles_t if op else None)
        return op, T.get_device(op, d_qk, d_off, d_len, d_seq, nq=nq, stream=stream, fill=G.CANARY, guard=G.GUARD,
                                res=gets.res if gets else None)

    def verify(k, op, gets, what):
        _, table, handles, packed = sets[k]
        torch.cuda.synchronize()
        fresh = T.Opened(op.file_t, op.file_cap, op.table, op.handles_t, op.block_cap, None)
        assert fresh.sync() == table, (what, fresh.sync(), table)
        assert fresh.handles() == handles, what
        assert G.tail_is_canary(op.handles_t, 16 * len(handles)), what
        G.compare_results(T.Gets(gets.res, nq, None).sync(), packed.wants[:nq], what)
        assert G.tail_is_canary(gets.res, 32 * nq), what

    load(0)
    op, gets = run()
    verify(0, op, gets, "warm")
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            run(s, op, gets)
    torch.cuda.synchronize()
    for k in (1, 2, 0):
        load(k)
        op.handles_t.view(torch.uint8).fill_(G.CANARY)
        gets.res.fill_(G.CANARY)
        op.table.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        verify(k, op, gets, f"replay of set {k}")
