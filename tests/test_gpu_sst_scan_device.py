"""lv_sst_scan_device on the GPU against the Python model
(tests/sst_scan_cases.py), field for field and byte for byte with every canary
checked: every case of the build's suite at several alignments of the file and
the arena, run and block counts around the scan tile, one block of many
entries, lengths around the cooperative-copy threshold, many versions of one
long key, prefixes that cross between key and tag, the damaged images, every
status with the retry, appending, the device chains on one stream, graph
capture."""
import numpy as np
import pytest

import lvgpu.memtable as MT
import lvgpu.table as T
import memtable_cases as M
import sst_build_cases as S
import sst_get_cases as G
import sst_scan_cases as C
from memtable_cases import make_table, tag
from write_batch_cases import CANARY, GUARD

pytestmark = pytest.mark.gpu

CASES = S.cases()
TILE = T.SS_TILE
W = T.SS_WAVE_COPY


def image_of(items, bs, ri):
    payload, ops = make_table(items)
    return payload, ops, S.model_build(payload, ops, bs, ri)[0]


@pytest.mark.parametrize("name", list(CASES))
def test_cases(gpu, name):
    import torch
    items, bs, ri = CASES[name]
    for b in (bs, 1):
        _, ops, image = image_of(items, b, ri)
        for shift, ashift in zip((0, 1, 5, 8, 15), (0, 3, 9, 3, 0)):
            sc, want = C.check_image(torch, gpu, image, shift=shift, arena_shift=ashift, tag_=(name, b, shift))
            assert want[0]["status"] == 0 and want[0]["table_entries"] == len(ops) and want[3]["status"] == 0


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 5 * TILE + 3])
def test_run_and_block_counts_around_the_tile(gpu, n):
    """restart_interval 1: runs equal entries; block_size 32: one to three
    entries a block, so the block scan crosses its tile too."""
    import torch
    _, ops, image = image_of(S.tile_items(n), 32, 1)
    for slack in (1, 4):
        sc, want = C.check_image(torch, gpu, image, shift=5, arena_shift=3, slack=slack, tag_=(n, slack))
        assert want[0]["status"] == 0 and want[0]["runs"] == n == want[0]["table_entries"]
        assert n <= TILE + 1 or want[0]["data_blocks"] > TILE


@pytest.mark.parametrize("ri", [1, 2, 16, 1024])
def test_one_block_of_2000_entries(gpu, ri):
    import torch
    _, ops, image = image_of(S.tile_items(2000, seed=ri), 1 << 20, ri)
    sc, want = C.check_image(torch, gpu, image, shift=1, tag_=ri)
    assert want[0]["data_blocks"] == 1 and want[0]["runs"] == -(-2000 // ri) and want[0]["table_entries"] == 2000


def test_lengths_around_the_copy_threshold(gpu):
    """Key suffixes, shared prefixes and values of W - 1, W, W + 1 and 16 W
    bytes, at six alignments of the source and of the arena."""
    import torch
    items = []
    for i, n in enumerate((W - 1, W, W + 1, 16 * W)):
        stem = bytes([65 + i]) * n
        items += [(stem, tag(9), b"v" * n), (stem + b"a", tag(8), b""), (stem + b"b" * n, tag(7), b"w" * (n + 1)),
                  (stem + b"b" * n + b"c", tag(6, 0), b"")]
    for ri in (16, 1):
        _, ops, image = image_of(items, 4096, ri)
        for shift, ashift in ((0, 0), (1, 15), (7, 1), (8, 8), (13, 4), (15, 9)):
            C.check_image(torch, gpu, image, shift=shift, arena_shift=ashift, tag_=(ri, shift, ashift))


@pytest.mark.parametrize("bs", [4096, 65536])
def test_300_versions_of_one_4k_key(gpu, bs):
    """Every entry's key comes almost entirely from the lane's own previous
    arena write."""
    import torch
    key = bytes(range(256)) * 16
    items = [(key, tag(1000 - i, i % 5 != 0), b"v%d" % i if i % 5 else b"") for i in range(300)]
    _, ops, image = image_of(items, bs, 16)
    sc, want = C.check_image(torch, gpu, image, shift=3, arena_shift=5, tag_=bs)
    assert want[0]["table_bytes"] > 300 * 4096 and want[3]["user_keys"] == 1


@pytest.mark.parametrize("name", ["tag_into_key", "tag_high_byte"])
def test_prefixes_across_key_and_tag(gpu, name):
    import torch
    for ri in (16, 1):
        _, ops, image = image_of(CASES[name][0], 4096, ri)
        for ashift in (0, 3, 9):
            C.check_image(torch, gpu, image, shift=ashift, arena_shift=ashift, tag_=(name, ri))


def test_damaged_images_and_flips(gpu):
    import torch
    seen, ok, bad = set(), 0, 0
    for name, image, table in C.damaged_cases():
        opened = C.open_table(image)
        use = None if table == opened else table
        _, want = C.check_image(torch, gpu, image, table=use, shift=5, arena_shift=3, tag_=name,
                                caps=(1 << 16, 2048, 256))
        st, mst = want[0]["status"], want[3]["status"]
        seen |= {st, ("mt", mst)}
        if name.startswith("flip/"):
            ok += st == 0
            bad += st == C.CORRUPT
    assert seen >= {0, C.NO_TABLE, C.CORRUPT, ("mt", 0), ("mt", C.MT_UNORDERED), ("mt", C.MT_UPSTREAM)}
    assert ok >= 20 and bad >= 20, (ok, bad)


def test_every_status_and_the_retry(gpu):
    import torch
    _, ops, image = image_of(*CASES["random_small_blocks"])
    table = C.open_table(image)
    full = C.model_scan(image, table)[0]
    ne, nb, nblk = full["table_entries"], full["table_bytes"], full["data_blocks"]
    sts = {}
    for caps in ((nb, ne - 1, nblk), (nb - 1, ne, nblk), (nb, ne, nblk - 1), (0, 0, nblk), (nb, ne, 0), (0, 0, 0),
                 (nb, 3, nblk), (nb, ne, nblk)):
        sc, want = C.check_image(torch, gpu, image, caps=caps, shift=1, tag_=caps)
        sts[caps] = want[0]["status"]
        if want[0]["status"] in (C.OP_OVER, C.ARENA_OVER, C.OP_OVER | C.ARENA_OVER):  # the retry
            got = sc.sync(check=False)
            _, again = C.check_image(torch, gpu, image, caps=(got["arena_bytes"], got["entries"], nblk))
            assert again[0]["status"] == 0
    assert list(sts.values()) == [C.OP_OVER, C.ARENA_OVER, C.BLOCK_OVER, C.OP_OVER | C.ARENA_OVER, C.BLOCK_OVER,
                                  C.BLOCK_OVER, C.OP_OVER, 0]
    # NO_TABLE: each open status, and a file_cap below the table's file_bytes
    for name, (bad, kw, st) in G.open_cases().items():
        if st and not kw:
            _, want = C.check_image(torch, gpu, bad, caps=(64, 4, 4), tag_=name)
            assert want[0]["status"] == C.NO_TABLE
    _, want = C.check_image(torch, gpu, image, table=dict(table, file_bytes=len(image) + 1), caps=(nb, ne, nblk))
    assert want[0]["status"] == C.NO_TABLE
    # the empty table
    _, want = C.check_image(torch, gpu, b"", caps=(16, 2, 2))
    assert want[0] == dict.fromkeys(C.TOTALS, 0) and want[3] == dict(entries=0, user_keys=0, status=0)
    # foreign tables
    base = G.base_image()[2]
    for t in C.foreign_tables(base):
        _, want = C.check_image(torch, gpu, base, table=t, caps=(4096, 64, 64), shift=1, tag_=str(t))


def _append(torch, gpu, parts, stream=None, fail_at=None):
    """Scans the images of `parts` one behind the other: (last Scanned, the
    model's ops and arena so far, every Scanned)."""
    tabs = [C.open_table(img) for img in parts]
    fulls = [C.model_scan(img, t)[0] for img, t in zip(parts, tabs)]
    acap = sum(f["table_bytes"] for f in fulls)
    ocap = sum(f["table_entries"] for f in fulls)
    bcap = max(t["data_blocks"] for t in tabs) or 1
    prev, pw, sofar, scs = None, None, ([], b""), []
    for i, (img, t) in enumerate(zip(parts, tabs)):
        use = dict(t, status=G.BAD_INDEX) if i == fail_at else None
        op, owner = C.open_on(torch, gpu, img, shift=i, table=use, stream=stream)
        want = C.model_scan(img, use or t, pw, arena_cap=acap, op_cap=ocap, block_cap=bcap, file_cap=len(img))
        sc = C.run_scan(torch, gpu, op, prev, arena_cap=acap, op_cap=ocap, block_cap=bcap, arena_shift=3, stream=stream)
        sc._owner = owner
        scs.append((sc, want, sofar))
        if not want[0]["status"]:
            sofar = (sofar[0] + want[1], sofar[1] + want[2])
        prev, pw = sc, want[0]
    return prev, sofar, scs


def test_appending_three_tables_then_sort_and_build(gpu):
    """Three scans into one arena, lv_memtable_build_device over the union and
    lv_sst_build_device over that, on one stream with no synchronisation in
    between: a major compaction that drops nothing."""
    import torch
    names = ["tags", "corner_keys", "duplicates"]  # (see test_sst_scan.py on duplicates)
    parts = [image_of(*CASES[n])[2] for n in names]
    items = [it for n in names for it in CASES[n][0]]
    s = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        last, sofar, scs = _append(torch, gpu, parts, stream=s)
        table = MT.build_device(last.arena_t[: last.arena_cap], last.ops_t, last.totals[0:1], last.totals[7:8],
                                op_cap=last.op_cap, stream=s, fill=CANARY, guard=GUARD)
        built = T.build_device(table, block_size=256, restart_interval=8, stream=s, fill=CANARY, guard=GUARD)
        st = T.verify_blocks(built.file_t[: built.file_cap], built.handles_t[: 2 * (built.block_cap + 2)], stream=s)
    s.synchronize()
    C.check_scan(last, scs[-1][1], prev_want=scs[-1][2], tag_="append")
    assert last.sync()["entries"] == len(items)
    payload, ops = make_table(items)
    want_file, want_handles, _ = S.model_build(payload, ops, 256, 8)
    assert built.file() == want_file and built.handles() == want_handles
    st = st.cpu().tolist()
    assert st[: len(want_handles)] == [T.BLOCK_OK] * len(want_handles)


def test_a_failing_append_reaches_the_last_totals(gpu):
    import torch
    parts = [image_of(*CASES[n])[2] for n in ("tags", "corner_keys", "duplicates")]
    last, sofar, scs = _append(torch, gpu, parts, fail_at=1)
    sts = [w[0]["status"] for _, w, _ in scs]
    assert sts == [0, C.NO_TABLE, C.UPSTREAM]
    for sc, want, before in scs:
        assert sc.sync(check=False) == want[0]
    C.check_scan(last, scs[-1][1], prev_want=sofar, tag_="failing append")  # only the first table's entries
    table = MT.build_device(last.arena_t[: last.arena_cap], last.ops_t, last.totals[0:1], last.totals[7:8],
                            op_cap=last.op_cap, fill=CANARY, guard=GUARD)
    assert table.sync_totals(check=False)["status"] == M.UPSTREAM and M.untouched(table)


def test_chain_rewrite_with_other_options(gpu):
    """Memtable build -> table build -> open -> scan with d_order -> table
    build with other options -> open -> get, one stream, one synchronisation.
    The second image is the model's; its gets are the first table's but for
    val_off and block."""
    import torch
    rng = np.random.default_rng(12)
    items = M.random_items(rng, 2500, alphabet=4, maxlen=20, seqs=30)
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
            built = T.build_device(table, block_size=512, stream=s, file_cap=100 if fail else None)
            op = T.open_device(built.file_t[: built.file_cap], built.totals[2:3], built.totals[7:8],
                               block_cap=built.block_cap, stream=s)
            gets1 = T.get_device(op, *dq, nq=len(queries), stream=s)
            sc = T.scan_device(op, arena_cap=len(payload), op_cap=len(ops), order=True, stream=s, fill=CANARY, guard=GUARD)
            built2 = T.build_device(sc.memtable(), block_size=3000, restart_interval=5, stream=s, fill=CANARY, guard=GUARD)
            op2 = T.open_device(built2.file_t[: built2.file_cap], built2.totals[2:3], built2.totals[7:8],
                                block_cap=built2.block_cap, stream=s)
            gets2 = T.get_device(op2, *dq, nq=len(queries), stream=s)
            mres = MT.get_device(sc.memtable(), *dq, nq=len(queries), stream=s)
        s.synchronize()
        g1, g2, gm = gets1.sync(), gets2.sync(), MT.results(mres, len(queries))
        if fail:  # the upstream status reaches the last totals and nothing is written
            assert sc.sync(check=False)["status"] == C.NO_TABLE and sc.mt() == dict(entries=0, user_keys=0, status=1)
            assert G.tail_is_canary(sc.arena_t, 0) and G.tail_is_canary(sc.ops_t, 0) and G.tail_is_canary(sc.order_t, 0)
            assert built2.sync_totals(check=False)["status"] == S.NO_TABLE and G.tail_is_canary(built2.file_t, 0)
            assert op2.sync(check=False)["status"] == G.UPSTREAM
            assert set(g2["status"].tolist()) == {G.NO_TABLE} and set(gm["status"].tolist()) == {M.NO_TABLE}
            continue
        assert sc.sync()["table_entries"] == len(ops) and sc.mt() == M.model_totals(payload, ops)[1]
        assert built2.file() == S.model_build(payload, ops, 3000, 5)[0]
        for f in ("tag", "val_len", "status", "reserved"):
            assert (g1[f] == g2[f]).all(), f
        assert (g1["status"] == gm["status"]).all() and {G.FOUND, G.DELETED, G.ABSENT} <= set(g2["status"].tolist())
        file2 = built2.file()
        arena = sc.arena()
        for r, m in zip(g2, gm):
            if int(r["status"]) == G.FOUND:
                vo, vl, mo = int(r["val_off"]), int(r["val_len"]), int(m["val_off"])
                assert file2[vo:vo + vl] == arena[mo:mo + vl]


def test_graph_capture(gpu):
    """Open + scan captured into one graph after a warm-up call; three replays
    over different images of one capacity, the outputs filled with the canary
    again between replays."""
    import torch
    sets = []
    for seed, n in ((1, 700), (2, 90), (3, 400)):
        _, ops, image = image_of(S.tile_items(n, seed=seed), 64, 4)
        sets.append((image, C.open_table(image)))
    fcap = max(len(s[0]) for s in sets) + 13
    bcap = max(s[1]["data_blocks"] for s in sets)
    fulls = [C.model_scan(img, t, order=True) for img, t in sets]
    acap, ocap = max(f[0]["table_bytes"] for f in fulls), max(f[0]["table_entries"] for f in fulls)
    buf = torch.full((fcap + 32,), CANARY, dtype=torch.uint8, device=gpu)
    file_t = buf[3:3 + fcap]
    d_fb = torch.zeros(1, dtype=torch.int64, device=gpu)

    def load(k):
        image = sets[k][0]
        buf.fill_(CANARY)
        file_t[: len(image)].copy_(torch.frombuffer(bytearray(image), dtype=torch.uint8))
        d_fb.fill_(len(image))

    def run(stream=None, op=None, sc=None):
        op = T.open_device(file_t, d_fb, block_cap=bcap, stream=stream, fill=CANARY, guard=GUARD,
                           table=op.table if op else None, handles_t=op.handles_t if op else None)
        kw = dict(arena_t=sc.arena_t, ops_t=sc.ops_t, order_t=sc.order_t, mt_totals=sc.mt_totals, totals=sc.totals) if sc else {}
        ws = sc._ws if sc else torch.full((T.scan_workspace_bytes(ocap, bcap),), 0x5A, dtype=torch.uint8, device=gpu)
        out = T.scan_device(op, arena_cap=acap, op_cap=ocap, block_cap=bcap, order=True, workspace=ws, stream=stream,
                            fill=CANARY, guard=GUARD, **kw)
        out._ws = ws
        return op, out

    def verify(k, sc, what):
        torch.cuda.synchronize()
        wt, wops, warena, wmt = fulls[k]
        fresh = T.Scanned(sc.arena_t, acap, sc.ops_t, ocap, bcap, sc.totals, sc.order_t, sc.mt_totals, None)
        assert fresh.sync() == wt, (what, k)
        assert fresh.arena() == warena and (fresh.ops() == C.ops_array(wops)).all() and fresh.mt() == wmt, (what, k)
        assert G.tail_is_canary(sc.arena_t, len(warena)) and G.tail_is_canary(sc.ops_t, 32 * len(wops)), (what, k)
        assert G.tail_is_canary(sc.order_t, 4 * len(wops)), (what, k)

    load(0)
    op, sc = run()  # the warm-up: the device is initialised
    verify(0, sc, "warm-up")
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        run(s, op, sc)
    for k in (1, 2, 0):
        load(k)
        for t in (sc.arena_t, sc.ops_t, sc.order_t):
            t.view(torch.uint8).fill_(CANARY)
        g.replay()
        verify(k, sc, "replay")
