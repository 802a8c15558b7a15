"""lv_compact_filter_device on the GPU against the Python model
(tests/compact_cases.py), field for field with every canary checked (around
d_order_out, [kept, op_cap) included, and around both totals): every CPU case
at all payload alignments, entry counts around the wave and the scan tile with
groups across every boundary and a tile that is dropped whole, long keys,
op_cap above the entries, every status; then, without the model, the
compaction invariant on one stream (scan, sort, filter, build, open, get
against the unfiltered memtable), the block checksums of the compacted image
and graph capture."""
import numpy as np
import pytest

import compact_cases as C
import lvgpu.compact as CP
import lvgpu.memtable as MT
import lvgpu.table as T
import memtable_cases as M
import sst_build_cases as S
import sst_get_cases as G
import sst_scan_cases as SC
from compact_cases import BASE_LEVEL
from memtable_cases import make_table, tag
from write_batch_cases import CANARY, GUARD, tail_is_canary

pytestmark = pytest.mark.gpu

CASES = C.cases()
TILE = CP.CF_TILE


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_cases(gpu, name):
    import torch
    items, gaps, settings = CASES[name]
    payload, ops, order, mt = C.table_of(items, gaps)
    shifts = range(8) if name in ("alignments", "key_lengths") else (0, 5)
    for S_, flags, ranges in settings:
        for shift in shifts:
            _, want = C.check_device(torch, gpu, payload, ops, order, mt, S_, ranges, flags, shift=shift,
                                     tag_=(name, S_, flags, shift))
            assert want[0]["status"] == 0


@pytest.mark.parametrize("n", [63, 64, 65, TILE - 1, TILE, TILE + 1, 5 * TILE + 3])
def test_wave_and_tile_boundaries(gpu, n):
    """Groups of versions across every wave and tile boundary (an entry's
    predecessor is another wave's or another workgroup's) and, from three
    tiles on, a group that covers the second tile whole: above its sequences
    that tile keeps nothing."""
    import torch
    payload, ops, order, mt = C.table_of(C.boundary_items(n, TILE))
    assert order.tolist() == list(range(n))  # the boundaries are where the generator put them
    for S_ in (0, 6, 19, 10 ** 6):
        for flags in (0, BASE_LEVEL):
            _, want = C.check_device(torch, gpu, payload, ops, order, mt, S_, None, flags, shift=n % 8, tag_=(n, S_, flags))
            if S_ == 10 ** 6 and n > 2 * TILE:
                kept = np.array(want[2])
                assert not ((kept >= TILE) & (kept < 2 * TILE)).any() and want[0]["dropped_hidden"] > TILE


def test_long_keys(gpu):
    """300 versions of one 4 KiB key; two 4 KiB keys that differ in the last
    byte only."""
    import torch
    key = bytes(range(256)) * 16
    one = [(key, tag(1000 - i, i % 5 != 4), b"" if i % 5 == 4 else b"v") for i in range(300)]
    two = [(key[:-1] + b"\x01", tag(7), b"a"), (key[:-1] + b"\x02", tag(6), b"b"), (key[:-1] + b"\x02", tag(5, 0), b"")]
    for items in (one, two, one + two):
        payload, ops, order, mt = C.table_of(items)
        for S_ in (3, 850, 2000):
            for shift in (0, 3):
                _, want = C.check_device(torch, gpu, payload, ops, order, mt, S_, None, BASE_LEVEL, shift=shift, tag_=S_)
        assert want[0]["kept"] == (1 if items is one else 2 if items is two else 3)


def test_op_cap_above_the_entries_and_no_entries(gpu):
    import torch
    items, gaps, _ = CASES["deletions"]
    payload, ops, order, mt = C.table_of(items, gaps)
    for cap in (len(ops) + 1, 3 * TILE + 1):
        C.check_device(torch, gpu, payload, ops, order, mt, 5, None, BASE_LEVEL, op_cap=cap, tag_=cap)
    empty = C.table_of([])
    for cap in (1, TILE + 1):
        _, want = C.check_device(torch, gpu, empty[0], empty[1], empty[2], empty[3], 5, None, BASE_LEVEL, op_cap=cap)
        assert want[0] == dict.fromkeys(C.TOTALS, 0) and want[1] == dict(entries=0, user_keys=0, status=0)
    # op_cap == 0: no d_ops, d_order or d_order_out at all
    t = C.device_table(torch, gpu, b"", empty[1], empty[2], empty[3], op_cap=1)
    f = CP.filter_device(t, 5, None, BASE_LEVEL, op_cap=0, fill=CANARY, guard=GUARD)
    assert f.sync() == dict.fromkeys(C.TOTALS, 0) and tail_is_canary(f.order_t, 0)


@pytest.mark.parametrize("name", list(C.status_cases()))
def test_statuses_leave_the_order_untouched(gpu, name):
    import torch
    kw, status = C.status_cases()[name]
    kw = dict(kw)
    f, want = C.check_device(torch, gpu, kw.pop("payload"), kw.pop("ops"), kw.pop("order"), kw.pop("mt"), kw.pop("S"),
                             kw.pop("ranges"), kw.pop("flags"), shift=3, tag_=name, **kw)
    assert want[0]["status"] == status
    if status:
        assert tail_is_canary(f.order_t, 0) and want[1] == C.NO_TABLE
        built = T.build_device(f, fill=CANARY, guard=GUARD)  # the consumers refuse it
        assert built.sync_totals(check=False)["status"] == S.NO_TABLE and tail_is_canary(built.file_t, 0)


def test_a_bad_index_in_a_later_tile(gpu):
    """The bad entry is in the third tile: the first two tiles' counts go
    nowhere and nothing is written."""
    import torch
    payload, ops, order, mt = C.table_of(C.boundary_items(3 * TILE, TILE))
    for at in (2 * TILE, 3 * TILE - 1):
        bad = order.copy()
        bad[at] = len(ops)
        f, want = C.check_device(torch, gpu, payload, ops, bad, mt, 6, None, BASE_LEVEL, tag_=at)
        assert want[0]["status"] == C.BAD_INPUT and tail_is_canary(f.order_t, 0)


# ---- the invariant: a compaction changes no answer at or above the snapshot ----
def _three_tables():
    """Three tables with overlapping keys, sequences 1-30 in all: values,
    deletions, overwritten and re-created keys, an exact duplicate."""
    rng = np.random.default_rng(31)
    keys = [b"k%02d" % i for i in range(12)] + [b"k0", b"k00", b"", b"long" * 30, b"long" * 30 + b"!"]
    parts, seq = [], 1
    for t in range(3):
        items = []
        for _ in range(10):
            k = keys[int(rng.integers(len(keys)))]
            typ = 0 if rng.random() < 0.35 else 1
            items.append((k, tag(seq, typ), b"" if typ == 0 else b"t%d-s%d" % (t, seq)))
            seq += 1
        parts.append(items)
    parts[2].append(parts[2][0])  # an exact duplicate
    return parts, keys, seq - 1


def _chain(torch, gpu, parts, S_, flags, ranges, stream):
    """scan (appended) -> memtable build -> filter -> table build -> open, on
    one stream with no synchronisation: (memtable, Filtered, Built, Opened)."""
    images = [S.model_build(*make_table(items), 64, 4)[0] for items in parts]
    tabs = [SC.open_table(img) for img in images]
    fulls = [SC.model_scan(img, t)[0] for img, t in zip(images, tabs)]
    acap, ocap = sum(f["table_bytes"] for f in fulls), sum(f["table_entries"] for f in fulls)
    bcap = max(t["data_blocks"] for t in tabs)
    prev, owners = None, []
    with torch.cuda.stream(stream):
        for i, img in enumerate(images):
            op, owner = SC.open_on(torch, gpu, img, shift=i, stream=stream)
            owners.append(owner)
            prev = SC.run_scan(torch, gpu, op, prev, arena_cap=acap, op_cap=ocap, block_cap=bcap, arena_shift=3, stream=stream)
        table = MT.build_device(prev.arena_t[: prev.arena_cap], prev.ops_t, prev.totals[0:1], prev.totals[7:8],
                                op_cap=prev.op_cap, stream=stream, fill=CANARY, guard=GUARD)
        f = CP.filter_device(table, S_, ranges, flags, stream=stream, fill=CANARY, guard=GUARD)
        built = T.build_device(f, block_size=64, restart_interval=4, stream=stream, fill=CANARY, guard=GUARD)
        opened = T.open_device(built.file_t[: built.file_cap], built.totals[2:3], built.totals[7:8],
                               block_cap=built.block_cap, stream=stream)
    return table, f, built, opened, (prev, owners)


@pytest.mark.parametrize("flags", [0, BASE_LEVEL])
def test_the_invariant_on_one_stream(gpu, flags):
    """For every user key and every snapshot in [S, the highest sequence + 1]
    the get over the compacted table is the get over the unfiltered memtable:
    the same status and the same value bytes.  With LV_COMPACT_BASE_LEVEL (and
    no deeper level) a dropped deletion answers ABSENT where the memtable
    answers DELETED; nothing else may differ."""
    import torch
    parts, keys, top = _three_tables()
    s = torch.cuda.Stream(device=gpu)
    dropped, seen = 0, set()
    for S_ in (0, 7, 15, 22, top, top + 1):
        queries = [(k + x, q) for k in keys for x in (b"", b"\x00") for q in range(S_, top + 2)]
        qk, off, ln, sq = M.pack_queries(queries)
        dq = G.dev_queries(torch, gpu, qk, off, ln, sq)
        torch.cuda.synchronize()
        table, f, built, opened, keep = _chain(torch, gpu, parts, S_, flags, None, s)
        with torch.cuda.stream(s):
            gets = T.get_device(opened, *dq, nq=len(queries), stream=s)
            mres = MT.get_device(table, *dq, nq=len(queries), stream=s)
            st = T.verify_blocks(built.file_t[: built.file_cap], built.handles_t[: 2 * (built.block_cap + 2)], stream=s)
        s.synchronize()
        tot = f.sync()
        assert tot["entries_in"] == sum(len(p) for p in parts) and tot["status"] == 0
        dropped += tot["dropped_hidden"] + tot["dropped_deletions"]
        assert built.sync_totals()["entries"] == tot["kept"] and opened.sync()["status"] == 0
        nh = built.sync_totals()["data_blocks"] + 2
        assert st.cpu().tolist()[:nh] == [T.BLOCK_OK] * nh  # lv_sst_verify_blocks_device over the compacted image
        g, m = gets.sync(), MT.results(mres, len(queries))
        file_, arena = built.file(), table.payload.cpu().numpy().tobytes()
        for (k, q), a, b in zip(queries, g, m):
            sa, sb = int(a["status"]), int(b["status"])
            seen.add(sb)
            if flags and sb == M.DELETED:
                assert sa in (G.DELETED, G.ABSENT), (S_, k, q, sa)
            else:
                assert sa == sb, (S_, k, q, sa, sb)
            if sb == M.FOUND:
                va, vb = int(a["val_off"]), int(b["val_off"])
                assert int(a["val_len"]) == int(b["val_len"])
                assert file_[va:va + int(a["val_len"])] == arena[vb:vb + int(b["val_len"])], (S_, k, q)
    assert seen == {M.ABSENT, M.FOUND, M.DELETED} and dropped > 0, (seen, dropped)


def test_graph_capture(gpu):
    """Open + scan + memtable build + filter + table build captured once after
    a warm-up; the replay runs over a second input of the same capacities and
    writes the model's image of the model's kept entries."""
    import torch
    sets = []
    for seed, n in ((1, 500), (2, 380)):
        rng = np.random.default_rng(seed)
        items = M.random_items(rng, n, alphabet=3, maxlen=6, seqs=20)
        payload, ops = make_table(items)
        image = S.model_build(payload, ops, 256, 8)[0]
        items = [items[i] for i in M.model_order(payload, ops)]  # what the scan hands on: the image's order
        payload, ops, order, mt = C.table_of(items)
        kept = C.model_filter(payload, ops, order, mt, 9, None, BASE_LEVEL)
        want = S.model_build(*make_table([items[i] for i in sorted(kept[2])]), 512, 16)[0]
        sets.append((image, SC.open_table(image), kept[0], want))
    fcap = max(len(x[0]) for x in sets) + 13
    bcap = max(x[1]["data_blocks"] for x in sets)
    fulls = [SC.model_scan(img, t)[0] for img, t, _, _ in sets]
    acap, ocap = max(f["table_bytes"] for f in fulls), max(f["table_entries"] for f in fulls)
    buf = torch.full((fcap + 32,), CANARY, dtype=torch.uint8, device=gpu)
    file_t = buf[3:3 + fcap]
    d_fb = torch.zeros(1, dtype=torch.int64, device=gpu)

    def load(k):
        image = sets[k][0]
        buf.fill_(CANARY)
        file_t[: len(image)].copy_(torch.frombuffer(bytearray(image), dtype=torch.uint8))
        d_fb.fill_(len(image))

    def run(stream=None):
        op = T.open_device(file_t, d_fb, block_cap=bcap, stream=stream)
        sc = T.scan_device(op, arena_cap=acap, op_cap=ocap, block_cap=bcap, stream=stream)
        table = MT.build_device(sc.arena_t[:acap], sc.ops_t, sc.totals[0:1], sc.totals[7:8], op_cap=ocap, stream=stream)
        f = CP.filter_device(table, 9, None, BASE_LEVEL, stream=stream, fill=CANARY, guard=GUARD)
        built = T.build_device(f, block_size=512, restart_interval=16, stream=stream, fill=CANARY, guard=GUARD)
        return op, sc, table, f, built

    def verify(k, out, what):
        torch.cuda.synchronize()
        _, _, _, f, built = out
        tot = dict(zip(C.TOTALS, (int(v) for v in f.compact_totals.cpu().numpy().view(np.uint64))))
        assert tot == sets[k][2], (what, tot, sets[k][2])
        n = int(built.totals.cpu().numpy().view(np.uint64)[2])
        assert built.file_t[:n].cpu().numpy().tobytes() == sets[k][3], what
        assert tail_is_canary(built.file_t, n) and tail_is_canary(f.order_t, 4 * tot["kept"]), what

    load(0)
    verify(0, run(), "warm-up")  # the device is initialised
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        out = run(s)
    for k in (1, 0):
        load(k)
        g.replay()
        verify(k, out, f"replay {k}")
