"""lv_sst_build_device on the GPU against the Python model
(tests/sst_build_cases.py), byte for byte: every case of the CPU suite, entry
counts around the scan tile with block chains that cross its edges, values and
keys around the wave-copy threshold at every alignment, every status with
nothing written, lv_sst_verify_blocks_device over the result, the device chain
from the memtable build on one stream, graph capture."""
import numpy as np
import pytest

import lvgpu.memtable as MT
import lvgpu.table as T
import memtable_cases as M
import sst_build_cases as C
from memtable_cases import make_table, tag

pytestmark = pytest.mark.gpu

TILE = T.SB_TILE
W = T.SB_WAVE_COPY
CASES = C.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_cases(gpu, name):
    import torch
    items, bs, ri = CASES[name]
    built, payload, ops = C.check_device(torch, gpu, items, bs, ri, shift=3, tag_=name)
    if items:  # the project's own verify accepts every trailer
        st = T.verify_blocks(built.file_t[: built.sync_totals()["file_bytes"]], built.handles_view())
        assert st.cpu().tolist() == [T.BLOCK_OK] * (built.sync_totals()["data_blocks"] + 2)


@pytest.mark.parametrize("ri", [1, 2, 16])
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 5 * TILE + 3])
def test_tile_and_chain_structure(gpu, n, ri):
    """block_size 32: a block holds one to three entries, so the chain of
    block starts crosses every tile edge where the data puts it; op_cap four
    times the count: surplus doubling passes and tiles run and exit."""
    import torch
    items = C.tile_items(n, seed=ri)
    C.check_device(torch, gpu, items, 32, ri, tag_=f"n={n} ri={ri}")
    built, _, _ = C.check_device(torch, gpu, items, 32, ri, op_cap=4 * n, tag_=f"n={n} ri={ri} op_cap 4n")
    assert built.sync_totals()["data_blocks"] > n // 4


def test_default_options_many_blocks(gpu):
    """Defaults (a NULL opt): ~6,000 entries of ~60 bytes, some 90 blocks of
    ~70 entries, restart runs of 16 cut by the block ends."""
    import torch
    rng = np.random.default_rng(3)
    items = M.random_items(rng, 6000, alphabet=4, maxlen=30, seqs=50)
    items = [(k, t, v * 6) for k, t, v in items]
    payload, ops = make_table(items)
    built = C.run_device(torch, gpu, payload, ops, None, None)
    C.compare_device(built, payload, ops, tag_="defaults")
    assert built.sync_totals()["data_blocks"] > 40


@pytest.mark.parametrize("a", range(0, 16, 3))
def test_copy_widths_and_alignments(gpu, a):
    """Key suffixes and values of 0 .. 2 W + 40 bytes and a few of several KiB,
    the payload shifted by a bytes: lane copies, wave copies with every head
    and tail, sources and destinations at every alignment."""
    import torch
    sizes = list(range(0, 40)) + list(range(W - 20, W + 40)) + [2 * W + 17, 1000, 4096, 5000]
    items = []
    for i, s in enumerate(sizes):
        items.append((b"k%04d" % i + b"K" * ((s * 7) % (2 * W + 30)), tag(i + 1), b"V" * s))
        items.append((b"k%04d" % i + b"L" * s, tag(i + 1), bytes([i % 251]) * ((s * 3) % 200)))
    rng = np.random.default_rng(a)
    gaps = [int(rng.integers(0, 7)) for _ in items]
    for bs, ri in ((4096, 16), (300, 3)):
        C.check_device(torch, gpu, items, bs, ri, shift=a, gaps=gaps, tag_=f"shift={a} bs={bs}")


def test_one_long_key_for_every_entry(gpu):
    """The worst case of the size kernel: one identical 4 KiB user key, the
    shared prefix running 4,096 bytes into the tag for every entry.  With the
    default block_size every entry is a block of its own (a block's first
    entry carries the whole key); with 64 KiB blocks all but one in sixteen
    share it."""
    import torch
    key = bytes(range(256)) * 16
    items = [(key, tag(1000 - i, i % 2), b"v%d" % i) for i in range(300)]
    built, _, _ = C.check_device(torch, gpu, items, tag_="long key")
    assert built.sync_totals()["data_blocks"] == 300
    built, _, _ = C.check_device(torch, gpu, items, 1 << 16, 16, tag_="long key, 64 KiB blocks")
    assert built.sync_totals()["data_blocks"] <= 3


def test_status_paths(gpu):
    import torch
    items, bs, ri = CASES["random_small_blocks"]
    payload, ops = make_table(items)
    _, _, tot = C.model_build(payload, ops, bs, ri)
    nb, fb = tot["data_blocks"], tot["file_bytes"]

    def untouched(b):
        return C.tail_is_canary(b.file_t, 0) and C.tail_is_canary(b.handles_t, 0)
    b = C.run_device(torch, gpu, payload, ops, bs, ri, file_cap=fb - 1)
    assert b.sync_totals(check=False) == dict(tot, status=C.FILE_OVER) and untouched(b)
    with pytest.raises(T.LvError, match="FILE_OVER"):
        b.sync_totals()
    b = C.run_device(torch, gpu, payload, ops, bs, ri, block_cap=nb - 1)
    assert b.sync_totals(check=False) == dict(tot, status=C.HANDLE_OVER) and untouched(b)
    b = C.run_device(torch, gpu, payload, ops, bs, ri, file_cap=0, block_cap=0)
    assert b.sync_totals(check=False) == dict(tot, status=C.FILE_OVER | C.HANDLE_OVER) and untouched(b)
    # the reported file_bytes is the retry's file_cap; larger capacities change nothing
    b = C.run_device(torch, gpu, payload, ops, bs, ri, file_cap=fb + 100, block_cap=nb + 7)
    C.compare_device(b, payload, ops, bs, ri, "larger caps")
    # NO_TABLE: the memtable's status is not 0
    b = C.run_device(torch, gpu, payload, ops, bs, ri, mt_status=M.BAD_OP)
    assert b.sync_totals(check=False) == dict(zip(C.TOTALS, [0] * 7 + [C.NO_TABLE])) and untouched(b)
    # the empty memtable: status 0, nothing written, no file
    payload0, ops0 = make_table([])
    b = C.run_device(torch, gpu, payload0, ops0, file_cap=64, block_cap=4)
    assert b.sync_totals() == dict(zip(C.TOTALS, [0] * 8)) and untouched(b)


def test_block_large(gpu):
    """A block of 2^32 - 1 bytes or more: reported with the true u64 sizes,
    nothing written.  The value's extent lies in a 4 GiB tensor that is
    allocated but never filled; no byte of it is read, because nothing is
    emitted."""
    import torch
    payload, ops = make_table([(b"a", tag(2), b"x"), (b"b", tag(1), b"y")])
    ops = ops.copy()
    ops[1]["val_off"], ops[1]["val_len"] = 16, (1 << 32) - 1
    d_pay = torch.empty((1 << 32) + 16, dtype=torch.uint8, device=gpu)
    d_pay[: len(payload)].copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
    table = MT.build_device(d_pay, M.dev_bytes(torch, gpu, ops), M.dev_i64(torch, gpu, [2]), op_cap=2)
    assert table.sync_totals()["entries"] == 2
    b = T.build_device(table, file_cap=1 << 20, block_cap=4, fill=C.CANARY, guard=C.GUARD)
    t = b.sync_totals(check=False)
    assert t["status"] == C.BLOCK_LARGE | C.FILE_OVER and t["entries"] == 2 and t["data_blocks"] == 1
    assert t["file_bytes"] > (1 << 32) and C.tail_is_canary(b.file_t, 0) and C.tail_is_canary(b.handles_t, 0)


def test_chain_with_no_host_sync(gpu):
    """Memtable build -> SSTable build -> verify on one stream with one
    synchronisation at the end; file_cap from lv_sst_build_file_bound and
    block_cap = op_cap, the defaults of a caller that knows neither count."""
    import torch
    rng = np.random.default_rng(9)
    items = M.random_items(rng, 3000, alphabet=4, maxlen=20, seqs=30)
    payload, ops = make_table(items)
    d_pay = M.dev_bytes(torch, gpu, payload)[: len(payload)]
    d_ops = M.dev_bytes(torch, gpu, ops)
    d_n = M.dev_i64(torch, gpu, [len(ops)])
    s = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        table = MT.build_device(d_pay, d_ops, d_n, stream=s)
        built = T.build_device(table, block_size=512, stream=s, fill=C.CANARY, guard=C.GUARD)
        # verify every slot the caller provided: those past data_blocks + 2 hold the canary, out of range
        st = T.verify_blocks(built.file_t[: built.file_cap], built.handles_t[: 2 * (built.block_cap + 2)], stream=s)
    s.synchronize()
    want_file, want_handles = C.compare_device(built, payload, ops, 512, 16, "chain")
    st = st.cpu().tolist()
    assert st[: len(want_handles)] == [T.BLOCK_OK] * len(want_handles)
    assert set(st[len(want_handles):]) <= {T.BLOCK_OUT_OF_RANGE}
    entries, _, _ = C.read_table(want_file)
    assert len(entries) == len(items)


def test_graph_capture(gpu):
    """The memtable build and the SSTable build captured into one graph after
    a warm-up call; three replays over different tables of one capacity (the
    second replay on is where a memset node would have replayed wrongly)."""
    import torch
    sets = []
    for seed, n in ((1, 2 * TILE + 7), (2, TILE // 2), (3, TILE + 1)):
        payload, ops = make_table(C.tile_items(n, seed=seed))
        sets.append((payload, ops))
    size = max(len(s[0]) for s in sets)
    cap = max(len(s[1]) for s in sets)
    bs, ri = 64, 4
    fcap = T.file_bound(size, cap, bs, ri)
    d_pay = torch.zeros(size, dtype=torch.uint8, device=gpu)
    d_ops = torch.zeros(cap * 32, dtype=torch.uint8, device=gpu)
    d_n = torch.zeros(1, dtype=torch.int64, device=gpu)
    mws = torch.empty(MT.build_workspace_bytes(cap), dtype=torch.uint8, device=gpu)
    sws = torch.empty(T.build_workspace_bytes(cap, cap), dtype=torch.uint8, device=gpu)

    def load(k):
        payload, ops = sets[k]
        d_pay.zero_()
        d_pay[: len(payload)].copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
        d_ops[: len(ops) * 32].copy_(torch.frombuffer(bytearray(ops.tobytes()), dtype=torch.uint8))
        d_n.fill_(len(ops))

    def run(stream=None):
        table = MT.build_device(d_pay, d_ops, d_n, op_cap=cap, workspace=mws, stream=stream)
        return T.build_device(table, block_size=bs, restart_interval=ri, file_cap=fcap, block_cap=cap, workspace=sws,
                              stream=stream, fill=C.CANARY, guard=C.GUARD)

    def verify(k, built, what):
        fresh = T.Built(built.file_t, built.file_cap, built.handles_t, built.block_cap, built.totals, None)
        C.compare_device(fresh, *sets[k], bs, ri, what)

    load(0)
    verify(0, run(), "warm")
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            built = run(s)
    torch.cuda.synchronize()
    for k in (1, 2, 0):
        load(k)
        built.file_t.fill_(C.CANARY)
        built.handles_t.view(torch.uint8).fill_(C.CANARY)
        sws.fill_(0x33)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        verify(k, built, f"replay of set {k}")
