"""The whole pipeline over the device entry points against the plain model of
the store's history (tests/store_cases.py), and byte for byte against the host
backend's run of the same history, so that a mismatch with the model is located
at the first stage that differs.  Outputs are canary-filled with guards behind
them and workspaces dirty (store_cases.DeviceBackend)."""
import numpy as np
import pytest

import lvgpu.compact as CP
import lvgpu.memtable as MT
import lvgpu.table as T
import lvgpu.version_edit as VE
import lvgpu.wal as LW
import lvgpu.write_batch as WB
import store_cases as SC
import wal_oracle as W
from store_cases import BITS_PER_KEY, CANARY, GUARD, OPT, Store, StoreModel
from test_store import SEEDS, assert_life, assert_tombstone_story

pytestmark = pytest.mark.gpu

STAGES = ("wlog", "mem", "images", "manifest", "version", "view", "files", "directory", "counters")  # in pipeline order


def device_store(gpu, fault=None):
    import torch
    return Store(SC.DeviceBackend(torch, gpu), fault)


def host_states(run):
    """The host backend's state at every checkpoint of `run(store, model, checkpoint)`."""
    states = []

    def remember(store, model, name):
        store.merged()
        states.append((name, store.state()))
    run(Store(SC.HostBackend()), StoreModel(), remember)
    return states


def same_as(states):
    """A checkpoint that compares the device's state with the host's, stage by stage."""
    at = iter(states)

    def compare(store, model, name):
        store.merged()
        want_name, want = next(at)
        got = store.state()
        assert name == want_name
        for stage in STAGES:
            assert got[stage] == want[stage], f"{name}: the device's {stage} differs from the host backend's"
    return compare


@pytest.mark.parametrize("seed", SEEDS)
def test_life_of_a_store(gpu, seed):
    """test_store.py's life over the device.  One checkpoint per generation in
    place of one per group (the per-group run takes several times the
    compaction-invariant test of test_gpu_compact_device.py); the shapes, the
    flushes, the compactions and the reopen are the same."""
    def run(store, model, checkpoint, checking=False):
        return SC.life(store, model, seed, per_group=False, checkpoint=checkpoint, checking=checking)
    states = host_states(run)
    store, model = device_store(gpu), StoreModel()
    total = SC.life(store, model, seed, per_group=False, checkpoint=same_as(states))
    assert_life(total, store, model, asked=50000, ranges=1500)
    # the host's own writer frames the device's records to the same log (the host backend's is the oracle's)
    assert LW.encode([b"one", b"x" * 40000], 0) == SC.HostBackend().frame(b"one" + b"x" * 40000, [0, 3], [3, 40000], 0)


def test_a_tombstone_above_a_deeper_value(gpu):
    states = host_states(lambda store, model, cp: SC.tombstone_story(store, model, lambda s, m: (cp(s, m, "t"),
                                                                                                SC.new_report())[1]))
    compare = same_as(states)

    def check_(store, model):
        compare(store, model, "t")
        return SC.check(store, model)
    facts, total = SC.tombstone_story(device_store(gpu), StoreModel(), check_)
    assert_tombstone_story(facts, total)


def test_one_generation_across_the_tiles(gpu):
    """One generation of 2 x the largest tile of the path + 37 ops in more than
    256 batches: every stage that tiles by ops, entries or records crosses two
    tile boundaries and ends in a partial tile, all in one chain."""
    tiles = dict(wb_decode=WB.WB_TILE, wb_encode=WB.WE_TILE, wal_decode=LW.DECODE_TILE, memtable=MT.MT_TILE,
                 filter=CP.CF_TILE, build=T.SB_TILE, scan=T.SS_TILE, edit_decode=VE.VD_TILE, edit_encode=VE.VE_TILE)
    n_ops = 2 * max(tiles.values()) + 37
    rng = np.random.default_rng(77)
    groups = SC.generation(rng, SC.universe(), 1, n_ops)
    batches = sum(len(g) for g in groups)
    ops = sum(len(b) for g in groups for b in g)
    assert batches > 256 and batches > WB.WB_TILE and ops >= n_ops

    def run(store, model, checkpoint, checking=False):
        total = SC.new_report()

        def point(name):
            checkpoint(store, model, name)
            if checking:
                SC.add(total, SC.check(store, model))
        store.write([b for g in groups for b in g])   # one group: the encode's scan tiles are crossed in one call
        for g in groups:
            for b in g:
                model.apply(b)
        store.recover()
        point("recovered")
        store.flush()
        point("flushed")
        store.compact(0, model.last_sequence // 2)
        point("compacted")
        store.reopen()
        point("reopened")
        return total
    states = host_states(run)
    store, model = device_store(gpu), StoreModel()
    total = run(store, model, same_as(states), checking=True)
    assert not total.mismatches, total.mismatches[:5]
    c = store.compactions[0]["totals"]
    reached = dict(wb_decode=batches, wb_encode=ops, wal_decode=batches, memtable=ops, filter=c["entries_in"], build=ops,
                   scan=None, edit_decode=None, edit_encode=None)
    for name in ("wb_decode", "wb_encode", "memtable", "filter", "build"):
        assert reached[name] > (2 if name != "wb_decode" else 1) * tiles[name] and reached[name] % tiles[name], name
    # the scan tiles by blocks and restart runs, the edit stages by records and rows: one partial tile each here
    assert len(store.compactions[0]["outputs"]) + 1 < VE.VE_TILE and c["kept"] // OPT["restart_interval"] < 2 * T.SS_TILE


def test_generation_in_a_graph(gpu):
    """One generation's recover -> flush chain (scan, WAL decode, WriteBatch
    decode, memtable build, Bloom build, open; linear) captured after a warm-up
    and replayed over two other groups of the same capacities: after each
    replay the image is the host backend's, byte for byte, and a store over it
    answers as the model.

    This test found the memset nodes at the head of lv_wal_decode_device and
    lv_write_batch_decode_device ("The store as a whole"): with them
    the second replay handed on 65 of the log's 120 records."""
    import torch
    dev, host = SC.DeviceBackend(torch, gpu), SC.HostBackend()
    keys = SC.universe()
    sets = []
    for seed in (11, 12, 13):
        group = [b for g in SC.generation(np.random.default_rng(seed), keys, 0, 600) for b in g]
        sets.append(group)
    logs = []
    target = None
    for group in sets:  # the same log length for all three: a last put takes up the difference
        def log_of(pad):
            store = Store(host)
            store.write(group + [[(SC.VALUE, b"pad", b"p" * pad)]])
            return bytes(store.wlog)
        if target is None:
            target = len(log_of(0)) + 1500
        pad = 0
        for _ in range(8):
            log = log_of(pad)
            if len(log) == target:
                break
            pad += target - len(log)
        assert len(log) == target, (len(log), target)
        group.append([(SC.VALUE, b"pad", b"p" * pad)])
        logs.append(log)
    buf = torch.zeros((target + 31) & ~15, dtype=torch.uint8, device=gpu)
    log_t = buf[:target]

    hold = []

    def load(k):
        log_t.copy_(torch.frombuffer(bytearray(logs[k]), dtype=torch.uint8))

    def run():
        dec, ops, table = dev.recover_chain(log_t)
        cap = table.op_cap
        built = T.build_bloom_device(table, BITS_PER_KEY, workspace=dev.dirty(T.build_bloom_workspace_bytes(cap, cap)),
                                     fill=CANARY, guard=GUARD, **OPT)
        opened = T.open_device(built.file_t[: built.file_cap], built.totals[2:3], built.totals[7:8], handles=False)
        # what the calls allocated stays referenced across the replays (a Decoded or an Ops lets go of its inputs
        # and its workspace once its totals have been read)
        hold.append([o._keep for o in (dec, ops, table, built, opened)])
        return dec, ops, table, built, opened, dec._keep[1:5]

    def verify(k, out, what):
        torch.cuda.synchronize()
        dec, ops, table, built, opened, scan = out
        for o in (dec, ops, table, built):
            o._tot = None
        opened._tab = None
        model = StoreModel()
        for b in sets[k]:
            model.apply(b)
        hs = Store(host)
        hs.wlog = bytearray(logs[k])
        hs.last_sequence = hs.recover()
        want = host.flush(hs.mem, 1, hs.edit(), 0)[0]
        image = built.file()
        assert log_t.cpu().numpy().tobytes() == logs[k], f"{what}: the log on the device is not the one loaded"
        o, c, i = W.scan_log(logs[k])  # the stage that differs first is named: the scan's arrays, then the records
        n = int(scan[3].cpu()[0])
        got = [x[:n].cpu().numpy().astype(np.int64) & m for x, m in zip(scan[:3], (-1, 0xFFFFFFFF, 0xFFFFFFFF))]
        assert n == len(o) and [g.tolist() for g in got] == [o, c, i], f"{what}: the scan's arrays differ"
        assert dec.records() == host.read_log(logs[k])[0], (
            f"{what}: the log's records differ: {dec.sync_totals()}, reports {dec.reports()[:4]}")
        assert ops.sync_totals()["last_sequence"] == model.last_sequence == hs.last_sequence, what
        assert ops.ops().tobytes() == hs.mem.ops.tobytes() and table.order().tobytes() == hs.mem.order.tobytes(), what
        assert image == want, f"{what}: the image differs from the host backend's"
        assert opened.sync()["file_bytes"] == len(want), what
        dev.canary_behind(built.file_t, len(image))
        store = Store(dev)
        store.directory[1], store.files[1] = (store.add_image(image), len(image)), (0, len(image), None, None)
        store.next_file, store.last_sequence = 2, model.last_sequence
        store.manifest_last_sequence = model.last_sequence
        store.open_version()
        store.take_bounds()
        rep = SC.check(store, model)
        assert not rep.mismatches and rep.found and rep.deleted and rep.absent, (what, rep.mismatches[:5])

    for k in (2, 1, 0):
        load(k)
        verify(k, run(), f"warm-up {k}")  # the device is initialised
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = run()
    torch.cuda.synchronize()
    for k in (1, 2, 0):
        load(k)
        torch.cuda.synchronize()
        g.replay()
        verify(k, out, f"replay {k}")
