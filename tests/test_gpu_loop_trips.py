"""The later trips of the capped-grid kernels.  A kernel whose grid is capped
walks the rest of its work in a grid-stride loop; on its second and third trip
a workgroup reuses LDS, carries registers over, stores deferred results and
consumes prefetched metadata.  Every test here sizes its input from the
device's compute units through tests/loop_trips.py (the launchers' own
arithmetic), asserts the trips it takes, and compares every output bit for bit
with a model that does not know about grids: the oracle hash, the Python
WriteBatch / WAL / table models (over a motif, tiled: test_loop_trips_models.py
ties the tiling to the models), values known by construction, and the host
twins that the CPU tests pin to the models."""
import ctypes

import numpy as np
import pytest

import loop_trips as LT
import loop_trips_cases as LC
import wal_oracle as W

pytestmark = pytest.mark.gpu

PEAK_LIMIT = 4 << 30


@pytest.fixture(scope="module", autouse=True)
def peak(gpu):
    """The module's own peak: the statistics start again here."""
    import gc
    import torch
    torch.zeros(1, device=gpu)  # (the allocator has no statistics for a device before its first allocation)
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(gpu)
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def cus(gpu):
    return LT.device_cus(gpu)


def _need(kernel, units, cus, want):
    got = LT.trips(kernel, units, cus)
    assert got >= want, f"{kernel}: {units} units on {cus} compute units take {got} trips, the test needs {want}"
    return got


# ---- hash_kernel --------------------------------------------------------------
def _oracle_hash():
    L = W.lib()
    L.oracle_hash_batch.restype = None
    L.oracle_hash_batch.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t]
    return L


@pytest.fixture(scope="module")
def hash_case(cus):
    """Keys laid end to end from arena offset 3, the layout of each wave-set
    chosen by the trip it is hashed on: trip 0 keys of 8-40 B (the wave stages
    its span in LDS), trip 1 keys of 70-300 B (64 of them span more than 4 KiB:
    not staged, key_from_mem), trip 2 keys of 8-40 B again with empty keys on
    the first and last lanes of some sets (the stage reused after a set that
    left it alone)."""
    n = LT.size_for("hash_kernel", 3, cus, 64 * 5 + 17)
    _need("hash_kernel", n, cus, 3)
    grid, per = LT.grid_of("hash_kernel", n, cus)
    assert per == 256
    rng = np.random.default_rng(20260)
    trip = (np.arange(n) // 64) // (4 * grid)
    assert trip.max() == 2 and (trip == 2).sum() == n - 2 * 256 * grid
    lens = rng.integers(8, 41, n).astype(np.uint32)
    long_ = rng.integers(70, 301, n).astype(np.uint32)
    lens[trip == 1] = long_[trip == 1]
    first2 = int(np.argmax(trip == 2))
    for s, lanes in ((0, [0]), (1, [63]), (2, [0, 1, 62, 63]), (4, [0, 63])):
        for lane in lanes:
            if first2 + 64 * s + lane < n:
                lens[first2 + 64 * s + lane] = 0
    lens[n - 1] = 0  # the last key of the ragged last set
    bounds = np.zeros(n + 1, dtype=np.uint64)
    bounds[1:] = np.cumsum(lens, dtype=np.uint64)
    bounds += 3
    assert int(bounds[-1]) < 1 << 32
    arena = rng.integers(0, 256, size=int(bounds[-1]) + 5, dtype=np.uint8)
    seeds = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    offs = bounds[:-1].copy()
    spans = (bounds[64::64][: n // 64] - bounds[0:-1:64][: n // 64]).astype(np.int64)
    t_of_set = trip[::64][: n // 64]
    assert spans[t_of_set == 1].min() > 4096 and spans[t_of_set != 1].max() + 16 <= 4096
    L = _oracle_hash()
    want = {}
    for name, sd in (("seeded", seeds), ("unseeded", None)):
        w = np.zeros(n, dtype=np.uint32)
        L.oracle_hash_batch(arena.ctypes.data, offs.ctypes.data, lens.ctypes.data, None if sd is None else sd.ctypes.data,
                            w.ctypes.data, n)
        want[name] = w
    assert not np.array_equal(want["seeded"], want["unseeded"])
    return dict(n=n, arena=arena, offs=offs, lens=lens, bounds=bounds, seeds=seeds, want=want, trip=trip)


def _t(gpu, a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu)


def _report(got, want, trip):
    bad = np.nonzero(got != want)[0]
    return None if bad.size == 0 else f"{bad.size} hashes differ, the first is key {int(bad[0])} of trip {int(trip[bad[0]])}"


@pytest.mark.parametrize("seeded", ["seeded", "unseeded"])
def test_hash_three_trips_offsets(gpu, hash_case, seeded):
    """lv_hash_batch_device over three trips of every wave: the result stored
    one set late, the clamped one-set-ahead metadata load and the LDS stage
    reused after wave_barrier, hashes and LV_HASH_SHARD."""
    import torch
    from lvgpu import hash as H
    c = hash_case
    a = torch.from_numpy(c["arena"]).to(gpu)
    ds = _t(gpu, c["seeds"], np.int32) if seeded == "seeded" else None
    o, ln = _t(gpu, c["offs"], np.int64), _t(gpu, c["lens"], np.int32)
    want = c["want"][seeded]
    got = H.hash_batch(a, o, ln, ds).cpu().numpy().view(np.uint32)
    assert _report(got, want, c["trip"]) is None, _report(got, want, c["trip"])
    sh = H.hash_batch(a, o, ln, ds, shard=True).cpu().numpy().view(np.uint32)
    assert _report(sh, want >> 28, c["trip"]) is None, _report(sh, want >> 28, c["trip"])


@pytest.mark.parametrize("width", [4, 8])
def test_hash_three_trips_packed(gpu, hash_case, width):
    """lv_hash_batch_packed over the same keys (they are laid end to end):
    lengths from the bound deltas, lane 63 and the last key reading the bound
    after them, on every trip."""
    import torch
    from lvgpu import hash as H
    c = hash_case
    a = torch.from_numpy(c["arena"]).to(gpu)
    b = _t(gpu, c["bounds"].astype(np.uint32) if width == 4 else c["bounds"], np.int32 if width == 4 else np.int64)
    for seeded in ("seeded", "unseeded"):
        ds = _t(gpu, c["seeds"], np.int32) if seeded == "seeded" else None
        want = c["want"][seeded]
        got = H.hash_batch_packed(a, b, ds).cpu().numpy().view(np.uint32)
        assert _report(got, want, c["trip"]) is None, (seeded, _report(got, want, c["trip"]))
    sh = H.hash_batch_packed(a, b, ds, shard=True).cpu().numpy().view(np.uint32)
    assert _report(sh, want >> 28, c["trip"]) is None


# ---- wb_count / wb_tiles / wb_emit ---------------------------------------------
def test_write_batch_three_trips(gpu, cus):
    """lv_write_batch_decode_device over 3 trips of wb_count and wb_emit (s_tile
    zeroed again, s_scan / s_base and the s_win windows reused) and 8 or more
    rounds of wb_tiles with its carry: the 997-record motif, tiled."""
    import torch
    import write_batch_cases as C
    import lvgpu.write_batch as WB
    n = LT.size_for("wb_emit", 3, cus, 300)
    assert n % 64 and n % WB.WB_TILE and n % LC.WB_MOTIF
    for k, want in (("wb_emit", 3), ("wb_count", 3), ("wb_tiles", 8)):
        _need(k, n, cus, want)
    payload, off, ln = LC.wb_motif()
    want = LC.wb_tiled(C.model(payload, off, ln), len(payload), n)
    p, o, l = LC.wb_tiled_inputs(payload, off, ln, n)
    d_pay = torch.from_numpy(np.frombuffer(p, dtype=np.uint8).copy()).to(gpu)
    d_n = C.dev_i64(torch, gpu, [n])
    ws = torch.full((WB.decode_workspace_bytes(n),), 0x5A, dtype=torch.uint8, device=gpu)
    ops = WB.decode_device(d_pay, C.dev_i64(torch, gpu, o), C.dev_i64(torch, gpu, l), d_n, None, rec_cap=n,
                           op_cap=want[3]["ops"] + 3, workspace=ws, fill=C.CANARY, guard=C.GUARD)
    C.compare(ops, want, "three trips")


# ---- wal_frame_kernel / wal_unframe_kernel ------------------------------------
@pytest.fixture(scope="module")
def wal_blocks(cus):
    recs, log = LC.wal_motif()
    mb = len(log) // LC.B
    nblocks = LT.size_for("wal_frame_kernel", 3, cus, 5)
    reps = -(-nblocks // mb)
    total = reps * mb  # whole motifs: at least the blocks asked for
    _need("wal_frame_kernel", total, cus, 3)
    _need("wal_unframe_kernel", total, cus, 3)
    grid, _ = LT.grid_of("wal_frame_kernel", total, cus)
    assert mb % 2 == 1 and grid % mb  # a workgroup's successive blocks are different blocks of the motif
    return dict(recs=recs, log=log, mb=mb, reps=reps, total=total, grid=grid)


def test_wal_encode_three_trips(gpu, wal_blocks):
    """lv_wal_encode_device over three trips of wal_frame_kernel: s_pos refilled
    for blocks of one to over a thousand fragments, against the Writer model of
    the motif, tiled."""
    import torch
    import lvgpu.wal as LW
    from wal_encode_cases import CANARY, GUARD, pack
    c = wal_blocks
    payload, off, ln = pack(c["recs"])
    reps = c["reps"]
    pay = np.tile(np.frombuffer(payload, dtype=np.uint8), reps)
    base = np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(len(payload)), len(off))
    offs, lens = np.tile(off, reps) + base, np.tile(ln, reps)
    need, _ = LW.encode_size(lens, 0)
    assert need == reps * len(c["log"])
    d_pay = torch.from_numpy(pay).to(gpu)
    buf = torch.full((need + 2 * GUARD + 32,), CANARY, dtype=torch.uint8, device=gpu)
    at = (-buf.data_ptr()) % 16 + 9 + GUARD
    got = LW.encode_device(d_pay, offs, lens, 0, out=buf[at:at + need])
    torch.cuda.synchronize()
    assert got.numel() == need
    host = buf.cpu().numpy()
    want = np.tile(np.frombuffer(c["log"], dtype=np.uint8), reps)
    bad = np.nonzero(host[at:at + need] != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, the first in block {int(bad[0]) // LC.B} (grid {c['grid']})"
    assert (host[:at] == CANARY).all() and (host[at + need:] == CANARY).all()


def test_wal_decode_three_trips(gpu, cus, wal_blocks):
    """lv_wal_scan_device + lv_wal_decode_device over three trips of
    wal_unframe_kernel (s_out / s_src / s_span refilled per block) with a
    flipped byte in a block of trip 0 and in one of trip 2, against the Reader
    model of the motif, tiled; the scan's wal_unsort goes round too."""
    import torch
    from wal_decode_cases import collect, guards_ok, headers, run_decode
    import lvgpu.wal as LW
    c = wal_blocks
    mb, grid, reps = c["mb"], c["grid"], c["reps"]
    g0, g2 = 1, 2 * grid + 2  # a block of trip 0 and one of trip 2
    assert g0 // grid == 0 and g2 // grid == 2 and g2 < c["total"] and g2 // mb != g0 // mb
    t = LC.WalTiled(c["log"], reps, {g0 // mb: g0 % mb, g2 // mb: g2 % mb})
    full = t.full_log()
    entries = reps * len(headers(c["log"]))
    _need("wal_unsort", entries + 3, cus, 2)
    r = collect(torch, run_decode(torch, gpu, full.tobytes(), pay_shift=5, cap=entries + 3))
    assert r.count == entries
    pay, lens, offs, reports, dropped, at = t.expected()
    tot = r.dec.sync_totals()
    assert tot == dict(records=len(lens), payload_bytes=len(pay), reports=len(reports), dropped_bytes=dropped, status=0)
    nrec = len(lens)
    got_pay = r.host[r.base:r.base + len(pay)]
    bad = np.nonzero(got_pay != np.frombuffer(pay, dtype=np.uint8))[0]
    assert bad.size == 0, f"{bad.size} payload bytes differ, the first at {int(bad[0])}"
    assert np.array_equal(r.dec.rec_len[:nrec].cpu().numpy(), lens)
    assert np.array_equal(r.dec.rec_off[:nrec].cpu().numpy(), np.concatenate([[0], np.cumsum(lens)[:-1]]))
    assert np.array_equal(r.dec.rec_log_off[:nrec].cpu().numpy(), offs)
    assert r.dec.reports() == reports and len(reports) >= 2
    rep_at = r.dec.rep_log_off[: len(reports)].cpu().numpy()
    for i, hdr in at.items():
        assert reports[i][1] == "checksum mismatch" and int(rep_at[i]) == hdr, (i, reports[i], int(rep_at[i]), hdr)
    assert guards_ok(r, len(pay))


# ---- wal_dec_classify / reduce / tiles / apply ------------------------------------
def test_wal_decode_entries_two_trips(gpu, cus):
    """One-byte records, enough scan entries for a second trip of
    wal_dec_reduce and wal_dec_apply (and of wal_dec_classify, and eight
    rounds of wal_dec_tiles): a FIRST / MIDDLE / LAST triple in the first tile
    of the second trip and a checksum mismatch after it.  Every expected value
    follows from the construction: entry i is the 8 bytes at 8 i."""
    import torch
    from wal_decode_cases import H, collect, flip, guards_ok, run_decode, set_type
    from wal_encode_cases import B, oracle_encode
    import lvgpu.wal as LW
    n = LT.size_for("wal_dec_reduce", 2, cus, 1025)
    for k in ("wal_dec_reduce", "wal_dec_apply", "wal_dec_classify", "wal_dec_tiles"):
        _need(k, n + 2, cus, 2)
        g, per = LT.grid_of(k, n + 2, cus)  # the grid is sized by scan_cap = n + 2, the loops run over the n entries
        assert -(-n // per) > g, k
    grid, tile = LT.grid_of("wal_dec_reduce", n + 2, cus)
    assert tile == LW.DECODE_TILE and n % tile and n % 64
    t0 = grid * tile  # the first entry of the second trip
    f, bad = t0 + 10, t0 + 500
    log = bytearray(oracle_encode([b"a"]) * n)
    for i, ty in ((f, W.FIRST), (f + 1, W.MIDDLE), (f + 2, W.LAST)):
        set_type(log, 8 * i, ty)
    flip(log, 8 * bad + H)
    r = collect(torch, run_decode(torch, gpu, bytes(log), pay_shift=3, cap=n + 2))
    assert r.count == n
    # the mismatch drops its entry and the rest of its block (or of the log)
    per = B // 8
    end = min((bad // per + 1) * per, n)
    alive = np.ones(n, dtype=bool)
    alive[bad:end] = False
    alive[f + 1:f + 3] = False  # the MIDDLE and the LAST belong to the FIRST's record
    want_log = 8 * np.nonzero(alive)[0].astype(np.int64)
    want_len = np.ones(want_log.size, dtype=np.int64)
    want_len[f] = 3
    tot = r.dec.sync_totals()
    assert tot == dict(records=want_log.size, payload_bytes=int(want_len.sum()), reports=1,
                       dropped_bytes=8 * (end - bad), status=0)
    k = want_log.size
    assert np.array_equal(r.dec.rec_log_off[:k].cpu().numpy(), want_log)
    assert np.array_equal(r.dec.rec_len[:k].cpu().numpy(), want_len)
    assert np.array_equal(r.dec.rec_off[:k].cpu().numpy(), np.concatenate([[0], np.cumsum(want_len)[:-1]]))
    assert (r.host[r.base:r.base + tot["payload_bytes"]] == ord("a")).all() and guards_ok(r, tot["payload_bytes"])
    assert r.dec.reports() == [(8 * (end - bad), "checksum mismatch")]
    assert int(r.dec.rep_log_off[0].item()) == 8 * bad


# ---- sb_bloom_emit / sb_bloom_big -------------------------------------------------
def test_bloom_build_three_trips(gpu, cus):
    """lv_sst_build_bloom_device over one-entry data blocks (block_size 1),
    enough for a third trip of sb_bloom_emit's waves: 1 to 40 keys to a filter
    window, so a wave's later filter is often smaller than the one before it in
    the same LDS (stale bits would show), against the serial Python model; then
    lv_sst_get_bloom_device for every key and 2,000 absent ones against the
    host twin."""
    import torch
    import lvgpu.table as T
    import sst_bloom_cases as SB
    import sst_get_cases as G
    n = LT.size_for("sb_bloom_emit", 3, 1, 7)  # (the cap is a constant: any cus)
    _need("sb_bloom_emit", n, 1, 3)
    _need("sb_bloom_big", n, 1, 3)
    _need("sst_blocks_kernel", n + 3, cus, 2)  # the seal of the data blocks, the filter block and the metaindex
    rng = np.random.default_rng(516)
    items = LC.bloom_items(n)
    built, payload, ops, want = SB.check_device(torch, gpu, items, 1, 16, 10, tag_="three trips")
    image, handles, tot, btot = want
    assert tot["data_blocks"] == n
    per_window = np.bincount([o >> SB.BASE_LG for o, _ in handles[:n]])
    assert per_window[per_window > 0].min() == 1 and per_window.max() >= 35 and btot["filter_keys"] == n
    # the filtered get: every key at its own snapshot, and keys the table does not hold
    held = [(k, t >> 8) for k, t, _ in items]
    absent = [(b"key%07d" % (3 * int(v) + 1), 1 << 40) for v in rng.integers(0, n, 2000)]
    queries = held + absent
    table, bloom, wants = SB.host_answers(image, queries)
    assert bloom["present"] == 1 and all(w["status"] == G.FOUND for w in wants[:n])
    assert sum(w["reserved"] == SB.FILTERED for w in wants[n:]) >= 1800 and all(w["status"] == G.ABSENT for w in wants[n:])
    op, bloom_t, owner = SB.open_both(torch, gpu, image, shift=3)
    qk, off, ln, sq, _ = G.pack_queries(queries, bad_query=False)
    got = SB.run_get(torch, gpu, op, bloom_t, qk, off, ln, sq)
    assert op.sync() == table and T.bloom_dict(bloom_t) == bloom
    for name in G.RESULT_FIELDS:
        w = np.array([x[name] for x in wants], dtype=np.uint64)
        bad = np.nonzero(got[name].astype(np.uint64) != w)[0]
        assert bad.size == 0, (name, int(bad[0]), int(got[name][bad[0]]), int(w[bad[0]]))


def test_bloom_big_three_trips(gpu, cus):
    """lv_sst_build_bloom_device at 64 bits per key over one-entry 4 KiB blocks,
    enough for a third trip of sb_bloom_big's waves, with one crowded block
    (281 keys: a filter of 2,249 bytes, beyond the wave's LDS) on each of the
    three trips, so the kernel sets bits on every trip and not only skips.  The
    crowded filters lie between 9-byte filters of their neighbours and start
    and end off the dword grid: the atomic ORs on shared dwords must keep the
    neighbours' bytes.  Every byte of the image and both totals against the
    serial Python model; then lv_sst_get_bloom_device over the crowded windows:
    every key they hold is found, and every absent key is filtered or not as
    the Python model's reader decides for that key."""
    import torch
    import lvgpu.table as T
    import sst_bloom_cases as SB
    import sst_get_cases as G
    nb = LT.size_for("sb_bloom_big", 3, 1, 7)  # (the cap is a constant: any cus)
    grid, per = LT.grid_of("sb_bloom_big", nb, 1)
    crowded = [per * 100 + 1, grid * per + per * 511 + 2, 2 * grid * per + 3]  # a wave 1, a wave 2 and a wave 3
    assert [b // (grid * per) for b in crowded] == [0, 1, 2] and crowded[-1] + 1 < nb
    items, where = LC.bloom_big_items(nb, set(crowded))
    # the launch sizes its grid by op_cap, the entries; the loop runs over the data blocks
    assert LT.grid_of("sb_bloom_big", len(items), 1) == (grid, per) and -(-nb // per) > 2 * grid
    _need("sb_bloom_big", nb, 1, 3)
    _need("sb_bloom_emit", nb, 1, 3)
    built, payload, ops, want = SB.check_device(torch, gpu, items, LC.BLOOM_BIG_BLOCK, 16, 64, tag_="big filters, three trips")
    image, handles, tot, btot = want
    assert tot["data_blocks"] == nb and btot["filter_keys"] == len(items)
    fo, fs = handles[-3]
    arr = fo + fs - 5 - 4 * btot["filters"]
    start = lambda w: G.le32(image, arr + 4 * w)
    sizes = np.diff([start(w) for w in range(btot["filters"] + 1)])  # (the word behind the array is the array's offset)
    big = np.nonzero(sizes > T.SB_BLOOM_LDS + 1)[0].tolist()
    assert big == [handles[b][0] >> SB.BASE_LG for b in crowded], (big, crowded)  # the model: exactly these windows
    ragged = 0
    for b, w in zip(crowded, big):
        assert sizes[w] == (where[b][1] * 64 + 7) // 8 + 1
        small = [int(s) for s in sizes[w - 4:w + 5] if 0 < s <= T.SB_BLOOM_LDS + 1]
        assert len(small) >= 2 and set(small) == {9}, small  # one key, 64 bits and the k byte, on either side
        ragged += (start(w) % 4 != 0) + (start(w + 1) % 4 != 0)
    assert ragged >= 4
    # the filtered get over the crowded windows
    held, absent = [], []
    for b in crowded:
        at, k = where[b]
        held += [(items[j][0], items[j][1] >> 8) for j in range(at, at + k)]
        absent += [(b"key%07d" % (int(items[j][0][3:]) + 1), 1 << 40) for j in range(at, at + k, 2)]
    queries = held + absent
    table, bloom, wants = SB.host_answers(image, queries)
    assert (table, bloom, wants[len(held):]) == SB.model_answers(image, absent)  # the Python reader, key by key
    assert bloom["present"] == 1 and all(w["status"] == G.FOUND for w in wants[: len(held)])
    assert all(w["status"] == G.ABSENT for w in wants[len(held):])
    assert sum(w["reserved"] == SB.FILTERED for w in wants[len(held):]) >= len(absent) - 3  # (64 bits a key)
    op, bloom_t, owner = SB.open_both(torch, gpu, image, shift=3)
    qk, off, ln, sq, _ = G.pack_queries(queries, bad_query=False)
    got = SB.run_get(torch, gpu, op, bloom_t, qk, off, ln, sq)
    assert op.sync() == table and T.bloom_dict(bloom_t) == bloom
    for name in G.RESULT_FIELDS:
        w = np.array([x[name] for x in wants], dtype=np.uint64)
        bad = np.nonzero(got[name].astype(np.uint64) != w)[0]
        assert bad.size == 0, (name, int(bad[0]), int(got[name][bad[0]]), int(w[bad[0]]))
    del built, op, bloom_t, owner


# ---- so_validate / so_emit --------------------------------------------------------
def test_table_open_two_trips(gpu, cus):
    """lv_sst_open_device over a table of one-entry blocks, enough for a second
    trip of so_validate and so_emit: the image and its handles from
    lv_sst_build_host, the table from lv_sst_open_host.  Then
    lv_sst_verify_blocks_device over the handles, where every workgroup of
    sst_blocks_kernel claims from its pool again and again: the trailers are
    the host build's (the scalar CRC), so OK for every block says the walk's
    CRCs are right, and one flipped byte must cost exactly its block."""
    import torch
    import lvgpu.table as T
    from lvgpu.write_batch import OP_DTYPE
    import sst_get_cases as G
    n = LT.size_for("so_validate", 2, 1, 11)
    _need("so_validate", n, 1, 2)
    _need("so_emit", n + 2, 1, 2)
    keys = np.char.add("k", np.char.zfill(np.arange(n).astype(str), 7)).astype("S8")
    payload = keys.tobytes()
    ops = np.zeros(n, dtype=OP_DTYPE)
    ops["tag"] = ((np.arange(n, dtype=np.uint64) % 5 + 1) << 8) | 1
    ops["key_off"] = 8 * np.arange(n, dtype=np.uint64)
    ops["val_off"] = ops["key_off"] + 3  # the value: five bytes of the key
    ops["key_len"], ops["val_len"] = 8, 5
    image, handles, tot = T.build_host(payload, ops, np.arange(n, dtype=np.uint32), dict(entries=n, user_keys=n, status=0),
                                       block_size=1)
    assert tot["data_blocks"] == n and tot["status"] == 0 and len(handles) == n + 2
    table, host_handles = T.open_host(image)
    assert host_handles == handles and table["data_blocks"] == n and table["status"] == 0
    owner, file_t = G.place(torch, gpu, image, 5)
    op = G.run_open(torch, gpu, file_t, len(image), block_cap=n)
    assert op.sync(check=False) == table
    got = op.handles_t[: 2 * (n + 2)].cpu().numpy().view(np.uint64).reshape(n + 2, 2)
    want = np.array(handles, dtype=np.uint64)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} handles differ, the first is {int(bad[0])}: {got[bad[0]]} != {want[bad[0]]}"
    from write_batch_cases import tail_is_canary
    assert tail_is_canary(op.handles_t, 16 * (n + 2))
    _need("sst_blocks_kernel", n + 2, cus, 2)
    hv = op.handles_view()
    st = T.verify_blocks(file_t, hv).cpu().numpy()
    assert (st == T.BLOCK_OK).all(), np.nonzero(st != T.BLOCK_OK)[0][:8]
    g_claims, per_claim = LT.grid_of("sst_blocks_kernel", n + 2, cus)
    j = g_claims * per_claim * 3 + 5  # a block of a workgroup's fourth claim
    assert j < n
    hurt = file_t.clone()
    hurt[handles[j][0] + 2] ^= 0x10
    st = T.verify_blocks(hurt, hv).cpu().numpy()
    assert np.nonzero(st != T.BLOCK_OK)[0].tolist() == [j] and st[j] == T.BLOCK_CHECKSUM_MISMATCH
    # a restart that only a second-trip lane of so_validate looks at: restart i + 1 of the index block
    # set to restart i, so restart i holds no entry and restart i + 1 two
    grid, per = LT.grid_of("so_validate", n, 1)
    i = grid * per + 2
    assert i + 1 < n
    arr = table["index_offset"] + table["index_size"] - 4 - 4 * n
    bad = bytearray(image)
    bad[arr + 4 * (i + 1):arr + 4 * (i + 2)] = bad[arr + 4 * i:arr + 4 * (i + 1)]
    want_t, _ = T.open_host(bytes(bad))
    assert want_t["status"] != 0 and want_t["data_blocks"] == n
    owner2, file2 = G.place(torch, gpu, bytes(bad), 5)
    op2 = G.run_open(torch, gpu, file2, len(bad), block_cap=n)
    assert op2.sync(check=False) == want_t
    assert tail_is_canary(op2.handles_t, 0), "handles written for a table with a status"


# ---- sb_carry / ss_carry / cf_carry: the second round of the carry scans -----------
def test_carry_scans_second_round(gpu):
    """More than 64 scan tiles of entries, of data blocks and of restart runs:
    the one wave of cf_carry, sb_carry (all four columns: block_size 1 makes
    every entry a data block, so the filters' column by block id is as long)
    and ss_carry goes round twice, its running sum carried over.  Memtable
    build -> compaction filter -> Bloom table build -> open -> scan on the
    device, every stage against its host twin."""
    import torch
    import lvgpu.compact as CP
    import lvgpu.memtable as MT
    import lvgpu.table as T
    import memtable_cases as M
    import sst_get_cases as G
    from lvgpu.write_batch import OP_DTYPE
    n = LT.size_for("sb_carry", 2, 1, 2517)
    for k in ("sb_carry", "ss_carry", "cf_carry"):
        _need(k, n, 1, 2)
    # 8-byte keys in order, every 101st a second version of the key before it (the filter drops those
    # below the snapshot), values of 0 to 11 bytes cut from the key area
    i = np.arange(n, dtype=np.uint64)
    ident = i - (i % 101 == 3)
    payload = np.char.add("u", np.char.zfill(ident.astype(str), 7)).astype("S8").tobytes()
    ops = np.zeros(n, dtype=OP_DTYPE)
    ops["tag"] = ((i + 1) << np.uint64(8)) | np.uint64(1)
    ops["key_off"], ops["key_len"] = 8 * i, 8
    ops["val_len"] = (i % 12).astype(np.uint32)
    ops["val_off"] = (8 * i) % np.uint64(len(payload) - 16)
    order, mt = MT.build_host(payload, ops)
    assert mt["status"] == 0 and mt["entries"] == n and mt["user_keys"] < n
    table, _buf = M.run_build(torch, gpu, payload, ops, shift=3)
    assert table.sync_totals() == mt and np.array_equal(table.order(), order)
    snapshot = n  # above most sequences: the older of two versions goes
    want_f = CP.filter_host(payload, ops, order, mt, snapshot)
    kept = want_f.totals["kept"]
    assert LT.trips("sb_carry", kept, 1) >= 2 and kept < n
    f = CP.filter_device(table, snapshot, fill=M.CANARY, guard=M.GUARD)
    assert f.sync() == want_f.totals and f.sync_totals() == want_f.mt_totals
    assert np.array_equal(f.order_t[:kept].cpu().numpy().view(np.uint32), want_f.order())
    image, handles, tot, btot = T.build_bloom_host(payload, ops, want_f.order(), want_f.mt_totals, 10, 1, 1)
    assert tot["status"] == 0 and tot["data_blocks"] == kept == btot["filter_keys"]
    built = T.build_bloom_device(f, 10, block_size=1, restart_interval=1, file_cap=len(image), block_cap=kept,
                                 fill=M.CANARY, guard=M.GUARD)
    assert built.sync_totals() == tot and built.sync_bloom_totals() == btot
    got = built.file_t[: len(image)].cpu().numpy()
    bad = np.nonzero(got != np.frombuffer(image, dtype=np.uint8))[0]
    assert bad.size == 0, f"{bad.size} bytes of the image differ, the first at {int(bad[0])} of {len(image)}"
    got_h = built.handles_t[: 2 * (kept + 3)].cpu().numpy().view(np.uint64).reshape(-1, 2)
    assert np.array_equal(got_h, np.array(handles, dtype=np.uint64))
    table_h, _ = T.open_host(image, handles=False)
    op = T.open_device(built.file_t[: built.file_cap], built.totals[2:3], built.totals[7:8], block_cap=kept,
                       fill=M.CANARY, guard=M.GUARD)
    assert op.sync() == table_h
    want_s, want_ops, want_arena, _ = T.scan_host(image, table_h)
    assert want_s["status"] == 0 and want_s["entries"] == kept
    sc = T.scan_device(op, arena_cap=want_s["arena_bytes"], op_cap=kept, block_cap=kept, fill=M.CANARY, guard=M.GUARD)
    assert sc.sync() == want_s
    assert np.array_equal(sc.ops(), want_ops[:kept]) and sc.arena() == want_arena[: want_s["arena_bytes"]].tobytes()


# ---- ss_count: the second trip over the tiles of restart runs ---------------------
def test_table_scan_second_trip(gpu):
    """lv_sst_scan_device over a table of more restart runs than ss_count has
    workgroups times a tile: restart_interval 1 makes every entry a run, and
    behind the 4,096 tiles of the first trip come a full tile and a ragged one,
    so two workgroups fill s_e / s_b a second time.  Memtable build -> table
    build -> verify -> open -> scan on the device.  The scan of a build is the
    sorted op table, here the input itself: every op's tag and lengths, its
    offsets (the arena is packed) and its key and value bytes gathered from
    the arena are compared on the device, for every entry.  The built image is
    tied to the Python model on the blocks that a prefix of the entries fully
    determines, and every data block's handle to the builder's rule.  Then one
    byte: an entry's non_shared length, in a run that only a second-trip lane
    walks, made to overrun its run and the entries behind it: CORRUPT, nothing
    written, as lv_sst_scan_host says of the same flip in the small image."""
    import torch
    import lvgpu.table as T
    import memtable_cases as M
    import sst_build_cases as S
    first_two = LT.size_for("ss_count", 2, 1)
    _, per = LT.grid_of("ss_count", first_two, 1)
    n = LT.size_for("ss_count", 2, 1, per + 299)  # the first trip's tiles, a full tile, 300 runs
    payload, ops = LC.scan_ops(n)
    first, boff, bsize, at = LC.scan_layout(ops["val_len"])
    nb = len(first) - 1
    grid, per = LT.grid_of("ss_count", n + nb, 1)  # the launch: run_cap = op_cap + block_cap; the loop: the runs
    assert per == T.SS_TILE and -(-n // per) == grid + 2 and n % per == 300
    _need("ss_count", n, 1, 2)
    table, buf = M.run_build(torch, gpu, payload, ops, shift=3)
    assert table.sync_totals() == dict(entries=n, user_keys=n, status=0)
    assert bool((table.order_t[:n] == torch.arange(n, dtype=torch.int32, device=gpu)).all())
    built = T.build_device(table, block_size=LC.SCAN_BLOCK, restart_interval=1, block_cap=nb, fill=M.CANARY, guard=M.GUARD)
    tot = built.sync_totals()
    assert (tot["entries"], tot["data_blocks"], tot["status"]) == (n, nb, 0)
    fb = tot["file_bytes"]
    hv = built.handles_view()
    want_h = torch.from_numpy(np.stack([boff, bsize], axis=1)).to(gpu)
    assert torch.equal(hv[:nb], want_h), "data block handles differ from the builder's rule"
    assert tot["metaindex_offset"] == int(boff[-1] + bsize[-1]) + 5
    # the Python model on a prefix: all of its blocks but the last are the table's first blocks
    pp, po = LC.scan_ops(4000)
    image_p, handles_p, _ = S.model_build(pp, po, LC.SCAN_BLOCK, 1)
    k = len(handles_p) - 3
    end = handles_p[k - 1][0] + handles_p[k - 1][1] + 5
    assert k >= 20 and built.file_t[:end].cpu().numpy().tobytes() == image_p[:end]
    st = T.verify_blocks(built.file_t[:fb], hv)
    assert bool((st == T.BLOCK_OK).all()), torch.nonzero(st != T.BLOCK_OK)[:8].tolist()
    op = T.open_device(built.file_t[:fb], built.totals[2:3], built.totals[7:8], block_cap=nb, fill=M.CANARY, guard=M.GUARD)
    opened = op.sync()
    assert (opened["data_blocks"], opened["file_bytes"], opened["status"]) == (nb, fb, 0)
    arena_bytes = int(ops["key_len"].sum(dtype=np.uint64) + ops["val_len"].sum(dtype=np.uint64))
    sc = T.scan_device(op, arena_cap=arena_bytes, op_cap=n, block_cap=nb, fill=M.CANARY, guard=M.GUARD)
    assert sc.sync() == dict(entries=n, arena_bytes=arena_bytes, table_entries=n, table_bytes=arena_bytes, data_blocks=nb,
                             runs=n, reserved=0, status=0)
    from write_batch_cases import tail_is_canary
    assert tail_is_canary(sc.ops_t, 32 * n) and tail_is_canary(sc.arena_t, arena_bytes)
    got = sc.ops_t[: 32 * n].view(torch.int64).view(n, 4)
    vlen = torch.from_numpy(ops["val_len"].astype(np.int64)).to(gpu)

    def same(name, g, w):
        bad = torch.nonzero(g != w)
        assert bad.numel() == 0, f"{name}: {bad.shape[0]} entries differ, the first is entry {int(bad[0][0])} of {n}"
    same("tag", got[:, 0], torch.from_numpy(ops["tag"].view(np.int64)).to(gpu))
    same("key_len and val_len", got[:, 3], 8 + (vlen << 32))
    koff = torch.cumsum(8 + vlen, 0) - (8 + vlen)
    same("key_off", got[:, 1], koff)
    same("val_off", got[:, 2], koff + 8)
    keys = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(gpu).view(n, 8)
    arena = sc.arena_t
    same("key bytes", arena[got[:, 1, None] + torch.arange(8, device=gpu)], keys)
    for j in (0, 1):  # the value: the key's last val_len bytes
        has = torch.nonzero(vlen > j)[:, 0]
        assert has.numel() > n // 4
        same(f"value byte {j}", arena[got[has, 2] + j], keys[has, 8 - vlen[has] + j])
    del keys, got, koff, want_h
    # the damage: the last entry of a block of the first tile of the second trip
    blk = int(np.searchsorted(first, grid * per + 500, side="right"))
    r = int(first[blk + 1]) - 1
    assert grid * per <= r < (grid + 1) * per and r // per - grid == 0 and r < n
    pos = int(boff[blk] + at[r]) + 1
    assert int(built.file_t[pos]) == 16 and int(built.file_t[pos - 1]) == 0
    hurt = built.file_t[:fb].clone()
    hurt[pos] = 0xFF
    op2 = T.open_device(hurt, built.totals[2:3], built.totals[7:8], block_cap=nb, fill=M.CANARY, guard=M.GUARD)
    assert op2.sync() == opened  # (the open reads the index, not the data blocks)
    sc2 = T.scan_device(op2, arena_cap=arena_bytes, op_cap=n, block_cap=nb, fill=M.CANARY, guard=M.GUARD)
    corrupt = dict(entries=0, arena_bytes=0, table_entries=0, table_bytes=0, data_blocks=nb, runs=0, reserved=0,
                   status=T.SCAN_CORRUPT)
    assert sc2.sync(check=False) == corrupt
    assert tail_is_canary(sc2.ops_t, 0) and tail_is_canary(sc2.arena_t, 0), "written to under a status"
    # the same flip in the prefix's image, by the host twin
    f4, o4, _, a4 = LC.scan_layout(po["val_len"])
    small = bytearray(image_p)
    at4 = int(o4[3] + a4[f4[4] - 1]) + 1
    assert small[at4] == 16
    small[at4] = 0xFF
    table_p, _ = T.open_host(bytes(small), handles=False)
    assert table_p["status"] == 0
    want_c = T.scan_host(bytes(small), table_p, arena_cap=1 << 17, op_cap=4000)[0]
    assert want_c == dict(corrupt, data_blocks=table_p["data_blocks"]) and T.scan_host(image_p, table_p)[0]["status"] == 0
    del table, buf, built, op, op2, sc, sc2, hurt, arena, vlen


# ---- combine_pieces_kernel ---------------------------------------------------------
def test_combine_pieces_second_trip(gpu, cus):
    """lv_crc32c_batch_strided over more split blocks than combine_pieces_kernel
    has waves: 16 KiB blocks, few enough that each is cut into pieces and too
    many pieces to be joined inside the walk, so the join kernel runs and its
    waves take a second block.  Seeded and masked, every CRC against the
    oracle."""
    import torch
    import lvgpu
    n = LT.size_for("combine_pieces_kernel", 2, cus, 903)
    _need("combine_pieces_kernel", n, cus, 2)
    blen = 16384
    t = torch.empty(n * blen + 64, dtype=torch.uint8, device=gpu)
    lvgpu.fill_splitmix(t, 0, 0xC0B1)
    seeds = np.random.default_rng(77).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    out = lvgpu.batch_strided(t, blen, blen, n, seed=torch.from_numpy(seeds.view(np.int32)).to(gpu), masked=True)
    kern = lvgpu.last_kernel()
    assert kern.endswith("+combine_pieces_kernel"), f"{n} blocks of {blen} bytes on {cus} compute units ran {kern}"
    got = out.cpu().numpy().view(np.uint32)
    host = t.cpu().numpy()
    L = W.lib()
    want = np.array([lvgpu.mask(L.oracle_extend(int(seeds[i]), host[i * blen:(i + 1) * blen].tobytes(), blen))
                     for i in range(n)], dtype=np.uint32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} CRCs differ, the first is block {int(bad[0])}"


# ---- hint_len_kernel ---------------------------------------------------------------
def test_hint_len_three_passes(gpu, cus):
    """lv_crc32c_batch_device_hint with LV_HINT_UNIFORM over eleven strides and
    300 lengths, laid end to end from arena offset 5 (not the aligned path):
    every thread of hint_len_kernel makes two passes of its unrolled loop and
    three tail iterations, the first 300 threads a third pass and no tail.  The
    clean call reports nothing and every CRC is the oracle's; one length of
    L - 1 at each kind of place in the two loops is reported as
    LV_HINT_ERR_NOT_UNIFORM and nothing else, and the word is cleared."""
    import torch
    import lvgpu
    n, stride = LT.hint_len_shape(cus, ragged=300)
    _need("hint_len_kernel", n, cus, 3)
    assert LT.trips("hint_len_kernel", n - 301, cus) == 3 and LT.trips("hint_len_kernel", n + 4 * stride, cus) == 4
    L = 40
    lens = np.full(n, L, dtype=np.uint32)
    offs = 5 + L * np.arange(n, dtype=np.uint64)
    a = torch.empty(5 + n * L + 16, dtype=torch.uint8, device=gpu)
    lvgpu.fill_splitmix(a, 0, 0x41E7)
    hint = lvgpu.hint_for(lens)
    assert hint.uniform == lvgpu.HINT_UNIFORM and hint.max_len == L and hint.total_bytes == n * L
    o = torch.from_numpy(offs.view(np.int64)).to(gpu)
    ln = torch.from_numpy(lens.view(np.int32)).to(gpu)
    lvgpu.batch_check()
    out = lvgpu.batch_hint(a, o, ln, hint, masked=True)
    assert lvgpu.last_kernel() == "hint_len_kernel+crc32c_classes_kernel"
    lvgpu.batch_check()
    got = out.cpu().numpy().view(np.uint32)
    want = np.zeros(n, dtype=np.uint32)
    host = a.cpu().numpy()
    W.lib().oracle_batch(host.ctypes.data, offs.ctypes.data, lens.ctypes.data, None, want.ctypes.data, n, 1)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} CRCs differ, the first is buffer {int(bad[0])}"
    t0 = stride // 2 + 77  # a thread with a tail, in a workgroup of the middle of the grid
    assert 300 <= t0 < stride
    lies = {t0 + (4 * u + s) * stride: ("unrolled", u, s) for u in (0, 1) for s in range(4)}
    lies.update({7 + 9 * stride: ("unrolled", 2, 1), n - 1: ("unrolled", 2, 3)})
    lies.update({t0 + (8 + k) * stride: ("tail", k, 0) for k in range(3)})
    lies.update({stride - 1: ("unrolled", 0, 0), stride: ("unrolled", 0, 1),         # either side of a stride
                 10 * stride - 1: ("tail", 1, 0), 10 * stride: ("unrolled", 2, 2)})  # ... and of one in the tail
    assert len(lies) == 17
    for i, place in sorted(lies.items()):
        assert 0 <= i < n and LT.hint_len_place(i, n, stride) == place, (i, place)
        ln[i] = L - 1
        lvgpu.batch_hint(a, o, ln, hint, masked=True, out=out)
        assert lvgpu.last_kernel() == "hint_len_kernel+crc32c_classes_kernel"
        with pytest.raises(lvgpu.HintViolation) as ei:
            lvgpu.batch_check()
        assert ei.value.violations == lvgpu.HINT_ERR_NOT_UNIFORM, (i, place, hex(ei.value.violations))
        ln[i] = L
        lvgpu.batch_hint(a, o, ln, hint, masked=True, out=out)
        lvgpu.batch_check()  # the word was cleared, and the lengths are the hint's again
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    del a, o, ln, out


def test_peak_device_memory(gpu, hash_case, wal_blocks):
    """The module stays under 4 GiB of device memory."""
    import torch
    print("peak device memory of the module:", torch.cuda.max_memory_allocated(gpu), "bytes")
    assert torch.cuda.max_memory_allocated(gpu) <= PEAK_LIMIT, torch.cuda.max_memory_allocated(gpu)
