"""The tilings of tests/loop_trips_cases.py against the Python models run on
three whole repetitions: what test_gpu_loop_trips.py expects of a tiled input
is what the model says of it.  No GPU."""
import numpy as np

import loop_trips_cases as LC
import write_batch_cases as C
from wal_decode_cases import oracle_read
from wal_encode_cases import B, oracle_encode


def test_write_batch_tiling_is_the_model_of_three_repetitions():
    payload, off, ln = LC.wb_motif()
    motif = C.model(payload, off, ln)
    st = motif[2]
    assert set(st.tolist()) == set(range(7))  # OK and each of the six ways a record is refused
    from lvgpu.write_batch import WB_SMALL
    assert (ln[st == C.OK] > WB_SMALL).any() and (ln[(st != C.OK) & (st != C.OUT_OF_RANGE)] > WB_SMALL).any()
    per = np.diff(motif[1].astype(np.int64))
    assert per.min() == 0 and per.max() >= 40 and len(st) == LC.WB_MOTIF
    for n in (3 * LC.WB_MOTIF, 2 * LC.WB_MOTIF + 300):
        p3, o3, l3 = LC.wb_tiled_inputs(payload, off, ln, n)
        want = C.model(p3, o3, l3)
        got = LC.wb_tiled(motif, len(payload), n)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert got[3] == want[3], (got[3], want[3])


def test_wal_tiling_is_the_model_of_three_repetitions():
    recs, log = LC.wal_motif()
    nb = len(log) // B
    assert nb % 2 == 1 and nb >= 37
    from wal_decode_cases import headers
    hs = headers(log)
    per_block = np.bincount([p // B for p, _, _ in hs], minlength=nb)
    assert per_block.min() == 1 and per_block.max() > 500
    types = {t for _, _, t in hs}
    assert types == {1, 2, 3, 4}
    ends = {(p + 7 + ln) % B for p, ln, _ in hs}
    assert any(B - 7 < e < B for e in ends if e)  # a tail shorter than a header
    # the encode side: the motif ends on a block boundary, so the log is periodic
    assert oracle_encode(recs * 3) == log * 3
    # the decode side, with a flip in the first and the last repetition
    t = LC.WalTiled(log, 3, {0: 1, 2: nb // 2})
    full = t.full_log().tobytes()
    assert full != log * 3
    want = oracle_read(full)
    pay, lens, offs, reps, dropped, at = t.expected()
    assert pay == b"".join(want[0]) and lens.tolist() == [len(r) for r in want[0]]
    assert offs.tolist() == want[1] and reps == want[2] and dropped == want[3]
    assert len(at) == 2 and [r for _, r in reps].count("checksum mismatch") == 2
    # a flip in any block leaves the Reader between records at the motif's end (a kill closes an open
    # record), so the repetitions stay independent: the last two blocks and the first
    for flips in ({0: nb - 1, 1: nb - 2}, {1: 0, 2: nb - 1}):
        t = LC.WalTiled(log, 3, flips)
        want = oracle_read(t.full_log().tobytes())
        pay, lens, offs, reps, dropped, at = t.expected()
        assert pay == b"".join(want[0]) and offs.tolist() == want[1] and reps == want[2] and dropped == want[3]


def test_scan_layout_is_the_model_build_of_a_prefix():
    """scan_ops is in memtable order and scan_layout places its blocks and
    entries where the Python table model does."""
    import memtable_cases as M
    import sst_build_cases as S
    n = 5000
    payload, ops = LC.scan_ops(n)
    assert M.model_order(payload, ops) == list(range(n))
    assert sorted(set(ops["val_len"].tolist())) == [0, 1, 2] and (ops["tag"] & 0xFF == 0).sum() == n // 7
    assert all(M.key_of(payload, o)[8 - int(o["val_len"]):] == payload[int(o["val_off"]):int(o["val_off"]) + int(o["val_len"])]
               for o in ops[:50])
    image, handles, tot = S.model_build(payload, ops, LC.SCAN_BLOCK, 1)
    first, boff, bsize, at = LC.scan_layout(ops["val_len"])
    assert tot["data_blocks"] == len(first) - 1 > 20 and len(set(np.diff(first).tolist())) > 2  # the counts drift
    assert [(int(o), int(s)) for o, s in zip(boff, bsize)] == handles[:-2]
    for blk in (0, 7, len(first) - 2):
        for i in (first[blk], first[blk] + 1, first[blk + 1] - 1):
            e = int(boff[blk] + at[i])
            key = M.key_of(payload, ops[i]) + int(ops["tag"][i]).to_bytes(8, "little")
            assert image[e:e + 19] == bytes([0, 16, int(ops["val_len"][i])]) + key, (blk, i)
    # a longer table begins with the same blocks: all of the prefix's but its last
    f2, o2, s2, _ = LC.scan_layout(LC.scan_ops(n + 999)[1]["val_len"])
    k = len(first) - 2
    assert np.array_equal(f2[:k + 1], first[:k + 1]) and np.array_equal(o2[:k], boff[:k]) and np.array_equal(s2[:k], bsize[:k])


def test_bloom_big_items_crowd_their_windows():
    import loop_trips as LT
    import sst_bloom_cases as SB
    from lvgpu.table import SB_BLOOM_LDS
    from memtable_cases import make_table
    crowded = {3, 40}
    items, where = LC.bloom_big_items(60, crowded)
    assert [k for k, _, _ in items] == sorted({k for k, _, _ in items}) and len(items) == 60 + 2 * LC.BLOOM_BIG_CROWD
    payload, ops = make_table(items)
    image, handles, tot, btot = SB.model_build(payload, ops, 64, LC.BLOOM_BIG_BLOCK, 16)
    assert tot["data_blocks"] == 60  # a crowded block holds its big entry too
    assert sorted(where) == sorted(crowded) and all(items[at + k - 1][2] and not items[at][2] for at, k in where.values())
    assert len(SB.create_filter([b"k"], 64)) == 9  # a one-entry block's filter: 64 bits and the k byte
    assert len(SB.create_filter([k for k, _, _ in items[:LC.BLOOM_BIG_CROWD + 1]], 64)) > SB_BLOOM_LDS + 1


def test_bloom_items_spread_their_blocks_over_the_windows():
    import loop_trips as LT
    import sst_bloom_cases as SB
    from memtable_cases import make_table
    n = LT.size_for("sb_bloom_emit", 3, 256, 7)
    items = LC.bloom_items(n)
    assert len(items) == n and [k for k, _, _ in items] == sorted({k for k, _, _ in items})
    payload, ops = make_table(items)
    image, handles, tot, btot = SB.model_build(payload, ops, 10, 1, 16)
    assert tot["data_blocks"] == n and btot["filter_keys"] == n
    starts = np.bincount([o >> SB.BASE_LG for o, _ in handles[:n]], minlength=btot["filters"])
    assert starts.min() == 0 and starts[starts > 0].min() == 1 and starts.max() >= 35
    # a wave takes blocks w, w + 4096, ...: some wave's later filter is smaller than its earlier one
    first = np.nonzero(np.diff(np.concatenate([[-1], [o >> SB.BASE_LG for o, _ in handles[:n]]])))[0]
    keys = {int(b): int(starts[handles[b][0] >> SB.BASE_LG]) for b in first}
    shrinks = sum(1 for b, k in keys.items() for later in (b + 4096, b + 8192) if later in keys and keys[later] < k)
    assert shrinks > 10
