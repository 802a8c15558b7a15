"""lv_write_batch_encode_device on the GPU against the Python model
(tests/write_batch_encode_cases.py), byte for byte and canary for canary:
record shapes, op counts around the scan tile and the carry's rounds, every
alignment of source and destination, every copy class, overlapping extents,
every status, one value of 2^28 bytes, streams, and the two chains the stage
exists for: back through lv_write_batch_decode_device, and through the WAL
stages to the memtable against the memtable built straight from d_ops_out."""
import numpy as np
import pytest

import lvgpu.write_batch as WB
import write_batch_cases as C
import write_batch_encode_cases as E
from write_batch_cases import M64
from write_batch_encode_cases import check, pool_table, short_len, table

pytestmark = pytest.mark.gpu

T, W, LANES = WB.WE_TILE, WB.WE_WAVE_COPY, WB.WE_COPY_LANES

SHAPES = {
    "no_records": [],
    "one_empty": [0],
    "empty_first": [0, 3, 1],
    "empty_last": [2, 5, 0],
    "three_empty_in_a_row": [4, 0, 0, 0, 1, 2],
    "only_empties": [0, 0, 0, 0],
    "mixed": [1, 0, 7, 1, 1, 0, 30, 2],
}


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("lead", [0, 5])
def test_record_shapes(gpu, name, lead):
    """Empty records wherever they can lie, and d_rec_op[0] != 0: the ops in
    front of the first record have types and extents no check accepts."""
    import torch
    src, ops, rec_op = pool_table(SHAPES[name], short_len, seed=len(name), lead=lead)
    r = check(torch, gpu, src, ops, rec_op, first_sequence=500, tag=name)
    t = r.want[4]
    assert t["status"] == 0 and t["records"] == len(SHAPES[name]) and t["ops"] == sum(SHAPES[name])
    assert t["out_bytes"] >= 12 * t["records"] and int(rec_op[0]) == lead


def test_fewer_records_than_capacity_and_upstream(gpu):
    import torch
    src, ops, rec_op = pool_table([2, 0, 3, 1, 4], short_len, seed=2, lead=1)
    # *d_records = 3 of the 5 the arrays could hold, op_cap beyond the ops
    r = check(torch, gpu, src, ops, rec_op, first_sequence=9, records=3, rec_cap=5, op_cap=len(ops), tag="3 of 5")
    assert r.want[4]["records"] == 3 and r.want[4]["ops"] == 5
    # a zero upstream status changes nothing; a set one gives the totals of zero records
    check(torch, gpu, src, ops, rec_op, first_sequence=9, upstream=0, tag="upstream 0")
    r = check(torch, gpu, src, ops, rec_op, first_sequence=9, upstream=4, tag="upstream 4")
    assert r.want[4] == dict(records=0, ops=0, key_bytes=0, value_bytes=0, out_bytes=0, last_sequence=8,
                             status=E.UPSTREAM, bad_record=M64, bad_op=M64)
    with pytest.raises(WB.LvError, match="UPSTREAM"):
        r.enc.sync_totals()
    # *d_records = rec_cap + 1
    r = check(torch, gpu, src, ops, rec_op, first_sequence=9, records=5, rec_cap=4, tag="rec_over")
    assert r.want[4]["status"] == E.REC_OVER and r.want[4]["records"] == 5 and r.want[4]["ops"] == 0


def test_without_an_op_table(gpu):
    """d_ops_out == NULL: the bytes and the record arrays alone."""
    import torch
    src, ops, rec_op = pool_table([3, 0, 70, 1], short_len, seed=8)
    r = check(torch, gpu, src, ops, rec_op, first_sequence=3, want_ops=False, tag="no ops_out")
    assert r.enc.ops_t is None and r.want[4]["ops"] == 74


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 64 * T + 1, 2 * 64 * T + 1])
@pytest.mark.parametrize("shape", ["single_op_records", "one_record", "mixed_records"])
def test_tile_edges(gpu, n, shape):
    """Op counts around one scan tile and in the carry's second and third
    round (64 tiles a round), as single-op records, as one record, and as that
    many records, empty and not."""
    import torch
    if shape == "single_op_records":
        counts = [1] * n
    elif shape == "one_record":
        counts = [n]
    else:
        counts = [(0, 2, 0, 3, 2, 0, 0, 2)[i % 8] for i in range(n)]  # at least n ops: the same rounds
    lens = (lambda rng: rng.randrange(0, 9)) if n > 4 * T else short_len
    src, ops, rec_op = pool_table(counts, lens, seed=n % 1000, lead=n % 3)
    r = check(torch, gpu, src, ops, rec_op, first_sequence=(1 << 40) + n, tag=f"{shape} n={n}")
    t = r.want[4]
    assert t["status"] == 0 and t["records"] == len(counts) and t["ops"] == sum(counts)
    assert t["ops"] == n if shape != "mixed_records" else n <= t["ops"] < n + n // 4
    if n > 2 * 64 * T:
        assert (t["ops"] + T - 1) // T > 128  # a third round of the carry


def mixed_small_table(seed):
    return pool_table([2, 0, 5, 1, 9, 0, 1], lambda rng: rng.choice([0, 1, 3, 15, 16, 17, 40, W - 1, W, W + 1, 200]),
                      seed=seed)


@pytest.mark.parametrize("a", range(16))
def test_alignment(gpu, a):
    """d_out and d_src each at every shift past a 16-B boundary."""
    import torch
    src, ops, rec_op = mixed_small_table(a)
    check(torch, gpu, src, ops, rec_op, first_sequence=77, out_shift=a, src_shift=(7 * a + 3) % 16, tag=f"a={a}")


COPY_LENGTHS = (0, 1, 15, 16, 17, W - 1, W, W + 1, 4096, 65537)


def copy_class_table():
    """Every length as a key and as a value, then a wave of nothing but long
    copies (64 / WE_COPY_LANES of them run at a time: group_copy's loop goes
    round sixteen times)."""
    rng = np.random.default_rng(31)
    blob = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    rec = []
    for n in COPY_LENGTHS:
        rec += [(blob(n), b"v3v"), (b"k2", blob(n)), (blob(n), None), (blob(n), blob(n))]
    long_wave = [(blob(W + 20 + i % 7), blob(3 * W + i)) for i in range(70)]
    return table([rec, [], long_wave])


@pytest.mark.parametrize("a", range(16))
def test_copy_classes_on_every_destination_alignment(gpu, a):
    """Lengths below, at and above the wave-copy threshold, 4 KiB and 64 KiB +
    1, as key and as value; the 16 shifts of d_out put each on all 16
    destination alignments."""
    import torch
    src, ops, rec_op = copy_class_table()
    assert 70 > 64 // LANES
    r = check(torch, gpu, src, ops, rec_op, first_sequence=1, out_shift=a, src_shift=(5 * a + 1) % 16, tag=f"a={a}")
    assert r.want[4]["status"] == 0


def test_a_wave_whose_only_long_copy_is_a_value(gpu):
    """64 ops, the first wave of the grid: every key short, one value long."""
    import torch
    rec = [(b"k%02d" % i, b"v" * (i % 9)) for i in range(64)]
    rec[37] = (b"k37", bytes(range(256)) * 3)
    src, ops, rec_op = table([rec])
    for a in (0, 9):
        check(torch, gpu, src, ops, rec_op, first_sequence=1, out_shift=a, tag=f"a={a}")
    # ... and one whose only long copy is a key
    rec[37] = (bytes(range(250)), b"")
    check(torch, gpu, *table([rec]), first_sequence=1, tag="key")


def test_overlapping_and_repeated_extents(gpu):
    import torch
    src = bytes(range(256)) * 40
    dt = WB.OP_DTYPE
    rows = [(1, 10, 12, 20, 100), (1, 10, 10, 20, 20), (0, 0, 0, 200, 0), (1, 199, 0, 1, 200),
            (1, 0, 0, len(src), len(src)), (1, 5, 6, 5000, 5000), (0, 5, 0, 5000, 0)]
    rows += [(1, 100, 100, 300, 300)] * 20
    ops = np.array(rows, dtype=dt)
    r = check(torch, gpu, src, ops, np.array([0, 2, 4, 7, len(rows)], dtype=np.uint64), first_sequence=5, tag="overlap")
    assert r.want[4]["out_bytes"] > 2 * len(src)


STATUS = list(E.status_cases())


@pytest.mark.parametrize("name", [c[0] for c in STATUS])
def test_status_cases(gpu, name):
    """Every status at its smallest input: the totals alone are written, every
    other array still holds the canary (check() compares them all)."""
    import torch
    _, src, ops, rec_op, op_cap, out_cap, status = next(c for c in STATUS if c[0] == name)
    r = check(torch, gpu, src, ops, rec_op, first_sequence=77, op_cap=op_cap, out_cap=out_cap, tag=name)
    assert r.want[4]["status"] == status
    if status:
        with pytest.raises(WB.LvError, match=WB.ENCODE_STATUS[status]):
            r.enc.sync_totals()


def test_bad_op_among_many_is_the_lowest(gpu):
    """Bad ops in several tiles: bad_op is the lowest index, bad_record its
    record; bad bounds in several workgroups likewise."""
    import torch
    counts = [(1, 0, 2, 5)[i % 4] for i in range(3000)]
    src, ops, rec_op = pool_table(counts, short_len, seed=4, lead=2)
    for i in (5000, 2345, 4999):
        ops[i]["key_off"] = len(src) + 1
    ops[2600]["tag"] = 2
    r = check(torch, gpu, src, ops, rec_op, first_sequence=1, tag="bad ops")
    t = r.want[4]
    assert t["status"] == E.BAD_OP and t["bad_op"] == 2345
    assert int(rec_op[t["bad_record"]]) <= 2345 < int(rec_op[t["bad_record"] + 1])
    bad = rec_op.copy()
    bad[2900], bad[700], bad[1500] = 0, M64, 3
    r = check(torch, gpu, src, ops, bad, first_sequence=1, tag="bad bounds")
    assert r.want[4]["status"] == E.BAD_BOUNDS and r.want[4]["bad_record"] == 699


def test_out_over_then_the_reported_size(gpu):
    import torch
    src, ops, rec_op = pool_table([3, 1, 0, 40, 2], lambda rng: rng.randrange(0, 300), seed=6)
    r = check(torch, gpu, src, ops, rec_op, first_sequence=10, out_cap=100, tag="short")
    t = r.enc.sync_totals(check=False)
    assert t["status"] == E.OUT_OVER and t["out_bytes"] > 100
    assert t["out_bytes"] <= WB.encode_bound(t["records"], t["ops"], t["key_bytes"], t["value_bytes"])
    r2 = check(torch, gpu, src, ops, rec_op, first_sequence=10, out_cap=t["out_bytes"], tag="again")
    assert r2.enc.sync_totals() == dict(t, status=0)


def test_one_value_of_2_28_bytes(gpu):
    """The first five-byte length, copied by one group of lanes: the header and
    the varint bytes exactly, the body compared on the device."""
    import torch
    n = 1 << 28
    g = torch.Generator(device=gpu)
    g.manual_seed(5)
    src = torch.randint(0, 256, (n + 3,), dtype=torch.uint8, device=gpu, generator=g)
    ops = np.array([((9 << 8) | 1, n, 1, 3, n)], dtype=WB.OP_DTYPE)
    head_len = 12 + 1 + 1 + 3 + 5
    enc = WB.encode_device(src, E.dev_ops(torch, gpu, ops), C.dev_i64(torch, gpu, [0, 1]), C.dev_i64(torch, gpu, [1]),
                           first_sequence=(1 << 56) + 5, out_cap=head_len + n, fill=C.CANARY, guard=C.GUARD)
    t = enc.sync_totals()
    assert t == dict(records=1, ops=1, key_bytes=3, value_bytes=n, out_bytes=head_len + n,
                     last_sequence=(1 << 56) + 5, status=0, bad_record=M64, bad_op=M64)
    head = enc.out_t[:head_len].cpu().numpy().tobytes()
    key = src[n:n + 3].cpu().numpy().tobytes()
    assert head == ((1 << 56) + 5).to_bytes(8, "little") + (1).to_bytes(4, "little") + bytes([1, 3]) + key + \
        bytes([0x80, 0x80, 0x80, 0x80, 0x01])
    assert torch.equal(enc.out_t[head_len:head_len + n], src[1:1 + n])
    assert C.tail_is_canary(enc.out_t, head_len + n)
    o = enc.ops()[0]
    assert (int(o["tag"]), int(o["key_off"]), int(o["key_len"]), int(o["val_off"]), int(o["val_len"])) == \
        (((((1 << 56) + 5) << 8) | 1) & M64, 14, 3, head_len, n)
    assert enc.rec_off().tolist() == [0] and enc.rec_len().tolist() == [head_len + n]


def test_streams(gpu):
    """A non-default stream; two calls back to back on two streams, each with
    its own workspace."""
    import torch
    a = pool_table([5, 0, 300, 2], lambda rng: rng.randrange(0, 200), seed=11)
    b = pool_table([1] * 1500, short_len, seed=12, lead=3)
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        ra = E.run(torch, gpu, *a, first_sequence=100, stream=s1)
    with torch.cuda.stream(s2):
        rb = E.run(torch, gpu, *b, first_sequence=200, stream=s2)
    with torch.cuda.stream(s1):
        rc = E.run(torch, gpu, *b, first_sequence=300, out_shift=3, stream=s1)
    s1.synchronize()
    s2.synchronize()
    for r, tag in ((ra, "a on s1"), (rb, "b on s2"), (rc, "b on s1")):
        E.compare(r, tag)


def test_chain_back_through_the_decode(gpu):
    """encode -> lv_write_batch_decode_device over (d_out, d_rec_off,
    d_rec_len, &totals->records): the ops are d_ops_out, the bounds d_rec_op -
    d_rec_op[0], every status LV_WB_OK, and the totals agree."""
    import torch
    counts = [(1, 0, 3, 1, 40, 2, 0, 1)[i % 8] for i in range(700)]
    src, ops, rec_op = pool_table(counts, lambda rng: rng.choice([0, 2, 9, 30, W, 300, 5000]), seed=21, lead=4)
    first = (1 << 56) - 1000  # the tags wrap inside the call
    r = E.run(torch, gpu, src, ops, rec_op, first_sequence=first)
    enc = r.enc
    dec = WB.decode_device(enc.out_t, enc.rec_off_t, enc.rec_len_t, enc.totals[0:1], enc.totals[6:7],
                           rec_cap=len(counts), op_cap=len(ops), fill=C.CANARY, guard=C.GUARD)
    E.compare(r, "encode")
    t, d = enc.sync_totals(), dec.sync_totals()
    assert d["status"] == 0 and d["bad_records"] == 0
    assert all(d[k] == t[k] for k in ("records", "ops", "key_bytes", "value_bytes"))
    assert (dec.statuses() == WB.OK).all()
    assert np.array_equal(dec.record_bounds(), rec_op - rec_op[0])
    assert (dec.ops() == enc.ops()).all()
    # ... and the decoded table feeds the encode as it is: the same bytes again
    r2 = E.run(torch, gpu, r.want[0], dec.ops(), dec.record_bounds(), first_sequence=first)
    E.compare(r2, "re-encode")
    assert r2.want[0] == r.want[0]


def test_chain_to_the_memtable_both_ways(gpu):
    """A commit group of a few thousand ops: encode; the host lengths from the
    sizing call; lv_wal_encode_device -> scan -> decode ->
    lv_write_batch_decode_device -> memtable build and get; and the memtable
    build and get straight over (d_out, d_ops_out).  Both answer every query
    as lv_memtable_get_host does over the model's bytes and ops."""
    import torch
    import lvgpu.memtable as MT
    import lvgpu.wal as LW
    import memtable_cases as M
    rng = np.random.default_rng(77)
    recs = []
    for r in range(900):
        rec = []
        for _ in range(int(rng.integers(0, 7))):
            key = b"user-key-%04d" % int(rng.integers(0, 500))
            rec.append((key, None if rng.random() < 0.2 else bytes(rng.integers(0, 256, size=int(rng.integers(0, 90)),
                                                                                  dtype=np.uint8))))
        recs.append(rec)
    recs[450].append((b"user-key-big", bytes(rng.integers(0, 256, size=70000, dtype=np.uint8))))
    src, ops, rec_op = table(recs, lead=2)
    first = 1000
    r = E.run(torch, gpu, src, ops, rec_op, first_sequence=first)
    enc = r.enc
    _, off_h, ln_h, _, tot_h = WB.encode_host(None, ops, rec_op, first, sizing=True, src_bytes=len(src))
    assert tot_h["status"] == 0 and 2000 < tot_h["ops"] < 6000
    need, frags = LW.encode_size(ln_h)
    assert need > 3 * 32768
    log_t = LW.encode_device(enc.out_t, off_h, ln_h)
    scan = LW.scan_device(log_t, frags + 8)
    dec = LW.decode_device(log_t, *scan, scan_cap=frags + 8)
    dops = WB.decode_device(dec.payload, dec.rec_off, dec.rec_len, dec.totals[0:1], dec.totals[4:5],
                            rec_cap=frags + 8, op_cap=len(ops))
    tab_log = MT.build_device(dec.payload, dops.ops_t, dops.totals[1:2], dops.totals[6:7], op_cap=dops.op_cap)
    tab_direct = MT.build_device(enc.out_t, enc.ops_t, enc.totals[1:2], enc.totals[6:7], op_cap=enc.op_cap)
    E.compare(r, "encode")
    w_out, _, _, w_ops, w_tot = r.want
    assert enc.sync_totals() == tot_h == w_tot and dops.sync_totals()["ops"] == w_tot["ops"]
    order, mt_tot = MT.build_host(w_out, w_ops)
    assert tab_log.sync_totals() == tab_direct.sync_totals() == mt_tot
    queries = M.queries_for(w_out, w_ops[:: 7])[:3000] + [(b"user-key-big", first + 10 ** 6), (b"absent", 5)]
    packed = M.pack_queries(queries)
    got_log = M.run_get(torch, gpu, tab_log, *packed)
    got_direct = M.run_get(torch, gpu, tab_direct, *packed)
    assert (got_log == got_direct).all()
    found = 0
    for i, (key, seq) in enumerate(queries):
        want = MT.get_host(w_out, w_ops, order, mt_tot, key, seq)
        g = {k: int(got_direct[i][k]) for k in want}
        assert g == want, (i, key, seq, g, want)
        found += want["status"] == 1
    assert found > 100
