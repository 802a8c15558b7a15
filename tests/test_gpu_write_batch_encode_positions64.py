"""lv_write_batch_encode_device with positions beyond 4 GiB, by the technique
of positions64_cases.py.

Source: the arena is a HIGH WINDOW laid across position 2^32 of a tensor that
is otherwise not initialised, with the complement of the window where a
position cut to 32 bits would land; the model runs on the local layout.

Output: about 4,100 Puts whose 1 MiB values are shifted windows of one arena of
1 MiB + 4,100 bytes, so d_out crosses 4 GiB while no host holds it; a few small
records follow.  The rows are compared on the device against an unfolded view
of the arena, the small tail and every offset against the model's arithmetic.

Each test asserts that the u64 quantity it is about exceeded 2^32 and frees its
tensors before it returns."""
import gc

import numpy as np
import pytest

import lvgpu.write_batch as WB
import positions64_cases as P
import write_batch_cases as C
import write_batch_encode_cases as E
from positions64_cases import HI
from write_batch_cases import CANARY, GUARD, M64, VALUE

pytestmark = pytest.mark.gpu


def _free(torch):
    gc.collect()
    torch.cuda.empty_cache()


def _dirty(torch, gpu, nbytes):
    return torch.full((max(nbytes, 16),), 0x5A, dtype=torch.uint8, device=gpu)


def test_source_above_the_line(gpu):
    """key_off / val_off beyond 2^32 for T + 9 ops, a key and a value across
    the line; a position cut to 32 bits would read the complement."""
    import torch
    rng = np.random.default_rng(64)
    blob = lambda n: rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes()
    recs, n = [], WB.WE_TILE + 9
    while sum(len(r) for r in recs) < n:
        recs.append([(blob(rng.integers(1, 30)), None if rng.random() < 0.25 else blob(rng.choice([0, 7, 40, 100, 300])))
                     for _ in range(int(rng.integers(0, 6)))])
    src, ops, rec_op = E.table(recs)
    ops["val_off"][(ops["tag"] & 0xFF) != VALUE] = 0  # (a DELETION's are not read: keep the rebase from wrapping)
    mid = len(ops) // 2
    j = next(i for i in range(mid, len(ops)) if int(ops[i]["tag"]) & 0xFF == VALUE and int(ops[i]["val_len"]) >= 40)
    cut = int(ops[j]["val_off"]) + 20  # inside a long value
    k = next(i for i in range(j + 1, len(ops)) if int(ops[i]["key_len"]) >= 8)
    ops[k]["key_off"], ops[k]["key_len"] = cut - 3, 8  # and a key across the line
    want = E.model(src, ops, rec_op, len(recs), 1 << 33, len(ops))
    assert want[4]["status"] == 0 and want[4]["ops"] >= n
    assert min(P.sides(ops["key_off"], ops["key_len"], cut)) >= 1
    t, base = P.high_window(torch, gpu, src, cut, P.complement(src))
    arena = t[: base + len(src)]
    high = P.rebase(ops, base)
    assert int(high["key_off"].max()) > HI and int(high["key_off"].min()) < HI and base < HI < base + len(src)
    out_cap = want[4]["out_bytes"]
    buf, d_out, out_base = E.guarded_out(torch, gpu, out_cap, 5)
    enc = WB.encode_device(arena, E.dev_ops(torch, gpu, high), C.dev_i64(torch, gpu, rec_op),
                           C.dev_i64(torch, gpu, [len(recs)]), first_sequence=1 << 33, out=d_out, out_cap=out_cap,
                           workspace=_dirty(torch, gpu, WB.encode_workspace_bytes(len(recs), len(ops))),
                           fill=CANARY, guard=GUARD)
    assert enc.sync_totals() == want[4]
    host = buf.cpu().numpy()
    assert host[out_base:out_base + out_cap].tobytes() == want[0]
    assert (host[:out_base] == CANARY).all() and (host[out_base + out_cap:] == CANARY).all()
    assert (enc.ops() == want[3]).all() and np.array_equal(enc.rec_off(), want[1]) and np.array_equal(enc.rec_len(), want[2])
    del enc, arena, t, buf, d_out
    _free(torch)


def test_output_above_the_line(gpu):
    """d_out beyond 2^32: 41 records of 100 Puts of a 1 MiB value, then three
    small records whose bytes, extents and op offsets all lie above the line."""
    import torch
    V, PER, NREC, KL = 1 << 20, 100, 41, 8
    NBIG = PER * NREC
    ENTRY = 1 + 1 + KL + 3 + V  # type, varint(8), key, varint(2^20), value
    REC = 12 + PER * ENTRY
    BIG = NREC * REC
    assert NBIG * V > HI and len(C.varint(V)) == 3
    first = (1 << 56) - 2000  # the tags wrap in the 56-bit sequence on the way
    g = torch.Generator(device=gpu)
    g.manual_seed(11)
    tail_src = np.random.default_rng(3).integers(0, 256, size=600, dtype=np.uint8).tobytes()
    arena = torch.empty(V + NBIG + len(tail_src), dtype=torch.uint8, device=gpu)
    arena[: V + NBIG] = torch.randint(0, 256, (V + NBIG,), dtype=torch.uint8, device=gpu, generator=g)
    arena[V + NBIG:].copy_(torch.frombuffer(bytearray(tail_src), dtype=torch.uint8))
    idx = np.arange(NBIG, dtype=np.uint64)
    ops = np.zeros(NBIG, dtype=WB.OP_DTYPE)
    ops["tag"], ops["key_off"], ops["key_len"], ops["val_off"], ops["val_len"] = VALUE, idx + 3, KL, idx, V
    # the small tail: its own little table over the arena's last 600 bytes
    dt = WB.OP_DTYPE
    small = np.array([(1, 0, 10, 12, 100), (0, 50, 0, 20, 0), (1, 100, 130, 30, 300), (1, 7, 7, 0, 0), (0, 400, 0, 200, 0),
                      (1, 590, 0, 10, 600)], dtype=dt)
    small_bounds = np.array([0, 2, 2, 5, 6], dtype=np.uint64)
    tail = E.model(tail_src, small, small_bounds, 4, first + NBIG, len(small))
    assert tail[4]["status"] == 0
    all_ops = np.concatenate([ops, P.rebase(small, V + NBIG)])
    rec_op = np.concatenate([np.arange(0, NBIG + 1, PER, dtype=np.uint64), small_bounds[1:] + np.uint64(NBIG)])
    records = NREC + 4
    out_bytes = BIG + tail[4]["out_bytes"]
    assert out_bytes > HI and BIG > HI
    buf, d_out, out_base = E.guarded_out(torch, gpu, out_bytes, 7)
    enc = WB.encode_device(arena, E.dev_ops(torch, gpu, all_ops), C.dev_i64(torch, gpu, rec_op),
                           C.dev_i64(torch, gpu, [records]), first_sequence=first, out=d_out, out_cap=out_bytes,
                           workspace=_dirty(torch, gpu, WB.encode_workspace_bytes(records, len(all_ops))),
                           fill=CANARY, guard=GUARD)
    t = enc.sync_totals()
    assert t == dict(records=records, ops=NBIG + 6, key_bytes=NBIG * KL + tail[4]["key_bytes"],
                     value_bytes=NBIG * V + tail[4]["value_bytes"], out_bytes=out_bytes,
                     last_sequence=(first - 1 + NBIG + 6) & M64, status=0, bad_record=M64, bad_op=M64)
    # the guards around d_out, whose used part ends above the line
    assert bool((buf[:out_base] == CANARY).all()) and bool((buf[out_base + out_bytes:] == CANARY).all())
    # the big records on the device: headers, entry heads, values
    rows = d_out[:BIG].view(NREC, REC)
    heads = np.zeros((NREC, 12), dtype=np.uint8)
    for r in range(NREC):
        heads[r] = np.frombuffer(((first + r * PER) & M64).to_bytes(8, "little") + PER.to_bytes(4, "little"), dtype=np.uint8)
    assert torch.equal(rows[:, :12], torch.from_numpy(heads).to(gpu))
    entries = rows[:, 12:].reshape(NREC, PER, ENTRY)
    keys = arena.unfold(0, KL, 1)    # keys[i] = arena[i : i + 8]
    values = arena.unfold(0, V, 1)   # values[i] = arena[i : i + 2^20], no copy
    lead = torch.tensor([1, KL], dtype=torch.uint8, device=gpu)
    vint = torch.tensor(list(C.varint(V)), dtype=torch.uint8, device=gpu)
    for r in range(NREC):
        e = entries[r]
        assert bool((e[:, :2] == lead).all()) and bool((e[:, 2 + KL:5 + KL] == vint).all()), r
        assert torch.equal(e[:, 2:2 + KL], keys[3 + r * PER:3 + (r + 1) * PER]), r
        assert torch.equal(e[:, 5 + KL:], values[r * PER:(r + 1) * PER]), r
    # the small tail, read back: every byte above the line
    assert d_out[BIG:].cpu().numpy().tobytes() == tail[0]
    # extents and op offsets against the model's arithmetic
    want_off = np.concatenate([np.arange(NREC, dtype=np.uint64) * np.uint64(REC), tail[1] + np.uint64(BIG)])
    want_len = np.concatenate([np.full(NREC, REC, dtype=np.uint64), tail[2]])
    assert np.array_equal(enc.rec_off(), want_off) and np.array_equal(enc.rec_len(), want_len)
    got = enc.ops()
    key_off = (idx // np.uint64(PER)) * np.uint64(REC) + np.uint64(12) + (idx % np.uint64(PER)) * np.uint64(ENTRY) + np.uint64(2)
    want_big = np.zeros(NBIG, dtype=dt)
    want_big["tag"] = (((np.uint64(first) + idx) & np.uint64((1 << 56) - 1)) << np.uint64(8)) | np.uint64(VALUE)
    want_big["key_off"], want_big["key_len"] = key_off, KL
    want_big["val_off"], want_big["val_len"] = key_off + np.uint64(KL + 3), V
    assert (got[:NBIG] == want_big).all()
    assert (got[NBIG:] == P.rebase(tail[3], BIG)).all()
    assert int(got["key_off"].max()) > HI and int((got["val_off"] > HI).sum()) > 6
    del enc, rows, entries, keys, values, buf, d_out, arena
    _free(torch)
