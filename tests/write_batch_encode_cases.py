"""The model, the case generators and the comparison helper of the WriteBatch
encode tests (test_write_batch_encode.py, test_gpu_write_batch_encode_*.py).

model() builds every record with write_batch_cases.WriteBatch, whose put /
delete / set_sequence restate write_batch.rs:57-78: it is what every output of
lv_write_batch_encode_host and lv_write_batch_encode_device is compared with,
byte for byte."""
import numpy as np

import write_batch_cases as C
from write_batch_cases import CANARY, DELETION, GUARD, M64, VALUE, WriteBatch, varint

UPSTREAM, REC_OVER, BAD_BOUNDS, BAD_OP, OUT_OVER = 1, 2, 4, 8, 16
TOTALS = ("records", "ops", "key_bytes", "value_bytes", "out_bytes", "last_sequence", "status", "bad_record", "bad_op")


def _dtype():
    from lvgpu.write_batch import OP_DTYPE
    return OP_DTYPE


def _ok(off, ln, n):
    return off <= n and ln <= n - off


def model(src, ops, rec_op, records, first_sequence, op_cap, out_cap=None, *, rec_cap=None, upstream=0):
    """(out bytes, rec_off, rec_len, ops_out, totals) of one call.  With a
    status the first four are None: only the totals are written.  The statuses
    are judged in the header's order: UPSTREAM, REC_OVER, BAD_BOUNDS, BAD_OP,
    OUT_OVER (out_cap None: ample)."""
    tot = dict(records=0, ops=0, key_bytes=0, value_bytes=0, out_bytes=0, last_sequence=(first_sequence - 1) & M64,
               status=0, bad_record=M64, bad_op=M64)
    if upstream:
        return None, None, None, None, dict(tot, status=UPSTREAM)
    if rec_cap is not None and records > rec_cap:
        return None, None, None, None, dict(tot, status=REC_OVER, records=records)
    tot["records"] = records
    b = [int(x) for x in rec_op[: records + 1]]
    for r in range(records):
        if not b[r] <= b[r + 1] <= op_cap:
            return None, None, None, None, dict(tot, status=BAD_BOUNDS, bad_record=r)
    n = len(src)
    for r in range(records):
        for i in range(b[r], b[r + 1]):
            o = ops[i]
            typ = int(o["tag"]) & 0xFF
            if typ > VALUE or not _ok(int(o["key_off"]), int(o["key_len"]), n) or \
                    (typ == VALUE and not _ok(int(o["val_off"]), int(o["val_len"]), n)):
                return None, None, None, None, dict(tot, status=BAD_OP, bad_record=r, bad_op=i)
    src = bytes(src)
    out, rec_off, rec_len, ops_out = bytearray(), [], [], []
    kb = vb = 0
    base = b[0] if records else 0
    for r in range(records):
        wb = WriteBatch()
        for i in range(b[r], b[r + 1]):
            o = ops[i]
            typ, ko, kl = int(o["tag"]) & 0xFF, int(o["key_off"]), int(o["key_len"])
            at = len(out) + len(wb.rep)
            tag = ((((first_sequence + i - base) & M64) << 8) | typ) & M64
            key_off = at + 1 + len(varint(kl))
            kb += kl
            if typ == VALUE:
                vo, vl = int(o["val_off"]), int(o["val_len"])
                wb.put(src[ko:ko + kl], src[vo:vo + vl])
                vb += vl
                ops_out.append((tag, key_off, key_off + kl + len(varint(vl)), kl, vl))
            else:
                wb.delete(src[ko:ko + kl])
                ops_out.append((tag, key_off, key_off + kl, kl, 0))
        wb.set_sequence(first_sequence + b[r] - base)
        assert wb.count == b[r + 1] - b[r]
        rec_off.append(len(out))
        rec_len.append(len(wb.rep))
        out += wb.rep
    nops = len(ops_out)
    tot.update(ops=nops, key_bytes=kb, value_bytes=vb, out_bytes=len(out), last_sequence=(first_sequence - 1 + nops) & M64)
    assert len(out) <= 12 * records + 11 * nops + kb + vb
    if out_cap is not None and len(out) > out_cap:
        return None, None, None, None, dict(tot, status=OUT_OVER)
    arr = np.array(ops_out, dtype=_dtype()) if ops_out else np.zeros(0, dtype=_dtype())
    return bytes(out), np.array(rec_off, dtype=np.uint64), np.array(rec_len, dtype=np.uint64), arr, tot


# ---- generators ----
POOL = np.random.default_rng(4242).integers(0, 256, size=(1 << 17) + (1 << 16), dtype=np.uint8).tobytes()


def table(recs, *, lead=0, seed=1, src=None):
    """(src, ops, rec_op) for recs = [[(key, value or None), ...], ...]: the
    keys and values laid end to end in an arena (or, with src given, found in
    it: every key and value must occur there).  `lead` ops that belong to no
    record come first, with a type and extents no check would accept:
    d_rec_op[0] = lead.  The upper 56 bits of every tag are noise, and a
    DELETION's value fields are wild."""
    rng = np.random.default_rng(seed)
    arena = bytearray() if src is None else None
    rows = [((int(rng.integers(1 << 56)) << 8) | 7, M64 - 5, M64 - 9, 77, 99) for _ in range(lead)]
    bounds = [lead]

    def place(b):
        if arena is None:
            at = src.find(b)
            assert at >= 0
            return at
        at = len(arena)
        arena.extend(b)
        return at
    for rec in recs:
        for key, value in rec:
            noise = int(rng.integers(1 << 56)) << 8
            ko = place(key)
            if value is None:
                rows.append((noise | DELETION, ko, M64 - int(rng.integers(1 << 20)), len(key), 0xFFFFFFFF))
            else:
                rows.append((noise | VALUE, ko, place(value), len(key), len(value)))
        bounds.append(len(rows))
    ops = np.array(rows, dtype=_dtype()) if rows else np.zeros(0, dtype=_dtype())
    return (bytes(arena) if src is None else src), ops, np.array(bounds, dtype=np.uint64)


def pool_table(counts, lens, *, seed=1, lead=0, deletes=0.25):
    """(POOL, ops, rec_op): records of counts[r] ops whose keys and values are
    windows of POOL (they overlap and repeat) of the lengths lens(rng) draws."""
    import random
    rng = random.Random(seed)
    rows = [((rng.getrandbits(56) << 8) | 9, M64 - 3, M64 - 1, 5, 5) for _ in range(lead)]
    bounds = [lead]
    for c in counts:
        for _ in range(c):
            kl = lens(rng)
            ko = rng.randrange(0, len(POOL) - kl + 1)
            noise = rng.getrandbits(56) << 8
            if rng.random() < deletes:
                rows.append((noise | DELETION, ko, rng.getrandbits(64), kl, rng.getrandbits(32)))
            else:
                vl = lens(rng)
                rows.append((noise | VALUE, ko, rng.randrange(0, len(POOL) - vl + 1), kl, vl))
        bounds.append(len(rows))
    ops = np.array(rows, dtype=_dtype()) if rows else np.zeros(0, dtype=_dtype())
    return POOL, ops, np.array(bounds, dtype=np.uint64)


def short_len(rng):
    return rng.randrange(0, 31)


def ref_multiple_table():
    """[Put foo bar, Delete box, Put baz boo] (write_batch.rs:240-258)."""
    return table([[(b"foo", b"bar"), (b"box", None), (b"baz", b"boo")]])


def ref_append_tables():
    """The concatenated ops of the four stages of the append test
    (write_batch.rs:276-297), each as one record."""
    stages = [[], [(b"a", b"va")], [(b"a", b"va"), (b"b", b"vb")],
              [(b"a", b"va"), (b"b", b"vb"), (b"b", b"vb"), (b"foo", None)]]
    return [table([s]) for s in stages]


def status_cases():
    """(name, src, ops, rec_op, op_cap, out_cap or None, status): every status
    the op table or the capacity can raise at its smallest input, and the
    inputs next to them that are accepted."""
    dt = _dtype()
    src = b"0123456789"

    def one(typ, ko, kl, vo=0, vl=0):
        return np.array([(typ, ko, vo, kl, vl)], dtype=dt), np.array([0, 1], dtype=np.uint64)
    yield ("type2", src) + one(2, 0, 1) + (1, None, BAD_OP)
    yield ("type255_noise", src) + one((5 << 8) | 255, 0, 1) + (1, None, BAD_OP)
    yield ("key_exact", src) + one(DELETION, 4, 6) + (1, None, 0)
    yield ("key_one_over", src) + one(DELETION, 4, 7) + (1, None, BAD_OP)
    yield ("key_off_at_end_empty", src) + one(DELETION, 10, 0) + (1, None, 0)
    yield ("key_off_past_end", src) + one(DELETION, 11, 0) + (1, None, BAD_OP)
    yield ("value_exact", src) + one(VALUE, 0, 1, 2, 8) + (1, None, 0)
    yield ("value_one_over", src) + one(VALUE, 0, 1, 2, 9) + (1, None, BAD_OP)
    yield ("key_off_wraps", src) + one(DELETION, M64, 2) + (1, None, BAD_OP)
    yield ("value_off_wraps", src) + one(VALUE, 0, 1, M64, 2) + (1, None, BAD_OP)
    yield ("deletion_wild_value", src) + one(DELETION, 0, 3, M64, 0xFFFFFFFF) + (1, None, 0)
    two = np.array([(VALUE, 0, 3, 3, 3), (DELETION, 1, 0, 2, 0)], dtype=dt)
    yield ("bounds_fall", src, two, np.array([0, 2, 1], dtype=np.uint64), 2, None, BAD_BOUNDS)
    yield ("last_bound_over", src, two, np.array([0, 1, 3], dtype=np.uint64), 2, None, BAD_BOUNDS)
    yield ("first_bound_over", src, two, np.array([3, 3], dtype=np.uint64), 2, None, BAD_BOUNDS)
    yield ("bounds_before_ops", src, np.array([(2, 0, 0, 1, 0), (2, 0, 0, 1, 0)], dtype=dt),
           np.array([0, 2, 1], dtype=np.uint64), 2, None, BAD_BOUNDS)
    yield ("second_op_bad", src, np.array([(VALUE, 0, 3, 3, 3), (VALUE, 0, 3, 3, 8)], dtype=dt),
           np.array([0, 0, 1, 1, 2], dtype=np.uint64), 2, None, BAD_OP)
    need = 12 * 2 + (1 + 1 + 3 + 1 + 3) + (1 + 1 + 2)
    yield ("out_exact", src, two, np.array([0, 1, 2], dtype=np.uint64), 2, need, 0)
    yield ("out_one_short", src, two, np.array([0, 1, 2], dtype=np.uint64), 2, need - 1, OUT_OVER)
    yield ("op_before_out", src, np.array([(VALUE, 0, 3, 3, 3), (3, 0, 0, 1, 0)], dtype=dt),
           np.array([0, 1, 2], dtype=np.uint64), 2, 0, BAD_OP)


VARINT_EDGES = (0, 127, 128, 16383, 16384, 2097151, 2097152)


# ---- the device call, checked ----
def dev_ops(torch, dev, ops):
    a = np.ascontiguousarray(ops, dtype=_dtype())
    if a.size == 0:
        return torch.zeros(32, dtype=torch.uint8, device=dev)
    return torch.from_numpy(a.view(np.uint8).copy()).to(dev)


def guarded_out(torch, dev, cap, shift=0):
    """(buffer, view of cap bytes at `shift` past a 16-B boundary) with GUARD
    canary bytes on both sides; the whole buffer holds the canary."""
    buf = torch.full((cap + 2 * GUARD + 32,), CANARY, dtype=torch.uint8, device=dev)
    base = (-buf.data_ptr()) % 16 + shift + GUARD
    return buf, buf[base:base + cap], base


class Run:
    """One device call: the Encoded, the guarded buffers, the model's answer."""


def run(torch, dev, src, ops, rec_op, *, first_sequence, src_shift=0, out_shift=0, records=None, upstream=None,
        rec_cap=None, op_cap=None, out_cap=None, want_ops=True, workspace=None, stream=None):
    import lvgpu.write_batch as WB
    r = Run()
    n = len(rec_op) - 1
    r.records = n if records is None else records
    r.rec_cap = max(n, 0) if rec_cap is None else rec_cap
    r.op_cap = len(ops) if op_cap is None else op_cap
    r.want = model(src, ops, rec_op, r.records, first_sequence, r.op_cap, out_cap, rec_cap=r.rec_cap,
                   upstream=upstream or 0)
    if out_cap is None:
        t = r.want[4]
        out_cap = t["out_bytes"] if not t["status"] else 64
    r.out_cap = out_cap
    r.src_buf, d_src = C.guarded_payload(torch, dev, src, src_shift)
    r.src, r.src_shift = bytes(src), src_shift
    r.out_buf, d_out, r.out_base = guarded_out(torch, dev, out_cap, out_shift)
    d_ops = dev_ops(torch, dev, ops)
    d_rec_op = C.dev_i64(torch, dev, rec_op)
    d_n = C.dev_i64(torch, dev, [r.records])
    d_up = None if upstream is None else C.dev_i64(torch, dev, [upstream])
    if workspace is None:  # dirty on purpose
        workspace = torch.full((max(WB.encode_workspace_bytes(r.rec_cap, r.op_cap), 16),), 0x5A, dtype=torch.uint8,
                               device=dev)
    r.enc = WB.encode_device(d_src, d_ops, d_rec_op, d_n, d_up, first_sequence=first_sequence, rec_cap=r.rec_cap,
                             op_cap=r.op_cap, out=d_out, out_cap=out_cap, workspace=workspace, stream=stream,
                             fill=CANARY, guard=GUARD, want_ops=want_ops)
    return r


def compare(r, tag=""):
    """Every byte the call wrote against the model, and every canary."""
    enc = r.enc
    w_out, w_off, w_len, w_ops, w_tot = r.want
    t = enc.sync_totals(check=False)
    assert t == w_tot, (tag, t, w_tot)
    host = r.out_buf.cpu().numpy()
    used = 0 if t["status"] else t["out_bytes"]
    assert (host[:r.out_base] == CANARY).all() and (host[r.out_base + used:] == CANARY).all(), \
        (tag, "d_out written outside [0, out_bytes)")
    n = 0 if t["status"] else t["records"]
    k = 0 if t["status"] else t["ops"]
    assert C.tail_is_canary(enc.rec_off_t, n * 8) and C.tail_is_canary(enc.rec_len_t, n * 8), \
        (tag, "record arrays written past the records")
    if enc.ops_t is not None:
        assert C.tail_is_canary(enc.ops_t, k * 32), (tag, "d_ops_out written past the ops")
    if not t["status"]:
        got = host[r.out_base:r.out_base + used].tobytes()
        if got != w_out:
            at = next(i for i in range(min(len(got), len(w_out))) if got[i] != w_out[i])
            raise AssertionError((tag, "d_out differs at byte", at, got[at:at + 16].hex(), w_out[at:at + 16].hex()))
        assert np.array_equal(enc.rec_off(), w_off), (tag, "rec_off")
        assert np.array_equal(enc.rec_len(), w_len), (tag, "rec_len")
        if enc.ops_t is not None:
            g = enc.ops()
            diff = np.nonzero(g != w_ops)[0]
            assert g.shape == w_ops.shape and diff.size == 0, (tag, "op", int(diff[0]), g[diff[0]], w_ops[diff[0]])
    src_host = r.src_buf.cpu().numpy()
    base = (-r.src_buf.data_ptr()) % 16 + r.src_shift + GUARD
    assert (src_host[:base] == CANARY).all() and (src_host[base + len(r.src):] == CANARY).all(), (tag, "source guards")
    assert src_host[base:base + len(r.src)].tobytes() == r.src, (tag, "source changed")


def check(torch, dev, src, ops, rec_op, *, first_sequence=1, tag="", **kw):
    """Runs the device call over a guarded source with canary-filled, guarded
    outputs and a dirty workspace, and compares every byte and every canary
    with the model."""
    r = run(torch, dev, src, ops, rec_op, first_sequence=first_sequence, **kw)
    compare(r, tag)
    return r


# ---- stress trials ----
STRESS_TRIALS = 100
STRESS_BUDGET = 4 << 20  # bytes of long keys and values in one trial


def stress_trial(seed, tile=1024, wave_copy=64):
    """(src, ops, rec_op, first_sequence, lead, (has_empty, has_long, has_big_record))
    of one trial: 1-3,000 records; 0, 1, a few or hundreds of ops each; key and
    value lengths 0, 1-30, around wave_copy or up to 64 KiB, windows of POOL.
    Every fifth trial holds an empty record, a long copy and a record above one
    tile."""
    import random
    rng = random.Random(9000 + seed)
    nrec = [1, 2, rng.randrange(3, 200), rng.randrange(200, 3001)][rng.randrange(4)]
    budget = [STRESS_BUDGET]
    counts = []
    for _ in range(nrec):
        kind = rng.randrange(40)
        counts.append(0 if kind < 3 else 1 if kind < 28 else rng.randrange(2, 8) if kind < 39 else rng.randrange(100, 400))
    if seed % 5 == 0:
        counts.insert(rng.randrange(len(counts) + 1), 0)
        counts.insert(rng.randrange(len(counts) + 1), tile + rng.randrange(1, 300))

    def lens(r):
        k = r.randrange(20)
        if k < 2:
            return 0
        if k < 16 or budget[0] <= 0:
            return r.randrange(1, 31)
        if k < 19:
            return r.randrange(max(wave_copy - 20, 0), wave_copy + 40)
        n = r.randrange(0, 65537)
        budget[0] -= n
        return n
    src, ops, rec_op = pool_table(counts, lens, seed=9000 + seed, lead=rng.randrange(0, 4))
    if seed % 5 == 0:  # a long copy, whatever the draws were
        j = int(rec_op[-1]) - 1
        ops[j]["tag"] = (int(ops[j]["tag"]) & ~0xFF) | VALUE
        ops[j]["val_off"], ops[j]["val_len"] = 17, 40000 + seed
    first = rng.choice([1, rng.getrandbits(40), M64 - rng.randrange(0, 50), rng.getrandbits(64)])
    live = ops[int(rec_op[0]):]
    is_val = (live["tag"] & 0xFF) == VALUE
    has_long = bool((live["key_len"] >= wave_copy).any() or (is_val & (live["val_len"] >= wave_copy)).any())
    flags = (0 in counts, has_long, max(counts) > tile)
    return src, ops, rec_op, first, int(rec_op[0]), flags
