"""The WriteBatch format in Python, case generators and the comparison helper
shared by the WriteBatch tests (test_write_batch.py,
test_gpu_write_batch_device.py, test_gpu_write_batch_stress.py).

WriteBatch restates write_batch.rs:57-90 and :131-161 (put / delete / clear /
set_sequence / append); iterate restates WriteBatch::iterate with a
MemTableInserter (write_batch.rs:92-122, :178-188) over coding.rs:186-204 and
:294-305.  It is the model every output of lv_write_batch_iterate and
lv_write_batch_decode_device is compared with."""
import numpy as np

HEADER = 12
DELETION, VALUE = 0, 1
OK, TOO_SMALL, BAD_VARINT, BAD_LENGTH, WRONG_COUNT, BAD_TAG, OUT_OF_RANGE = range(7)
UPSTREAM, REC_OVER, OP_OVER = 1, 2, 4
M64 = (1 << 64) - 1

CANARY = 0xA5
GUARD = 64


def varint(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


class WriteBatch:
    def __init__(self):
        self.rep = bytearray(HEADER)

    @property
    def count(self):
        return int.from_bytes(self.rep[8:12], "little")

    def set_count(self, n):
        self.rep[8:12] = (n & 0xFFFFFFFF).to_bytes(4, "little")

    @property
    def sequence(self):
        return int.from_bytes(self.rep[0:8], "little")

    def set_sequence(self, seq):
        self.rep[0:8] = (seq & M64).to_bytes(8, "little")
        return self

    def put(self, key, value):
        self.set_count(self.count + 1)
        self.rep.append(VALUE)
        self.rep += varint(len(key)) + bytes(key) + varint(len(value)) + bytes(value)
        return self

    def delete(self, key):
        self.set_count(self.count + 1)
        self.rep.append(DELETION)
        self.rep += varint(len(key)) + bytes(key)
        return self

    def clear(self):
        self.rep = bytearray(HEADER)

    def append(self, src):
        self.set_count(self.count + src.count)
        assert len(src.rep) >= HEADER
        self.rep += src.rep[HEADER:]

    def bytes(self):
        return bytes(self.rep)


def _varstring(rep, pos):
    """(status, length, position past the length)."""
    result, shift, n = 0, 0, len(rep)
    while shift <= 28 and pos < n:
        b = rep[pos]
        pos += 1
        result |= ((b & 0x7F) << shift) & 0xFFFFFFFF
        shift += 7
        if not b & 0x80:
            if n - pos < result:
                return BAD_LENGTH, 0, pos
            return OK, result, pos
    return BAD_VARINT, 0, pos


def iterate_ext(rep):
    """(status, ops, sequence, count); ops = [(tag, key_off, key_len, val_off,
    val_len)] with offsets into rep, every op handed to the Handler before the
    return."""
    rep = bytes(rep)
    if len(rep) < HEADER:
        return TOO_SMALL, [], 0, 0
    seq = int.from_bytes(rep[0:8], "little")
    count = int.from_bytes(rep[8:12], "little")
    pos, ops, status = HEADER, [], OK
    while pos < len(rep):
        tag = rep[pos]
        pos += 1
        if tag > VALUE:
            status = BAD_TAG
            break
        status, klen, pos = _varstring(rep, pos)
        if status:
            break
        koff = pos
        pos += klen
        voff, vlen = pos, 0
        if tag == VALUE:
            status, vlen, pos = _varstring(rep, pos)
            if status:
                break
            voff = pos
            pos += vlen
        ops.append(((((seq + len(ops)) << 8) | tag) & M64, koff, klen, voff, vlen))
    if status == OK and len(ops) != count:
        status = WRONG_COUNT
    return status, ops, seq, count


def iterate(rep):
    """(status, [(tag, key, value)]): what the Handler received."""
    rep = bytes(rep)
    status, ops, _, _ = iterate_ext(rep)
    return status, [(t, rep[ko:ko + kl], rep[vo:vo + vl]) for t, ko, kl, vo, vl in ops]


def print_contents(rep):
    """The reference tests' print_contents (write_batch.rs:200-238), in the
    order its expected strings pin: user key ascending, then sequence
    ascending ("Put(b, vb)@201Put(b, vb)@202", write_batch.rs:293-296, where
    the reference itself notes that C++ LevelDB orders these the other way)."""
    status, ops = iterate(rep)
    out = ""
    for tag, key, value in sorted(ops, key=lambda o: (o[1], o[0] >> 8)):
        if tag & 0xFF == VALUE:
            out += f"Put({key.decode()}, {value.decode()})"
        else:
            out += f"Delete({key.decode()})"
        out += f"@{tag >> 8}"
    assert status != BAD_TAG, "the reference panics here"
    if status != OK:  # iterate returned an Err, "WriteBatch has wrong count" included
        out += "ParseError()"
    return out


# ---- the reference's own cases (write_batch.rs:240-297) ----
def ref_multiple():
    return WriteBatch().put(b"foo", b"bar").delete(b"box").put(b"baz", b"boo").set_sequence(100)


def ref_corruption():
    b = WriteBatch().put(b"foo", b"bar").delete(b"box").set_sequence(200)
    del b.rep[-1:]
    return b


def ref_append_stages():
    """The four (rep, expected print_contents) stages of the append test."""
    b1, b2 = WriteBatch().set_sequence(200), WriteBatch().set_sequence(300)
    out = []
    b1.append(b2)
    out.append((b1.bytes(), ""))
    b2.put(b"a", b"va")
    b1.append(b2)
    out.append((b1.bytes(), "Put(a, va)@200"))
    b2.clear()
    b2.put(b"b", b"vb")
    b1.append(b2)
    out.append((b1.bytes(), "Put(a, va)@200Put(b, vb)@201"))
    b2.delete(b"foo")
    b1.append(b2)
    out.append((b1.bytes(), "Put(a, va)@200Put(b, vb)@201Put(b, vb)@202Delete(foo)@203"))
    return out


def hdr(seq, count):
    return (seq & M64).to_bytes(8, "little") + (count & 0xFFFFFFFF).to_bytes(4, "little")


def status_cases():
    """(name, rep, status, ops emitted): every status at its smallest input."""
    put_ab = bytes([VALUE, 1]) + b"a" + bytes([1]) + b"b"
    yield "ok_empty", hdr(5, 0), OK, 0
    for n in range(HEADER):
        yield f"too_small_{n}", bytes(range(1, n + 1)), TOO_SMALL, 0
    yield "ends_after_tag", hdr(1, 1) + bytes([VALUE]), BAD_VARINT, 0
    yield "ends_after_tag0", hdr(1, 1) + bytes([DELETION]), BAD_VARINT, 0
    yield "ends_inside_varint2", hdr(1, 1) + bytes([DELETION, 0x80]), BAD_VARINT, 0
    yield "varint5_continues", hdr(1, 1) + bytes([DELETION, 0x80, 0x80, 0x80, 0x80, 0x80, 0]), BAD_VARINT, 0
    # fifth byte 0x70: bits 32..34 fall off, the value is 2
    yield "varint5_top_bits", hdr(1, 1) + bytes([DELETION, 0x82, 0x80, 0x80, 0x80, 0x70]) + b"xy", OK, 1
    yield "varint5_top_bits_short", hdr(1, 1) + bytes([DELETION, 0x82, 0x80, 0x80, 0x80, 0x70]) + b"x", BAD_LENGTH, 0
    yield "varint5_big", hdr(1, 1) + bytes([DELETION, 0xFF, 0xFF, 0xFF, 0xFF, 0x0F]) + b"x", BAD_LENGTH, 0
    yield "length_one_more", hdr(1, 1) + bytes([DELETION, 3]) + b"ab", BAD_LENGTH, 0
    yield "length_exact", hdr(1, 1) + bytes([DELETION, 2]) + b"ab", OK, 1
    yield "tag2", hdr(1, 2) + put_ab + bytes([2, 0]), BAD_TAG, 1
    yield "tag255", hdr(1, 1) + bytes([255]), BAD_TAG, 0
    yield "count_high", hdr(1, 2) + put_ab, WRONG_COUNT, 1
    yield "count_low", hdr(1, 0) + put_ab, WRONG_COUNT, 1
    yield "value_fails_no_op", hdr(1, 1) + bytes([VALUE, 1]) + b"k" + bytes([5]) + b"abcd", BAD_LENGTH, 0
    yield "value_varint_missing", hdr(1, 1) + bytes([VALUE, 1]) + b"k", BAD_VARINT, 0
    yield "after_one_op", hdr(9, 2) + put_ab + bytes([VALUE, 1]) + b"k" + bytes([0x80]), BAD_VARINT, 1
    yield "empty_key_value", hdr(1, 2) + bytes([VALUE, 0, 0, DELETION, 0]), OK, 2


def mixed_batch(nops, seed=3, seq=1000, maxlen=40):
    rng = np.random.default_rng(seed)
    b = WriteBatch().set_sequence(seq)
    for _ in range(nops):
        key = rng.integers(0, 256, size=int(rng.integers(0, maxlen)), dtype=np.uint8).tobytes()
        if rng.random() < 0.3:
            b.delete(key)
        else:
            b.put(key, rng.integers(0, 256, size=int(rng.integers(0, 4 * maxlen)), dtype=np.uint8).tobytes())
    return b


def wave_batch(small, nops=30, seed=3, seq=5000):
    """A mixed batch made longer than `small` bytes (the wave class) by a last
    Put whose value the walk skips."""
    return mixed_batch(nops, seed=seed, seq=seq, maxlen=60).put(b"pad", bytes(small)).bytes()


def one_put(seq, klen=16, vlen=100, fill=0x61):
    """db_bench's record: one Put of a 16-B key and a 100-B value (131 bytes)."""
    return WriteBatch().set_sequence(seq).put(bytes([fill & 0xFF]) * klen, bytes([(fill + 1) & 0xFF]) * vlen).bytes()


def pack(reps, gaps=None):
    """(payload, rec_off, rec_len) of reps laid in order, gaps[i] bytes of
    0xEE before rep i."""
    payload, off = bytearray(), []
    for i, r in enumerate(reps):
        if gaps is not None:
            payload += b"\xEE" * int(gaps[i])
        off.append(len(payload))
        payload += r
    return bytes(payload), np.array(off, dtype=np.uint64), np.array([len(r) for r in reps], dtype=np.uint64)


# ---- the model of one device call ----
def model(payload, rec_off, rec_len):
    """(ops structured array, bounds, statuses, totals dict) of a call whose
    capacities suffice."""
    from lvgpu.write_batch import OP_DTYPE
    P = len(payload)
    ops, bounds, statuses = [], [0], []
    kb = vb = bad = last = 0
    for o, n in zip((int(x) for x in rec_off), (int(x) for x in rec_len)):
        if o > P or n > P - o:
            st, rops, seq = OUT_OF_RANGE, [], 0
        else:
            st, rops, seq, _ = iterate_ext(payload[o:o + n])
        for t, ko, kl, vo, vl in rops:
            ops.append((t, ko + o, vo + o, kl, vl))
            kb += kl
            vb += vl
        if rops:
            last = max(last, (seq + len(rops) - 1) & M64)
        bad += st != OK
        statuses.append(st)
        bounds.append(len(ops))
    arr = np.array(ops, dtype=OP_DTYPE) if ops else np.zeros(0, dtype=OP_DTYPE)
    totals = dict(records=len(statuses), ops=len(ops), key_bytes=kb, value_bytes=vb, bad_records=bad,
                  last_sequence=last, status=0)
    return arr, np.array(bounds, dtype=np.uint64), np.array(statuses, dtype=np.uint32), totals


def dev_i64(torch, dev, a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size == 0:
        return torch.zeros(1, dtype=torch.int64, device=dev)
    return torch.from_numpy(a.view(np.int64).copy()).to(dev)


def guarded_payload(torch, dev, payload, shift=0, tail_exact=False):
    """The payload in device memory at `shift` bytes past a 16-B boundary with
    GUARD canary bytes on both sides.  tail_exact: the payload's last byte is
    the last byte of its allocation's used part (the guard still follows, in
    the same allocation: an overread of up to the granule stays harmless, and a
    kernel that trusted bytes behind the payload would read canaries)."""
    buf = torch.full((len(payload) + 2 * GUARD + 32,), CANARY, dtype=torch.uint8, device=dev)
    base = (-buf.data_ptr()) % 16 + shift + GUARD
    t = buf[base:base + len(payload)]
    if len(payload):
        t.copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
    return buf, t


def tail_is_canary(t, used):
    """True if every byte of the uint8 view of tensor t from `used` on holds the canary."""
    import torch
    b = t.view(torch.uint8)
    return bool((b[used:] == CANARY).all())


def run(torch, dev, payload, rec_off, rec_len, *, shift=0, records=None, upstream=None, rec_cap=None, op_cap=None,
        workspace=None, stream=None):
    """One lv_write_batch_decode_device call over a guarded payload with
    canary-filled outputs: (Ops, payload buffer)."""
    import lvgpu.write_batch as WB
    buf, d_pay = guarded_payload(torch, dev, payload, shift)
    d_off, d_len = dev_i64(torch, dev, rec_off), dev_i64(torch, dev, rec_len)
    n = len(rec_off)
    d_n = dev_i64(torch, dev, [n if records is None else records])
    d_up = None if upstream is None else dev_i64(torch, dev, [upstream])
    cap = max(n, 1) if rec_cap is None else rec_cap
    if workspace is None:  # dirty on purpose
        workspace = torch.full((WB.decode_workspace_bytes(cap),), 0x5A, dtype=torch.uint8, device=dev)
    ops = WB.decode_device(d_pay, d_off, d_len, d_n, d_up, rec_cap=cap, op_cap=op_cap, workspace=workspace,
                           stream=stream, fill=CANARY, guard=GUARD)
    return ops, buf


def compare(ops, want, tag=""):
    """The outputs of a call whose status is 0 against model()'s."""
    w_ops, w_bounds, w_st, w_tot = want
    t = ops.sync_totals()
    assert t == w_tot, (tag, t, w_tot)
    got_b = ops.record_bounds()
    assert np.array_equal(got_b, w_bounds), (tag, "bounds", got_b[:8], w_bounds[:8])
    got_s = ops.statuses()
    bad = np.nonzero(got_s != w_st)[0]
    assert bad.size == 0, (tag, "status of record", int(bad[0]), int(got_s[bad[0]]), int(w_st[bad[0]]))
    got = ops.ops()
    assert got.shape == w_ops.shape, (tag, got.shape, w_ops.shape)
    diff = np.nonzero(got != w_ops)[0]
    assert diff.size == 0, (tag, "op", int(diff[0]), got[diff[0]], w_ops[diff[0]])
    n, k = w_tot["records"], w_tot["ops"]
    assert tail_is_canary(ops.ops_t, k * 32), (tag, "d_ops written past the ops")
    assert tail_is_canary(ops.rec_op, (n + 1) * 8), (tag, "d_rec_op written past records + 1")
    assert tail_is_canary(ops.rec_status, n * 4), (tag, "d_rec_status written past records")


def untouched(ops):
    """True if every output array but the totals still holds the canary."""
    return tail_is_canary(ops.ops_t, 0) and tail_is_canary(ops.rec_op, 0) and tail_is_canary(ops.rec_status, 0)


def check(torch, dev, payload, rec_off, rec_len, *, shift=0, op_cap=None, tag=""):
    """Runs the device call and compares the ops, bounds, statuses and totals
    with the model, and the canaries behind every output array and around the
    payload."""
    payload = bytes(payload)
    ops, buf = run(torch, dev, payload, rec_off, rec_len, shift=shift, op_cap=op_cap)
    want = model(payload, rec_off, rec_len)
    compare(ops, want, tag)
    host = buf.cpu().numpy()
    base = (-buf.data_ptr()) % 16 + shift + GUARD
    assert (host[:base] == CANARY).all() and (host[base + len(payload):] == CANARY).all(), (tag, "payload guards")
    assert host[base:base + len(payload)].tobytes() == payload, (tag, "payload changed")
    return ops, want


# ---- stress trials ----
STRESS_TRIALS = 100
_POOL = np.random.default_rng(99).integers(0, 256, size=1 << 17, dtype=np.uint8).tobytes()


def _rand_bytes(rng, n):
    o = rng.randrange(0, len(_POOL) - n + 1)
    return _POOL[o:o + n]


def _rand_len(rng, window):
    k = rng.randrange(10)
    if k == 0:
        return 0
    if k < 7:
        return rng.randrange(1, 31)
    if k < 9:
        return rng.randrange(window - 40, window + 40)
    return rng.randrange(0, 65537)


def stress_trial(seed, small=256, window=4096):
    """(payload, rec_off, rec_len, has_wave_class, has_bad) of one trial:
    1-3,000 records; 0, 1, a few or hundreds of ops each; key and value lengths
    0, 1-30, around the window or up to 64 KiB; about 5 % of the records
    corrupted (truncation, a flipped byte, a wrong count); packed or gapped."""
    import random
    rng = random.Random(7000 + seed)
    nrec = [1, 2, rng.randrange(3, 200), rng.randrange(200, 3001)][rng.randrange(4)]
    budget = 4 << 20  # bytes of long keys and values in one trial
    reps = []
    for _ in range(nrec):
        kind = rng.randrange(40)
        nops = 0 if kind < 2 else 1 if kind < 28 else rng.randrange(2, 8) if kind < 39 else rng.randrange(100, 400)
        b = WriteBatch().set_sequence(rng.randrange(1 << 56))
        for _ in range(nops):
            simple = nops >= 100 or budget <= 0 or rng.random() < 0.9
            kl = rng.randrange(1, 31) if simple else _rand_len(rng, window)
            vl = rng.randrange(0, 120) if simple else _rand_len(rng, window)
            if not simple:
                budget -= kl + vl
            if rng.random() < 0.25:
                b.delete(_rand_bytes(rng, kl))
            else:
                b.put(_rand_bytes(rng, kl), _rand_bytes(rng, vl))
        rep = bytearray(b.rep)
        if rng.random() < 0.05:
            how = rng.randrange(3)
            if how == 0:
                del rep[rng.randrange(len(rep) + 1):]
            elif how == 1:  # among the first bytes, where a short record's entry headers are
                rep[rng.randrange(min(len(rep), 64))] ^= 1 << rng.randrange(8)
            else:
                rep[8:12] = ((b.count + rng.randrange(1, 3)) & 0xFFFFFFFF).to_bytes(4, "little")
        reps.append(bytes(rep))
    if seed % 5 == 0:  # never hollow: a wave-class record and a bad one
        reps.append(wave_batch(small, seed=seed))
        reps.append(mixed_batch(4, seed=seed).bytes()[:-1])
        reps.append(wave_batch(small, nops=70, seed=seed + 1)[:-3])  # a bad wave-class record
    gaps = [rng.randrange(40) for _ in reps] if rng.random() < 0.5 else None
    payload, off, ln = pack(reps, gaps)
    has_wave = bool((ln > small).any())
    has_bad = any(iterate_ext(r)[0] != OK for r in reps)
    return payload, off, ln, has_wave, has_bad


