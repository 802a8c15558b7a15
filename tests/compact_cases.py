"""The compaction filter in Python, case generators and the comparison helpers
shared by the compaction tests (test_compact.py, test_gpu_compact_device.py,
test_gpu_compact_stress.py).

model_filter is the model every output of lv_compact_filter_* is compared with:
upstream's DoCompactionWork loop (include/lvgpu/compact.h) written with Python
bytes, and IsBaseLevelForKey as a linear walk of (lo, hi) pairs."""
import numpy as np

from memtable_cases import MAX_SEQUENCE, dev_bytes, dev_i64, make_table, model_order, tag
from memtable_cases import key_of as make_key  # noqa: F401  (the tests name an entry's key with it)
from write_batch_cases import CANARY, GUARD, guarded_payload, tail_is_canary

BASE_LEVEL = 1
UPSTREAM, BAD_INPUT, BAD_RANGE = 1, 2, 4
TOTALS = ("entries_in", "kept", "dropped_hidden", "dropped_deletions", "unparsed", "user_keys", "reserved", "status")
NO_TABLE = dict(entries=0, user_keys=0, status=1)  # what every status leaves in *mt_totals_out
ORDER_CANARY = 0xA5A5A5A5


def range_dtype():
    from lvgpu.compact import RANGE_DTYPE
    return RANGE_DTYPE


def raw_ranges(ranges):
    """[(lo, hi)] -> (rows [(lo_off, hi_off, lo_len, hi_len)], key bytes); a
    (rows, keys) pair passes through (rows a test made out of range)."""
    if ranges is None:
        return [], b""
    if isinstance(ranges, tuple):
        return [tuple(int(v) for v in r) for r in ranges[0]], bytes(ranges[1])
    keys, rows = b"", []
    for lo, hi in ranges:
        rows.append((len(keys), len(keys) + len(lo), len(lo), len(hi)))
        keys += lo + hi
    return rows, keys


def for_binding(ranges):
    """What lvgpu.compact takes: None, or (RANGE_DTYPE array, key bytes)."""
    rows, keys = raw_ranges(ranges)
    if not rows:
        return None
    return np.array(rows, dtype=range_dtype()), keys


def _inside(off, ln, total):
    return off <= total and ln <= total - off


def model_filter(payload, ops, order, mt, S, ranges=None, flags=0, *, op_cap=None, payload_bytes=None):
    """(totals dict, mt_totals_out dict, kept op indices or None with a status)."""
    rows, rkeys = raw_ranges(ranges)
    n = mt["entries"]
    op_cap = len(ops) if op_cap is None else op_cap
    pbytes = len(payload) if payload_bytes is None else payload_bytes
    tot = dict.fromkeys(TOTALS, 0)
    tot["entries_in"] = n
    st = 0
    if mt["status"]:
        st = UPSTREAM
    else:
        for lo_off, hi_off, lo_len, hi_len in rows:
            if not _inside(lo_off, lo_len, len(rkeys)) or not _inside(hi_off, hi_len, len(rkeys)) or \
                    rkeys[lo_off:lo_off + lo_len] > rkeys[hi_off:hi_off + hi_len]:
                st |= BAD_RANGE
                break
        if n > op_cap:
            st |= BAD_INPUT
    if not st:
        for i in range(n):
            idx = int(order[i])
            if idx >= op_cap or not _inside(int(ops[idx]["key_off"]), int(ops[idx]["key_len"]), pbytes):
                st = BAD_INPUT
                break
    if st:
        tot["status"] = st
        return tot, dict(NO_TABLE), None
    spans = [(rkeys[a:a + al], rkeys[b:b + bl]) for a, b, al, bl in rows]

    def base_level(k):
        return bool(flags & BASE_LEVEL) and not any(lo <= k <= hi for lo, hi in spans)

    ko, kl, tags = ops["key_off"].tolist(), ops["key_len"].tolist(), ops["tag"].tolist()
    kept, cur, last_seq, last_kept = [], None, MAX_SEQUENCE, None
    for i in range(n):
        idx = int(order[i])
        k, typ, seq = payload[ko[idx]:ko[idx] + kl[idx]], tags[idx] & 0xFF, tags[idx] >> 8
        drop = False
        if typ > 1:
            cur, last_seq = None, MAX_SEQUENCE
            tot["unparsed"] += 1
        else:
            if cur is None or k != cur:
                cur, last_seq = k, MAX_SEQUENCE
            if last_seq <= S:
                drop = True
                tot["dropped_hidden"] += 1
            elif typ == 0 and seq <= S and base_level(k):
                drop = True
                tot["dropped_deletions"] += 1
            last_seq = seq
        if not drop:
            tot["user_keys"] += last_kept is None or k != last_kept
            last_kept = k
            kept.append(idx)
    tot["kept"] = len(kept)
    return tot, dict(entries=len(kept), user_keys=tot["user_keys"], status=0), kept


# ---- cases: name -> (items, gaps, [(S, flags, ranges)]) -----------------------
def _versions(key, seqs, typ=1):
    return [(key, tag(s, typ), b"" if typ == 0 else b"v%d" % s) for s in seqs]


THRESHOLD_S = (0, 2, 3, 4, 6, 7, MAX_SEQUENCE - 1)
RANGE_LO, RANGE_HI = b"bbb", b"ddd"


def range_lists():
    many = [(b"r%04d" % i, b"r%04d~" % i) for i in range(4095)] + [(RANGE_LO, RANGE_HI)]
    assert len(many) == 4096
    return {"none": [], "one": [(RANGE_LO, RANGE_HI)], "4096": many}


def aligned_items():
    """Key lengths 7, 8, 9, 15, 16, 17 with every pair of payload alignments
    mod 8 between an entry and its predecessor: two versions of one key and a
    key that differs in the last byte only, behind gaps that walk the offsets."""
    items, gaps = [], []
    for ln in (7, 8, 9, 15, 16, 17):
        for a in range(8):
            stem = bytes([97 + a]) * (ln - 1)
            for j, it in enumerate(_versions(stem + b"x", (9, 4)) + _versions(stem + b"y", (8,))):
                items.append(it)
                gaps.append((a + 3 * j) % 8 + 1)
    return items, gaps


def cases():
    both = lambda ss: [(s, f, None) for s in ss for f in (0, BASE_LEVEL)]
    p16 = b"0123456789abcdef"
    c = {}
    c["thresholds"] = (_versions(b"k", range(1, 7)) + _versions(b"j", (3,)) + _versions(b"l", (3,)), None,
                       [(s, 0, None) for s in THRESHOLD_S])
    c["duplicates"] = (_versions(b"d", (5, 9, 5, 9, 5)) + _versions(b"d", (5, 5), 0), None, both((4, 5, 8, 9, 10)))
    dels = (_versions(b"first", (5,), 0) + _versions(b"first", (3,)) +
            _versions(b"shadowed", (7, 2)) + _versions(b"shadowed", (5,), 0) +
            _versions(b"shadowing", (6,), 0) + _versions(b"shadowing", (4,)) +
            _versions(b"at_s", (5,), 0) + _versions(b"above_s", (6,), 0))
    c["deletions"] = (dels, None, both((4, 5, 6, 7)))
    unp = (_versions(b"u", (6, 5, 3, 2)) + _versions(b"u", (4,), 2) + _versions(b"v", (9, 6)) +
           _versions(b"v", (8,), 0xFF) + _versions(b"v", (7,), 0) + _versions(b"w", (1,), 2))
    c["unparsed"] = (unp, None, both((6, 9, 1)))
    keys = [b"", b"a", b"ab", p16, p16 + b"x", p16 + b"y", p16 + b"x\x00", p16 + b"xx", p16 * 3, p16 * 3 + b"\x00"]
    c["key_lengths"] = ([it for k in keys for it in _versions(k, (7, 3)) + _versions(k, (5,), 0)], None, both((2, 5, 8)))
    al, gaps = aligned_items()
    c["alignments"] = (al, gaps, both((3, 9)))
    rk = [RANGE_LO, RANGE_HI, b"bba", b"ddd\x00", b"bb", b"ccc", b"dde", b"", b"r0007", b"r0007~", b"r0007~~"]
    c["ranges"] = ([it for k in rk for it in _versions(k, (3,), 0) + _versions(k, (1,))], None,
                   [(5, BASE_LEVEL, r) for r in range_lists().values()] + [(2, BASE_LEVEL, range_lists()["one"])])
    return c


def table_of(items, gaps=None):
    """(payload, ops, order, mt totals) of items: the model's memtable."""
    payload, ops = make_table(items, gaps)
    order = np.array(model_order(payload, ops), dtype=np.uint32)
    keys = {bytes(k) for k, _, _ in items}
    return payload, ops, order, dict(entries=len(ops), user_keys=len(keys), status=0)


def status_cases():
    """name -> (kwargs of model_filter / the bindings, the status expected)."""
    items = _versions(b"a", (3, 2)) + _versions(b"b", (4,), 0) + [(b"tail", tag(9), b"")]  # the payload ends with a key
    payload, ops, order, mt = table_of(items)
    base = dict(payload=payload, ops=ops, order=order, mt=mt, S=5, ranges=None, flags=BASE_LEVEL)
    over = order.copy()
    over[2] = len(ops)
    dt = range_dtype()
    keys = b"aaazzz"
    return {
        "ok": (base, 0),
        "upstream": (dict(base, mt=dict(mt, status=4)), UPSTREAM),
        "entries_over": (dict(base, mt=dict(mt, entries=len(ops) + 1)), BAD_INPUT),
        "index_at_cap": (dict(base, order=over), BAD_INPUT),
        "extent_one_past": (dict(base, payload_bytes=len(payload) - 1), BAD_INPUT),
        "range_extent": (dict(base, ranges=(np.array([(0, 3, 3, 4)], dtype=dt), keys)), BAD_RANGE),
        "range_offset": (dict(base, ranges=(np.array([(7, 3, 0, 3)], dtype=dt), keys)), BAD_RANGE),
        "range_wraps": (dict(base, ranges=(np.array([(2 ** 64 - 1, 3, 2, 3)], dtype=dt), keys)), BAD_RANGE),
        "range_lo_above_hi": (dict(base, ranges=[(b"b", b"a")]), BAD_RANGE),
        "range_and_entries": (dict(base, ranges=[(b"b", b"a")], mt=dict(mt, entries=len(ops) + 1)), BAD_RANGE | BAD_INPUT),
        "range_hides_index": (dict(base, ranges=[(b"b", b"a")], order=over), BAD_RANGE),
    }


# ---- the host twin ----
def check_host(payload, ops, order, mt, S, ranges=None, flags=0, *, op_cap=None, payload_bytes=None, tag_=""):
    """lv_compact_filter_host against the model, field for field, with the
    canaries of order_out: the model's triple."""
    import lvgpu.compact as CP
    want = model_filter(payload, ops, order, mt, S, ranges, flags, op_cap=op_cap, payload_bytes=payload_bytes)
    got = CP.filter_host(payload, ops, order, mt, S, for_binding(ranges), flags, op_cap=op_cap,
                         payload_bytes=payload_bytes, fill=ORDER_CANARY)
    assert got.totals == want[0], (tag_, got.totals, want[0])
    assert got.mt_totals == want[1], (tag_, got.mt_totals, want[1])
    kept = want[0]["kept"]
    if want[2] is not None:
        assert got.order_out[:kept].tolist() == want[2], (tag_, got.order_out[:kept].tolist()[:8], want[2][:8])
    assert (got.order_out[kept:] == ORDER_CANARY).all(), (tag_, "order_out written at or beyond kept")
    return want


# ---- the device ----
def guarded_i64(torch, dev, n):
    """An int64 output of n words between canary words: (owner, the slice)."""
    buf = torch.full((8 * (n + 8),), CANARY, dtype=torch.uint8, device=dev).view(torch.int64)
    return buf, buf[4:4 + n]


def guards_intact(torch, buf, n):
    b = buf.view(torch.uint8)
    return bool((b[:32] == CANARY).all()) and bool((b[32 + 8 * n:] == CANARY).all())


def device_table(torch, dev, payload, ops, order, mt, *, shift=0, op_cap=None):
    """The quadruple in device memory as a lvgpu.memtable.Table: the payload
    `shift` bytes past a 16-B boundary between canaries, ops and order padded
    to op_cap."""
    import lvgpu.memtable as MT
    buf, d_pay = guarded_payload(torch, dev, payload, shift)
    cap = max(len(ops), 1) if op_cap is None else op_cap
    pad = max(cap - len(ops), 0)
    d_ops = dev_bytes(torch, dev, np.concatenate([ops, np.zeros(pad, dtype=ops.dtype)]))
    d_order = dev_bytes(torch, dev, np.concatenate([np.asarray(order, dtype=np.uint32), np.zeros(pad, dtype=np.uint32)]))
    d_mt = dev_i64(torch, dev, [mt["entries"], mt["user_keys"], mt["status"]])
    t = MT.Table(d_pay, d_ops, cap, d_order.view(torch.int32), d_mt, None)
    t._buf = buf
    return t


def run_device(torch, dev, table, S, ranges=None, flags=0, *, payload_bytes=None, stream=None):
    """One lv_compact_filter_device call with a canary-filled d_order_out,
    both totals between canary words and a dirty workspace: the Filtered."""
    import lvgpu.compact as CP
    import lvgpu.memtable as MT
    src = table
    if payload_bytes is not None:
        src = MT.Table(table.payload[:payload_bytes], table.ops_t, table.op_cap, table.order_t, table.totals, table)
    mt_buf, mt_out = guarded_i64(torch, dev, 3)
    tot_buf, tot = guarded_i64(torch, dev, 8)
    ws = torch.full((max(CP.filter_workspace_bytes(src.op_cap), 16),), 0x5A, dtype=torch.uint8, device=dev)
    f = CP.filter_device(src, S, for_binding(ranges), flags, mt_totals=mt_out, totals=tot, workspace=ws, stream=stream,
                         fill=CANARY, guard=GUARD)
    f._guards = (mt_buf, tot_buf)
    return f


def compare_device(torch, f, want, tag_=""):
    """A Filtered against model_filter's triple, with every canary."""
    got = f.sync(check=False)
    assert got == want[0], (tag_, got, want[0])
    mt = dict(zip(("entries", "user_keys", "status"), (int(v) for v in f.totals.cpu().numpy().view(np.uint64))))
    assert mt == want[1], (tag_, mt, want[1])
    kept = want[0]["kept"]
    if want[2] is not None:
        out = f.order_t[:kept].cpu().numpy().view(np.uint32)
        diff = np.nonzero(out != np.array(want[2], dtype=np.uint32))[0]
        assert diff.size == 0, (tag_, "d_order_out differs at", int(diff[0]), out[diff[0]:diff[0] + 4].tolist())
    assert tail_is_canary(f.order_t, 4 * kept), (tag_, "d_order_out written at or beyond kept")
    assert guards_intact(torch, f._guards[0], 3) and guards_intact(torch, f._guards[1], 8), (tag_, "totals guards")


def check_device(torch, dev, payload, ops, order, mt, S, ranges=None, flags=0, *, shift=0, op_cap=None,
                 payload_bytes=None, tag_=""):
    """Runs the filter on the device and compares it with the model: (Filtered,
    the model's triple)."""
    cap = max(len(ops), 1) if op_cap is None else op_cap
    table = device_table(torch, dev, payload, ops, order, mt, shift=shift, op_cap=cap)
    padded = np.concatenate([ops, np.zeros(max(cap - len(ops), 0), dtype=ops.dtype)])
    want = model_filter(payload, padded, order, mt, S, ranges, flags, op_cap=cap, payload_bytes=payload_bytes)
    f = run_device(torch, dev, table, S, ranges, flags, payload_bytes=payload_bytes)
    compare_device(torch, f, want, tag_)
    return f, want


# ---- tile and wave boundaries ----
def boundary_items(n, tile):
    """n entries whose user-key groups straddle every wave (64) and tile
    boundary: groups of 7 versions starting 3 entries before each boundary,
    single-version keys between them, and, from the second tile on, one group
    that covers a whole tile and more, so that at a snapshot above its
    sequences all of that tile is dropped."""
    items, i, g = [], 0, 0
    long_from, long_to, long_done = tile - 5, 2 * tile + 5, n <= 2 * tile  # covers tile 1 whole
    while i < n:
        if not long_done and i >= long_from:
            m = long_to - i
            items += [(b"key%07d" % g, tag(100 + m - v, 0 if v % 5 == 4 else 1), b"x") for v in range(m)]
            i += m
            long_done = True
        elif (i + 3) % 64 == 0:
            m = min(7, n - i)
            items += [(b"key%07d" % g, tag(20 - v, 0 if v == 2 else 1), b"y") for v in range(m)]
            i += m
        else:
            items.append((b"key%07d" % g, tag(5 + g % 3, 0 if g % 11 == 0 else 1), b"z"))
            i += 1
        g += 1
    assert len(items) == n
    return items


# ---- stress trials ----
STRESS_TRIALS = 100


def stress_trial(seed):
    """(payload, ops, order, mt, S, ranges, flags) of one trial: random_items
    over few keys and sequences (long groups), now and then an unparsed type
    byte, a random snapshot, the flag, and a few ranges cut from the keys."""
    from memtable_cases import random_items
    rng = np.random.default_rng(4000 + seed)
    n = int([0, 1, rng.integers(2, 70), rng.integers(70, 1200), rng.integers(1200, 4000)][int(rng.integers(5))])
    seqs = int(rng.choice([3, 12, 60]))
    items = random_items(rng, n, alphabet=int(rng.choice([2, 4])), maxlen=int(rng.choice([3, 10, 24])), seqs=seqs)
    if seed % 4 == 0:
        items = [(k, (t & ~0xFF) | 7, v) if rng.random() < 0.03 else (k, t, v) for k, t, v in items]
    gaps = [int(g) for g in rng.integers(0, 9, size=n)] if seed % 2 else None
    payload, ops, order, mt = table_of(items, gaps)
    S = int(rng.integers(0, seqs + 2))
    flags = BASE_LEVEL if seed % 3 else 0
    ranges = None
    if flags and n and seed % 2:
        keys = sorted({k for k, _, _ in items})
        ranges = []
        for _ in range(int(rng.integers(1, 5))):
            a, b = sorted(int(x) for x in rng.integers(0, len(keys), size=2))
            ranges.append((keys[a], keys[b]))
    return payload, ops, order, mt, S, ranges, flags
