"""Inputs of the loop-trip tests (test_gpu_loop_trips.py) that are built from a
motif tiled with numpy, so that a log of thousands of blocks or a batch of
millions of records gets its expected outputs from one run of the Python model
over the motif.  test_loop_trips_models.py ties each tiling to the model run
on three whole repetitions."""
import numpy as np

import wal_oracle as W
import write_batch_cases as C
from wal_decode_cases import flip, headers, oracle_read
from wal_encode_cases import B, H, oracle_encode

# ---- WriteBatch: a motif of 997 records (prime: tile edges move through it) ----
WB_MOTIF = 997


def wb_motif():
    """(payload, rec_off, rec_len) of the motif: lane-class records of 0 to 40
    ops (most have one), two wave-class records (longer than kWbSmall, one of
    them malformed at its end), a record with count 0, one malformed record
    of each status, and an extent beyond the payload."""
    from lvgpu.write_batch import WB_SMALL
    rng = np.random.default_rng(4242)
    reps = []
    for i in range(WB_MOTIF):
        nops = int(rng.integers(0, 41)) if i % 53 == 7 else (0 if i % 97 == 3 else 1 + int(rng.integers(0, 3)) // 2)
        reps.append(C.mixed_batch(nops, seed=9000 + i, seq=(i + 1) << 20, maxlen=12).bytes())
    assert any(C.iterate_ext(r)[3] == 0 for r in reps) and max(len(C.iterate_ext(r)[1]) for r in reps) >= 35
    reps[100] = C.wave_batch(WB_SMALL, nops=30, seed=5, seq=77 << 30)
    reps[611] = C.wave_batch(WB_SMALL, nops=70, seed=6, seq=78 << 30)[:-3]  # BAD_LENGTH after its ops
    put_ab = bytes([C.VALUE, 1]) + b"a" + bytes([1]) + b"b"
    bad = {200: bytes(5),                                        # TOO_SMALL
           201: C.hdr(1, 1) + bytes([C.DELETION, 0x80]),         # BAD_VARINT
           202: C.hdr(1, 1) + bytes([C.DELETION, 3]) + b"ab",    # BAD_LENGTH
           203: C.hdr(1, 2) + put_ab,                            # WRONG_COUNT
           204: C.hdr(1, 2) + put_ab + bytes([2, 0])}            # BAD_TAG
    for i, r in bad.items():
        reps[i] = r
    payload, off, ln = C.pack(reps, gaps=[int(rng.integers(0, 5)) for _ in reps])
    ln[205] = 1 << 62  # OUT_OF_RANGE, however long the payload grows by repetition
    return payload, off, ln


def wb_tiled(motif_model, motif_bytes, n):
    """The model's outputs for the first n records of the motif repeated end to
    end (every repetition's payload is a copy of the motif's, motif_bytes
    further on): (ops, bounds, statuses, totals)."""
    m_ops, m_bounds, m_st, m_tot = motif_model
    R = len(m_st)
    assert n >= R  # (the last sequence is the motif's)
    reps = -(-n // R)
    k_ops = len(m_ops)
    ops = np.tile(m_ops, reps)
    shift = np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(motif_bytes), k_ops)
    ops["key_off"] += shift
    ops["val_off"] += shift
    bounds = (np.tile(m_bounds[:-1], reps).reshape(reps, R) +
              (np.arange(reps, dtype=np.uint64) * np.uint64(k_ops))[:, None]).reshape(-1)
    bounds = np.concatenate([bounds, [np.uint64(reps * k_ops)]]).astype(np.uint64)[: n + 1]
    st = np.tile(m_st, reps)[:n]
    ops = ops[: int(bounds[n])]
    tot = dict(records=n, ops=int(bounds[n]), key_bytes=int(ops["key_len"].sum(dtype=np.uint64)),
               value_bytes=int(ops["val_len"].sum(dtype=np.uint64)), bad_records=int((st != C.OK).sum()),
               last_sequence=m_tot["last_sequence"], status=0)
    return ops, bounds, st, tot


def wb_tiled_inputs(payload, off, ln, n):
    """(payload, rec_off, rec_len) of the first n records of the repeated motif."""
    R = len(off)
    reps = -(-n // R)
    base = np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(len(payload)), R)
    return payload * reps, (np.tile(off, reps) + base)[:n], np.tile(ln, reps)[:n]


# ---- WAL: a motif of an odd number of whole 32 KiB blocks ----
def wal_motif(min_blocks=36):
    """(records, log): blocks of one to several hundred fragments, FIRST /
    MIDDLE / LAST chains, a record over three blocks, block tails shorter than
    a header, ending exactly on a block boundary after an odd number of
    blocks."""
    rng = np.random.default_rng(808)
    mk = lambda k: rng.integers(0, 256, size=k, dtype=np.uint8).tobytes()
    recs = []
    size = lambda: len(oracle_encode(recs))

    def fill_to(left):
        """One record that leaves exactly `left` bytes in its block."""
        room = B - size() % B
        if room < H:
            room = B  # the Writer pads the tail and starts a block
        k = room - H - left
        if k < 0:
            k += B - H  # (runs on into the next block as FIRST + LAST)
        recs.append(mk(k))
    recs += [mk(int(rng.integers(0, 40))) for _ in range(700)]      # ~60 B apiece: hundreds of fragments a block
    fill_to(3)                                                      # a 3-byte zero trailer
    recs += [mk(2 * B + 4000)]                                      # three blocks: FIRST, MIDDLE, LAST
    recs += [mk(int(rng.integers(50, 200))) for _ in range(500)]
    fill_to(6)
    recs += [mk(B - H)]                                             # one fragment fills a block
    recs += [mk(int(rng.integers(0, 3000))) for _ in range(60)]
    fill_to(0)
    recs += [mk(int(rng.integers(0, 16))) for _ in range(4000)]    # ~15 B apiece: over a thousand a block
    fill_to(7)                                                      # then an empty record's header ends the block
    recs += [b""]
    while size() < min_blocks * B:
        recs += [mk(int(rng.integers(0, 1 << int(rng.integers(4, 17))))) for _ in range(20)]
        recs += [mk(int(rng.integers(0, 30))) for _ in range(300)]
    fill_to(0)
    if (size() // B) % 2 == 0:
        recs += [mk(B - H)]
    log = oracle_encode(recs)
    assert len(log) % B == 0 and (len(log) // B) % 2 == 1
    return recs, log


def wal_flip_at(log, block):
    """The position of a payload byte of the second fragment with one that
    starts in `block` (the first if it is the only one), and that fragment's
    header offset."""
    fr = [h for h in headers(log) if h[0] // B == block and h[1] > 0]
    p, ln, _ = fr[min(1, len(fr) - 1)]
    return p + H + ln // 2, p


class WalTiled:
    """The Reader model of the motif's log repeated `reps` times, with one byte
    flipped in the repetitions named in `flips` ({repetition: motif block})."""

    def __init__(self, log, reps, flips):
        self.log, self.reps, self.flips = log, reps, dict(flips)
        self.L = len(log)
        self.variants = {None: oracle_read(log)}
        self.flip_pos = {}
        for blk in set(self.flips.values()):
            bad = bytearray(log)
            pos, hdr = wal_flip_at(log, blk)
            flip(bad, pos)
            self.variants[blk] = oracle_read(bytes(bad))
            self.flip_pos[blk] = (pos, hdr)

    def full_log(self):
        out = np.tile(np.frombuffer(self.log, dtype=np.uint8), self.reps)
        for rep, blk in self.flips.items():
            out[rep * self.L + self.flip_pos[blk][0]] ^= 0x40
        return out

    def expected(self):
        """(payload bytes, rec_len, rec_log_off, [(bytes, reason)], dropped bytes,
        {index of a flip's first report: its header's log offset})."""
        pay, lens, offs, reps_, dropped, at = [], [], [], [], 0, {}
        cache = {}
        for k in range(self.reps):
            v = self.flips.get(k)
            if v not in cache:
                recs, ro, rp, dr = self.variants[v]
                cache[v] = (b"".join(recs), np.array([len(r) for r in recs], dtype=np.int64),
                            np.array(ro, dtype=np.int64), rp, dr)
            p, ln, ro, rp, dr = cache[v]
            pay.append(p)
            lens.append(ln)
            offs.append(ro + k * self.L)
            if v is not None:
                at[len(reps_)] = k * self.L + self.flip_pos[v][1]
            reps_ += rp
            dropped += dr
        return b"".join(pay), np.concatenate(lens), np.concatenate(offs), reps_, dropped, at


# ---- Bloom build: one-entry data blocks, 1 to 40 of them to a filter window ----
def bloom_items(n):
    """n entries in key order for block_size 1 (every entry its own data
    block), their values sized so that stretches of the file hold about c block
    starts per 2 KiB filter window, c drawn from 1..40 for each stretch of 20
    blocks (about a ninth of the blocks are then the first of a window, so the
    LDS slot of many a wave builds a second filter, as often a smaller one as a
    larger); at c = 1 blocks of two windows each, so a window holds exactly one
    start and the window behind it none."""
    from memtable_cases import tag
    rng = np.random.default_rng(515)
    items, i = [], 0
    while len(items) < n:
        c = int(rng.integers(1, 41))
        vlen = 4090 if c == 1 else max(2048 // c - 36, 0)
        for _ in range(20):
            items.append((b"key%07d" % i, tag(10 + i % 7), bytes([65 + i % 26]) * (vlen + i % 3)))
            i += 3  # (keys 3 i + 1 are absent)
    return items[:n]


# ---- Table scan: a restart run per entry, known by construction ----
SCAN_BLOCK = 4096  # block_size; restart_interval is 1


def scan_ops(n):
    """(payload, ops) of n entries already in memtable order: entry i has the
    user key i as 8 big-endian bytes, sequence i + 1, every 7th a deletion, and
    otherwise a value of (i // 500) % 3 bytes, the key's last ones (the low
    bytes of i): stretches of entries of one size, so the blocks hold from 166
    to 178 entries and their edges move through the scan tiles."""
    from lvgpu.write_batch import OP_DTYPE
    i = np.arange(n, dtype=np.uint64)
    payload = i.astype(">u8").tobytes()
    dele = i % np.uint64(7) == 6
    ops = np.zeros(n, dtype=OP_DTYPE)
    ops["tag"] = ((i + np.uint64(1)) << np.uint64(8)) | (~dele).astype(np.uint64)
    ops["key_off"], ops["key_len"] = np.uint64(8) * i, 8
    ops["val_len"] = np.where(dele, 0, i // np.uint64(500) % np.uint64(3)).astype(np.uint32)
    ops["val_off"] = ops["key_off"] + np.uint64(8) - ops["val_len"].astype(np.uint64)
    return payload, ops


def scan_layout(val_len):
    """The data blocks of scan_ops' table under block_size SCAN_BLOCK and
    restart_interval 1, by the builder's rule in numpy: an entry is 3 length
    bytes, the 16-byte internal key and the value, with a 4-byte restart of its
    own; a block ends with the first entry that brings buffer + restarts + 4
    to the block size.  (first entry of each block and n behind them, block
    offsets, block sizes, the offset of every entry in its block)."""
    size = 19 + np.asarray(val_len, dtype=np.int64)
    n = size.size
    c = np.cumsum(size + 4)
    first, a = [], 0
    while a < n:
        first.append(a)
        a = int(np.searchsorted(c, (c[a - 1] if a else 0) + SCAN_BLOCK - 4)) + 1
    first = np.array(first + [n], dtype=np.int64)
    b = np.concatenate([[0], np.cumsum(size)])
    counts = np.diff(first)
    bsize = b[first[1:]] - b[first[:-1]] + 4 * counts + 4
    boff = np.concatenate([[0], np.cumsum(bsize + 5)[:-1]])
    at = b[:-1] - np.repeat(b[first[:-1]], counts)
    return first, boff, bsize, at


# ---- Bloom build: one-entry 4 KiB blocks and a few crowded ones ----
BLOOM_BIG_BLOCK = 4096  # block_size
BLOOM_BIG_CROWD = 280   # entries without a value in front of a crowded block's big entry


def bloom_big_items(nblocks, crowded):
    """(items in key order, {crowded block: (index of its first item, items)})
    for block_size 4096: every block ends with an entry whose value fills a
    block by itself, so a block is one entry of about 4,125 bytes and every
    second or third 2 KiB window holds one block start; the blocks named in
    `crowded` begin with BLOOM_BIG_CROWD more entries of about 12 bytes
    (prefix-compressed 10-byte keys, no value), so at 64 bits per key the
    filter of such a block's window is beyond the 2,048 bytes a wave of
    sb_bloom_emit builds in LDS, between the 9-byte filters of its neighbours.
    Keys are key%07d of multiples of 3."""
    from memtable_cases import tag
    items, where, i = [], {}, 0

    def put(vlen):
        nonlocal i
        items.append((b"key%07d" % i, tag(10 + i % 7), bytes([65 + i % 26]) * vlen))
        i += 3  # (keys 3 i + 1 are absent)
    for b in range(nblocks):
        if b in crowded:
            where[b] = (len(items), BLOOM_BIG_CROWD + 1)
            for _ in range(BLOOM_BIG_CROWD):
                put(0)
        put(BLOOM_BIG_BLOCK - 6 + i % 3)
    return items, where
