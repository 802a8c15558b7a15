"""The SSTable build in Python, written straight from the format section of
include/lvgpu/table.h: BlockBuilder and TableBuilder objects and serial code
(no scans, no sizes ahead of the bytes), a model READER that opens what they
wrote, the case tables and the comparison helpers shared by test_sst_build.py
and test_gpu_sst_build_device.py.

model_build is the model every output of lv_sst_build_host and
lv_sst_build_device is compared with, byte for byte; read_table, walking the
footer, the index block and every data block's restart array, is the check
that the bytes mean the memtable's entries."""
import numpy as np

import memtable_cases as M
from memtable_cases import make_table, tag
from write_batch_cases import CANARY, GUARD, guarded_payload, tail_is_canary, varint

NO_TABLE, HANDLE_OVER, FILE_OVER, BLOCK_LARGE = 1, 2, 4, 8
BLOCK_SIZE, RESTART_INTERVAL = 4096, 16
MAXTAG = bytes([1]) + b"\xff" * 7
MAGIC = 0xDB4775248B80FB57
TOTALS = ("entries", "data_blocks", "file_bytes", "metaindex_offset", "metaindex_size", "index_offset",
          "index_size", "status")


def crc_lib():
    import lvgpu
    return lvgpu


def fixed32(v):
    return int(v).to_bytes(4, "little")


def ikey(key, t):
    return bytes(key) + int(t).to_bytes(8, "little")


def common_prefix(a, b):
    n = 0
    while n < len(a) and n < len(b) and a[n] == b[n]:
        n += 1
    return n


class BlockBuilder:
    def __init__(self, restart_interval):
        self.restart_interval = restart_interval
        self.buffer = bytearray()
        self.restarts = [0]
        self.counter = 0
        self.last_key = b""

    def add(self, key, value):
        if self.counter < self.restart_interval:
            shared = common_prefix(self.last_key, key)
        else:
            self.restarts.append(len(self.buffer))
            self.counter = 0
            shared = 0
        self.buffer += varint(shared) + varint(len(key) - shared) + varint(len(value)) + key[shared:] + value
        self.last_key = key
        self.counter += 1

    def estimate(self):
        return len(self.buffer) + 4 * len(self.restarts) + 4

    def empty(self):
        return not self.buffer

    def finish(self):
        return bytes(self.buffer) + b"".join(fixed32(r) for r in self.restarts) + fixed32(len(self.restarts))


def user(k):
    return k[:-8]


def shortest_separator(a, b):
    ua, ub = user(a), user(b)
    d = common_prefix(ua, ub)
    if d >= min(len(ua), len(ub)):
        return a
    c = ua[d]
    if c < 0xFF and c + 1 < ub[d]:
        return ua[:d] + bytes([c + 1]) + MAXTAG
    return a


def short_successor(a):
    ua = user(a)
    for i, c in enumerate(ua):
        if c != 0xFF:
            t = ua[:i] + bytes([c + 1])
            return t + MAXTAG if len(t) < len(ua) else a
    return a


def handle_encoding(offset, size):
    return varint(offset) + varint(size)


def trailer(raw):
    L = crc_lib()
    return b"\x00" + fixed32(L.mask(L.value(raw + b"\x00")))


class TableBuilder:
    def __init__(self, block_size=BLOCK_SIZE, restart_interval=RESTART_INTERVAL):
        self.block_size, self.restart_interval = block_size, restart_interval
        self.file = bytearray()
        self.data = BlockBuilder(restart_interval)
        self.index = BlockBuilder(1)
        self.pending = None
        self.last_key = b""
        self.handles = []

    def write_block(self, raw):
        h = (len(self.file), len(raw))
        self.file += raw + trailer(raw)
        return h

    def flush(self):
        self.pending = self.write_block(self.data.finish())
        self.handles.append(self.pending)
        self.data = BlockBuilder(self.restart_interval)

    def add(self, key, value):
        if self.pending is not None:
            self.index.add(shortest_separator(self.last_key, key), handle_encoding(*self.pending))
            self.pending = None
        self.last_key = key
        self.data.add(key, value)
        if self.data.estimate() >= self.block_size:
            self.flush()

    def finish(self):
        if not self.data.empty():
            self.flush()
        meta = self.write_block(BlockBuilder(self.restart_interval).finish())
        if self.pending is not None:
            self.index.add(short_successor(self.last_key), handle_encoding(*self.pending))
            self.pending = None
        index = self.write_block(self.index.finish())
        footer = handle_encoding(*meta) + handle_encoding(*index)
        self.file += footer + bytes(40 - len(footer)) + MAGIC.to_bytes(8, "little")
        return meta, index


def entries_of(payload, ops, order=None):
    """[(internal key, value)] of the op table in memtable order."""
    order = M.model_order(payload, ops) if order is None else order
    out = []
    for i in order:
        o = ops[int(i)]
        vo, vl = int(o["val_off"]), int(o["val_len"])
        out.append((ikey(M.key_of(payload, o), int(o["tag"])), payload[vo:vo + vl]))
    return out


def model_build(payload, ops, block_size=BLOCK_SIZE, restart_interval=RESTART_INTERVAL, order=None):
    """(file bytes, handles [(offset, size)] of data blocks + metaindex + index,
    totals dict) of the flush of (payload, ops)."""
    ents = entries_of(payload, ops, order)
    if not ents:
        return b"", [], dict(zip(TOTALS, [0] * 8))
    tb = TableBuilder(block_size, restart_interval)
    for k, v in ents:
        tb.add(k, v)
    meta, index = tb.finish()
    tot = dict(entries=len(ents), data_blocks=len(tb.handles), file_bytes=len(tb.file), metaindex_offset=meta[0],
               metaindex_size=meta[1], index_offset=index[0], index_size=index[1], status=0)
    return bytes(tb.file), tb.handles + [meta, index], tot


# ---- the model reader ----
def get_varint(b, at):
    v, shift = 0, 0
    while True:
        c = b[at]
        at += 1
        v |= (c & 0x7F) << shift
        if not c & 0x80:
            return v, at
        shift += 7


def read_block(file, offset, size):
    """The raw block at a handle, its trailer checked."""
    raw = file[offset:offset + size]
    assert len(raw) == size and file[offset + size:offset + size + 5] == trailer(raw), ("trailer", offset, size)
    return raw


def block_entries(raw):
    """[(key, value)] of a block, walked restart by restart: every restart
    offset must be where an entry with shared == 0 starts, the entries of one
    restart run must end where the next begins, and the last at the array."""
    n = int.from_bytes(raw[-4:], "little")
    arr = len(raw) - 4 - 4 * n
    assert n >= 1 and arr >= 0
    restarts = [int.from_bytes(raw[arr + 4 * i:arr + 4 * i + 4], "little") for i in range(n)]
    assert restarts[0] == 0 and restarts == sorted(set(restarts))
    out = []
    for r, start in enumerate(restarts):
        end = restarts[r + 1] if r + 1 < n else arr
        at, key = start, b""
        while at < end:
            first = at == start
            shared, at = get_varint(raw, at)
            non_shared, at = get_varint(raw, at)
            vlen, at = get_varint(raw, at)
            assert shared <= len(key) and not (first and shared), ("shared", r, at, shared)
            key = key[:shared] + raw[at:at + non_shared]
            at += non_shared
            out.append((key, raw[at:at + vlen]))
            at += vlen
        assert at == end, ("restart run overruns", r, at, end)
    return out, restarts


def internal_less(a, b):
    """InternalKeyComparator over two internal keys."""
    ua, ub = user(a), user(b)
    if ua != ub:
        return ua < ub
    return int.from_bytes(a[-8:], "little") > int.from_bytes(b[-8:], "little")


def read_table(file):
    """Opens a table image: (entries [(internal key, value)], index
    [(key, (offset, size))], per-block entry lists)."""
    assert len(file) >= 48 and int.from_bytes(file[-8:], "little") == MAGIC
    foot = file[-48:]
    mo, at = get_varint(foot, 0)
    ms, at = get_varint(foot, at)
    io, at = get_varint(foot, at)
    isz, at = get_varint(foot, at)
    assert foot[at:40] == bytes(40 - at)
    assert block_entries(read_block(file, mo, ms))[0] == []
    idx, idx_restarts = block_entries(read_block(file, io, isz))
    assert len(idx_restarts) == max(len(idx), 1)  # restart_interval 1
    index, blocks, entries = [], [], []
    for key, value in idx:
        o, at = get_varint(value, 0)
        s, at = get_varint(value, at)
        assert at == len(value)
        index.append((key, (o, s)))
        ents, _ = block_entries(read_block(file, o, s))
        assert ents
        blocks.append(ents)
        entries += ents
    return entries, index, blocks


def index_seek(index, blocks, target):
    """Table::InternalGet's path: the first index entry whose key is not less
    than target names the block; the first entry there not less than target."""
    for (key, _), ents in zip(index, blocks):
        if not internal_less(key, target):
            for k, v in ents:
                if not internal_less(k, target):
                    return k, v
            return None  # (the next block's first entry, for an iterator)
    return None


# ---- cases ----
def seq_items(n, klen=6, vlen=3, start=0):
    return [(b"%0*d" % (klen, start + i), tag(100 + i), b"v" * vlen) for i in range(n)]


def cases():
    """name -> (items, block_size, restart_interval): the smallest shapes at
    which each mechanism can go wrong."""
    c = {}
    D = (BLOCK_SIZE, RESTART_INTERVAL)
    for n in (0, 1, 15, 16, 17, 32, 33):
        c[f"count_{n}"] = (seq_items(n), *D)
    # a block whose end coincides with a restart: entries of 15 bytes (1+1+1+ (1+8) shared 3 of "k00i"... )
    c["end_on_restart"] = (seq_items(40, klen=4, vlen=2), 64, 4)
    # the estimate after the deciding entry at block_size - 1, block_size, block_size + 1
    for d in (-1, 0, 1):
        # two entries, no shared prefix; estimate = 32 + (1 + 1 + 2 + 9 + vlen) + 4 + 4 with a 2-byte varint(vlen)
        first = (b"a", tag(1), b"x" * 20)  # 1 + 1 + 1 + 9 + 20 = 32
        vlen = 200 + d - 32 - 8 - 4 - 9
        c[f"threshold_{d:+d}"] = ([first, (b"b", tag(2), b"y" * vlen), (b"c", tag(3), b"z")], 200, 16)
    c["one_big_entry"] = ([(b"a", tag(1), b"s"), (b"big", tag(2), b"B" * 9000), (b"c", tag(3), b"t")], *D)
    # shared prefixes across the key / tag boundary, both ways
    c["tag_high_byte"] = ([(b"same", tag((s << 40) | 7), b"v") for s in (1, 2, 3, 200)], *D)
    c["tag_into_key"] = ([(b"a", tag(5), b"1"), (b"a\x01\x05" + bytes(5) + b"zz", tag(9), b"2"),
                          (b"a\x01\x05", tag(1), b"3")], *D)
    c["duplicates"] = ([(b"dup", tag(42), b"same")] * 3 + [(b"dup", tag(42, 0), b"")] * 2, *D)
    c["empty_and_deleted"] = ([(b"", tag(3), b""), (b"", tag(2, 0), b""), (b"k", tag(1), b""), (b"k", tag(9, 0), b""),
                               (b"z", tag(4), b"val")], *D)
    for w in (127, 128, 16383, 16384):
        base = b"P" * w
        c[f"varint_shared_{w}"] = ([(base + b"a", tag(1), b"v"), (base + b"b", tag(2), b"w")], 1 << 20, 16)
        c[f"varint_nonshared_{w}"] = ([(b"K" * (w - 8), tag(1), b"v")] if w > 8 else [], 1 << 20, 16)
        c[f"varint_value_{w}"] = ([(b"k", tag(1), b"V" * w), (b"l", tag(2), b"W" * w)], 1 << 20, 16)
    # separators: every block one entry (block_size 1)
    sep = {"prefix_of_next": [b"abc", b"abcd"], "next_shorter": [b"abcd", b"abd"], "same_user_key": [b"same", b"same"],
           "differs_at_ff": [b"ab\xffq", b"ac"], "plus_one_is_limit": [b"abc", b"abd"],
           "shortened": [b"abcd", b"abz"], "shortened_first_byte": [b"a", b"c"]}
    for name, keys in sep.items():
        c[f"sep_{name}"] = ([(k, tag(9 - i), b"v") for i, k in enumerate(keys)], 1, 16)
    for name, key in {"empty": b"", "all_ff": b"\xff\xff\xff", "ff_ff_41": b"\xff\xff\x41\x42\x43", "one_byte": b"k",
                      "first_byte": b"hello"}.items():
        c[f"succ_{name}"] = ([(key, tag(1), b"v")], *D)
    # many blocks over keys with shared stems, deletions, duplicates
    rng = np.random.default_rng(5)
    c["random_small_blocks"] = (M.random_items(rng, 300, alphabet=3, maxlen=12, seqs=6), 64, 4)
    c["random_default"] = (M.random_items(rng, 500, alphabet=4, maxlen=30, seqs=50), *D)
    c["corner_keys"] = (M.corner_items(), 256, 3)
    c["tags"] = (M.tag_items(), 48, 2)
    return c


def tile_items(n, seed=0):
    """n entries of 14-20 bytes behind shared stems: with block_size 32 a block
    holds one to three of them, so the chain of block starts crosses every
    tile edge at a place the data decides."""
    rng = np.random.default_rng(1000 + seed)
    return [(b"k%05d" % (i // 2) + b"x" * int(rng.integers(0, 3)), tag(int(rng.integers(1, 4)), int(rng.integers(0, 2))),
             b"v" * int(rng.integers(0, 4))) for i in range(n)]


def adversarial_tables(rng, trials=200):
    """Random tables for the file bound: tiny and huge keys, empty values, one
    entry per block, long shared prefixes."""
    for t in range(trials):
        n = int(rng.integers(1, 40))
        kind = t % 4
        items = []
        for i in range(n):
            if kind == 0:
                key = bytes(rng.integers(0, 256, size=int(rng.integers(0, 4)), dtype=np.uint8))
            elif kind == 1:
                key = bytes(rng.integers(0, 256, size=int(rng.integers(100, 400)), dtype=np.uint8))
            elif kind == 2:
                key = b"S" * int(rng.integers(0, 300)) + bytes(rng.integers(0, 256, size=2, dtype=np.uint8))
            else:
                key = b"\xff" * int(rng.integers(0, 5)) + bytes(rng.integers(250, 256, size=3, dtype=np.uint8))
            val = b"" if rng.random() < 0.5 else b"v" * int(rng.integers(0, 200))
            items.append((key, tag(int(rng.integers(0, 5)), int(rng.integers(0, 2))), val))
        yield items, int(rng.choice([1, 7, 64, 300, 4096])), int(rng.choice([1, 2, 16, 1024]))


# ---- one device call ----
def run_device(torch, dev, payload, ops, block_size=BLOCK_SIZE, restart_interval=RESTART_INTERVAL, *, shift=0,
               file_cap=None, block_cap=None, mt_status=0, op_cap=None, stream=None):
    """lv_memtable_build_device, then lv_sst_build_device over its outputs on a
    guarded payload, with a canary-filled file and handle array and a dirty
    workspace.  Returns the lvgpu.table.Built."""
    import lvgpu.table as T
    table, buf = M.run_build(torch, dev, payload, ops, shift=shift, op_cap=op_cap, stream=stream)
    if mt_status:
        table.totals[2] = mt_status
    want_file, want_handles, _ = model_build(payload, ops, block_size or BLOCK_SIZE, restart_interval or RESTART_INTERVAL)
    fc = len(want_file) if file_cap is None else file_cap
    bc = max(len(want_handles) - 2, 0) if block_cap is None else block_cap
    ws = torch.full((max(T.build_workspace_bytes(table.op_cap, bc), 16),), 0x5A, dtype=torch.uint8, device=dev)
    built = T.build_device(table, block_size=block_size, restart_interval=restart_interval, file_cap=fc, block_cap=bc,
                           workspace=ws, stream=stream, fill=CANARY, guard=GUARD)
    built._buf = buf
    return built


def compare_device(built, payload, ops, block_size=BLOCK_SIZE, restart_interval=RESTART_INTERVAL, tag_=""):
    """The image, the handles and the totals of a call whose status is 0
    against the model, and the canaries behind both outputs."""
    want_file, want_handles, want_tot = model_build(payload, ops, block_size, restart_interval)
    t = built.sync_totals()
    assert t == want_tot, (tag_, t, want_tot)
    got = built.file()
    if got != want_file:
        at = next(i for i, (a, b) in enumerate(zip(got, want_file)) if a != b)
        raise AssertionError((tag_, "file differs at", at, got[at:at + 16].hex(), want_file[at:at + 16].hex()))
    assert built.handles() == want_handles, (tag_, built.handles()[:4], want_handles[:4])
    assert tail_is_canary(built.file_t, len(want_file)), (tag_, "d_file written at or beyond file_bytes")
    assert tail_is_canary(built.handles_t, 16 * len(want_handles)), (tag_, "d_handles written beyond its count")
    return want_file, want_handles


def check_device(torch, dev, items, block_size=BLOCK_SIZE, restart_interval=RESTART_INTERVAL, *, shift=0, gaps=None,
                 tag_="", **kw):
    payload, ops = make_table(items, gaps)
    built = run_device(torch, dev, payload, ops, block_size, restart_interval, shift=shift, **kw)
    compare_device(built, payload, ops, block_size, restart_interval, tag_)
    return built, payload, ops
