"""Record lists and oracle helpers shared by the WAL encode tests
(test_wal_encode_size.py, test_gpu_wal_encode_device.py,
test_gpu_wal_encode_stress.py).  The reference for every byte is
oracle/wal_oracle.py's Writer."""
import numpy as np

import wal_oracle as W

B, H = W.BLOCK_SIZE, W.HEADER_SIZE
# dest_length values around every block edge the Writer distinguishes
EDGES = [0, 1, B - H - 1, B - H, B - H + 1, B - 1, B, 5 * B + 17]


def oracle_encode(recs, dest_length=0):
    d = bytearray()
    w = W.Writer(d, dest_length)
    for r in recs:
        w.add_record(r)
    return bytes(d)


def random_records(rng, n, maxlog=17):
    out = []
    for _ in range(n):
        ln = int(rng.integers(0, 1 << int(rng.integers(0, maxlog + 1))))
        out.append(rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes())
    return out


def writer_recipe(dest_length):
    """The records of tests/test_gpu_wal.py::test_encode_matches_writer."""
    rng = np.random.default_rng(dest_length)
    return [b"", b"foo"] + random_records(rng, 200) + [bytes(3 * B + 5), b""]


def trailer_edge(k, dest_length, fill=None):
    """A first record sized to leave exactly k bytes in its block, then b"",
    b"x" and a 2 B + 3 byte record: k < 7 makes a k-byte zero trailer, at k = 7
    the empty record's header ends flush with the block, at k = 8 it leaves a
    one-byte trailer.  When
    the Writer's first block has no room for such a record (fewer than 7 + k
    bytes left), the record runs on into the next block and leaves k bytes
    there: its FIRST fragment then has as little as zero bytes."""
    bo = dest_length % B
    if B - bo < H:
        bo = 0  # the Writer pads and starts a new block
    first = B - bo - H - k
    if first < 0:
        first = (B - bo - H) + (B - H - k)
    rng = np.random.default_rng(1000 * k + dest_length) if fill is None else fill
    mk = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    return [mk(first), b"", b"x", mk(2 * B + 3)]


def physical_records(log, dest_length):
    """W.wal_physical_records for a log appended at dest_length: the oracle's
    walker starts at a block boundary, so the existing bytes of the first block
    are stood in for by one unverified record of that size (dropped from the
    result) -- possible when they hold a header (>= 7 bytes) or nothing.
    For 1..6 existing bytes no record fits, and the walk is restated here."""
    bo = dest_length % B
    if bo == 0:
        return W.wal_physical_records(log)
    if bo >= H:
        prefix = bytes(4) + bytes([(bo - H) & 0xFF, (bo - H) >> 8, W.FULL]) + bytes(bo - H)
        got = W.wal_physical_records(prefix + log)
        assert got[0] == (0, bo - H, W.FULL)
        return [(p - bo, ln, t) for p, ln, t in got[1:]]
    out, pos = [], 0
    while pos < len(log):
        left = B - (bo + pos) % B
        if left < H:
            pos += left
            continue
        ln, t = log[pos + 4] | (log[pos + 5] << 8), log[pos + 6]
        out.append((pos, ln, t))
        pos += H + ln
    return out


def pack(recs):
    """(payload bytes, rec_off, rec_len) of records laid end to end."""
    ln = np.array([len(r) for r in recs], dtype=np.uint64)
    off = np.zeros(len(recs), dtype=np.uint64)
    if len(recs) > 1:
        off[1:] = np.cumsum(ln[:-1])
    return b"".join(recs), off, ln


# ---- GPU side: canary-guarded runs of encode_device ----
CANARY = 0xA5
GUARD = 64


def first_diff(got, want):
    if len(got) != len(want):
        return f"length {len(got)} != {len(want)}"
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    d = np.nonzero(a != b)[0]
    return None if d.size == 0 else f"first difference at byte {int(d[0])} of {len(want)}: {a[d[0]]} != {b[d[0]]}"


def to_dev(torch, data, dev, shift=0):
    """A uint8 tensor holding `data` whose first byte lies `shift` bytes past a
    16-B aligned address."""
    buf = torch.empty(len(data) + 32, dtype=torch.uint8, device=dev)
    base = (-buf.data_ptr()) % 16 + shift
    t = buf[base:base + len(data)]
    if len(data):
        t.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def encode_checked(torch, dev, payload, off, ln, dest_length=0, out_shift=0, pay_shift=0, stream=None):
    """encode_device into a canary-guarded buffer at the given alignments;
    returns (log bytes, whether both guards are intact)."""
    import lvgpu.wal as LW
    need, _ = LW.encode_size(ln, dest_length)
    d_pay = to_dev(torch, payload, dev, pay_shift)
    buf = torch.full((need + 2 * GUARD + 32,), CANARY, dtype=torch.uint8, device=dev)
    base = (-buf.data_ptr()) % 16 + out_shift + GUARD
    out = buf[base:base + need]
    got = LW.encode_device(d_pay, off, ln, dest_length, out=out, stream=stream)
    assert got.data_ptr() == out.data_ptr() and got.numel() == need
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    guards_ok = bool((host[:base] == CANARY).all() and (host[base + need:] == CANARY).all())
    return host[base:base + need].tobytes(), guards_ok
