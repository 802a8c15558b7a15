"""The store as a whole: a plain model of its history, a seeded workload and a
driver that walks log bytes -> memtable -> level-0 table -> compaction -> a
level run -> MANIFEST -> reopen through the library, over two backends (the
host twins, the device entry points), shared by test_store.py and
test_gpu_store.py.

StoreModel is written from the reference alone: a batch's ops take sequence,
sequence + 1, ... (write_batch.rs:142-154, WriteBatchInternal::set_sequence and
the MemTableInserter), and Get returns the newest entry of the user key with
sequence <= snapshot, a deletion hiding what lies beneath it (memtable.rs:105-143
over the LookupKey of dbformat.rs:96-103).  It imports none of the stage models
(*_cases.py): a convention two stage models share wrongly shows up against it.

Store keeps between operations only what a host keeps: the bytes of the two
logs and of the image arena, the file directory (number -> offset and size in
the arena), the applied version and the counters of a VersionSet.  Inside an
operation the device backend hands counts and statuses on in device memory."""
import ctypes
from types import SimpleNamespace

import numpy as np

import lvgpu.compact as CP
import lvgpu.memtable as MT
import lvgpu.table as T
import lvgpu.version as V
import lvgpu.version_edit as VE
import lvgpu.wal as LW
import lvgpu.write_batch as WB
import wal_oracle as W

FOUND, DELETED, ABSENT = "FOUND", "DELETED", "ABSENT"
DELETION, VALUE = 0, 1                      # dbformat.rs:39-40
MAX = (1 << 56) - 1                         # dbformat.rs:35
STATUS = {0: ABSENT, 1: FOUND, 2: DELETED}  # LV_MT_GET_* == LV_SST_GET_* for the three answers
CANARY, GUARD = 0xA5, 64
OPT = dict(block_size=256, restart_interval=4)
BITS_PER_KEY = 10
MAX_FILE_BYTES = 2048
HAS = VE.HAS_LOG_NUMBER | VE.HAS_NEXT_FILE | VE.HAS_LAST_SEQUENCE
FAULTS = ("ranges_omitted", "first_sequence_off_by_one", "level0_oldest_first", "compaction_inputs_not_removed",
          "dest_length_zero", "floor_ignored")


# ---- the model -------------------------------------------------------------------
class StoreModel:
    """history[user_key] = [(seq, type, value)] in write order."""

    def __init__(self):
        self.history = {}
        self.last_sequence = 0

    def apply(self, batch):
        for typ, key, value in batch:
            self.last_sequence += 1
            self.history.setdefault(key, []).append((self.last_sequence, typ, value if typ == VALUE else b""))

    def newest(self, key, snapshot):
        best = None
        for e in self.history.get(key, ()):
            if e[0] <= snapshot and (best is None or e[0] > best[0]):
                best = e
        return best

    def get(self, key, snapshot):
        e = self.newest(key, snapshot)
        if e is None:
            return ABSENT, None
        return (FOUND, e[2]) if e[1] == VALUE else (DELETED, None)

    def range(self, lo, hi, snapshot, limit):
        out = []
        for key in sorted(self.history):
            if key < lo or (hi is not None and key >= hi):
                continue
            st, v = self.get(key, snapshot)
            if st == FOUND:
                out.append((key, v))
                if len(out) == limit:
                    break
        return out


# ---- the workload ----------------------------------------------------------------
def universe():
    """About 120 user keys in key order: the empty key, keys that are prefixes
    of one another, a long key and its extension."""
    keys = {b"", b"a", b"ab", b"abc", b"abc\x00", b"abd", b"k", b"k0", b"k05", b"k050", b"k0500", b"k05\xff",
            b"z" * 200, b"z" * 200 + b"!", b"\xff", b"\xff\xff"}
    keys |= {b"k%03d" % i for i in range(0, 208, 2)}
    return sorted(keys)


WINDOWS = ((0.0, 0.7), (0.3, 1.0), (0.45, 0.7), (0.55, 0.85))  # the share of the key space a generation writes


def generation(rng, keys, g, n_ops=1500, big=False):
    """Generation g (0-based) as three groups of batches of (type, key, value):
    batches of 1 to 40 ops, deletions and re-puts over few keys, the empty
    value, and with `big` one value above 4 KiB."""
    lo, hi = WINDOWS[g % len(WINDOWS)]
    window = keys[int(lo * len(keys)): max(int(hi * len(keys)), int(lo * len(keys)) + 2)]
    sizes = [40, 1]
    while sum(sizes) < n_ops:
        sizes.append(int(min(40, rng.geometric(0.22))))
    rng.shuffle(sizes)
    batches, at_big = [], int(rng.integers(len(sizes)))
    for b, n in enumerate(sizes):
        batch = []
        for _ in range(n):
            key = window[int(rng.integers(len(window)))]
            if rng.random() < 0.42:
                batch.append((DELETION, key, b""))
            else:
                ln = 0 if rng.random() < 0.05 else int(rng.integers(1, 40))
                batch.append((VALUE, key, rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes()))
        if big and b == at_big:
            batch[0] = (VALUE, batch[0][1], rng.integers(0, 256, size=4200, dtype=np.uint8).tobytes())
        batches.append(batch)
    cut = (len(batches) // 3, 2 * len(batches) // 3)
    return [batches[: cut[0]], batches[cut[0]: cut[1]], batches[cut[1]:]]


def user(ikey):
    return bytes(ikey[:-8])


def tag_of(ikey):
    return int.from_bytes(ikey[-8:], "little")


def pack_queries(queries):
    """[(key, seq)] as (key bytes, offsets, lengths, sequences), a gap byte between keys."""
    qk, off, ln = bytearray(), [], []
    for key, _ in queries:
        qk += b"\xee"
        off.append(len(qk))
        ln.append(len(key))
        qk += key
    return (bytes(qk), np.array(off, dtype=np.int64), np.array(ln, dtype=np.int32),
            np.array([s for _, s in queries], dtype=np.int64))


def scan_size(image, tab):
    """(entries, key and value bytes) of a table image: lv_sst_scan_host's sizing pass."""
    L = T._bind_scan()
    t = T.SstTable(*[int(tab[n]) for n in T.TABLE_FIELDS])
    tot = T.ScanTotals()
    rc = L.lv_sst_scan_host(bytes(image), ctypes.byref(t), None, None, 0, None, 0, None, None, ctypes.byref(tot))
    assert rc == 0 and not tot.status & ~(T.SCAN_OP_OVER | T.SCAN_ARENA_OVER), (rc, tot.status)  # the true sizes
    return int(tot.entries), int(tot.arena_bytes)


def edit_rows(edit, src, files, deleted):
    """One VersionEdit as the row tables of lvgpu.version_edit: `files` are
    (level, number, size, smallest_off, smallest_len, largest_off, largest_len)
    over src, `deleted` (level, number)."""
    e = np.zeros(1, dtype=VE.EDIT_DTYPE)
    e["log_number"], e["next_file_number"], e["last_sequence"], e["has"] = (edit["log_number"], edit["next_file_number"],
                                                                            edit["last_sequence"], HAS)
    f = np.zeros(len(files), dtype=VE.FILE_DTYPE)
    for row, (level, number, size, so, sl, lo, ll) in zip(f, files):
        row["level"], row["number"], row["file_size"] = level, number, size
        row["smallest_off"], row["smallest_len"], row["largest_off"], row["largest_len"] = so, sl, lo, ll
    d = np.zeros(len(deleted), dtype=VE.DELETED_DTYPE)
    for row, (level, number) in zip(d, deleted):
        row["level"], row["number"] = level, number
    return e, f, d


def blocks_ok(image, handles):
    """Every block's trailer: the type byte 0 and the masked CRC32C of the
    contents and the type (table.h), by the oracle's CRC."""
    for off, size in handles:
        body = image[off: off + size + 1]
        if len(body) != size + 1 or body[-1] != 0:
            return False
        if W.mask(W.value(body)) != int.from_bytes(image[off + size + 1: off + size + 5], "little"):
            return False
    return True


def decoded_edits(pay, edits, files, deleted, bf, bd):
    out = []
    for r, e in enumerate(edits):
        fs = [(int(f["level"]), int(f["number"]), int(f["file_size"]),
               pay[int(f["smallest_off"]): int(f["smallest_off"]) + int(f["smallest_len"])],
               pay[int(f["largest_off"]): int(f["largest_off"]) + int(f["largest_len"])])
              for f in files[int(bf[r]): int(bf[r + 1])]]
        ds = [(int(d["level"]), int(d["number"])) for d in deleted[int(bd[r]): int(bd[r + 1])]]
        out.append(dict(has=int(e["has"]), status=int(e["status"]), log_number=int(e["log_number"]),
                        next_file_number=int(e["next_file_number"]), last_sequence=int(e["last_sequence"]),
                        files=fs, deleted=ds))
    return out


# ---- the host backend ------------------------------------------------------------
class HostBackend:
    """The *_host twins; the log is framed by the oracle's Writer and read by
    lv_wal_reader over the oracle's scan (lvgpu.wal.encode and Scan.host take
    their CRCs from a device, which the host tests do not have)."""
    name = "host"

    def frame(self, payload, rec_off, rec_len, dest_length):
        log = bytearray()
        w = W.Writer(log, dest_length)
        for o, n in zip(rec_off, rec_len):
            w.add_record(payload[int(o): int(o) + int(n)])
        return bytes(log)

    def read_log(self, log):
        rep = W.ReportCollector()
        rd = LW.Reader(log, LW.Scan.from_arrays(*W.scan_log(log)), rep, True, 0)
        records = []
        while True:
            r = rd.read_record()
            if r is None:
                return records, rep.dropped_bytes
            records.append(r)

    def write(self, arena, ops, rec_op, first_sequence, dest_length):
        out, rec_off, rec_len, _, t = WB.encode_host(arena, ops, rec_op, first_sequence, want_ops=False)
        assert t["status"] == 0, t
        return self.frame(out, rec_off, rec_len, dest_length), t["last_sequence"]

    def recover(self, log):
        records, dropped = self.read_log(log)
        payload, rows, last, bad = b"".join(records), [], 0, 0
        at = 0
        for rec in records:
            st, ops, seq, _ = WB.iterate(rec)
            bad += st != WB.OK
            if ops:
                last = max(last, seq + len(ops) - 1)
            rows += [(tag, at + ko, at + vo, kl, vl) for tag, ko, kl, vo, vl in ops]
            at += len(rec)
        ops = np.array(rows, dtype=WB.OP_DTYPE) if rows else np.zeros(0, dtype=WB.OP_DTYPE)
        order, tot = MT.build_host(payload, ops)
        assert tot["status"] == 0, tot
        return HostTable(payload, ops, order, tot, last_sequence=last, dropped=dropped, bad_records=bad)

    def flush(self, mem, number, edit, dest_length):
        image, handles, t, _ = T.build_bloom_host(mem.payload, mem.ops, mem.order, mem.totals, BITS_PER_KEY, **OPT)
        assert t["status"] == 0, t
        tab, _ = T.open_host(image, handles=False)
        bounds = np.zeros(2 * (len(mem.payload) + 16), dtype=np.uint8)
        vf, used = V.file_host(np.frombuffer(image, dtype=np.uint8), 0, len(image), tab, number, 0, bounds, 0)
        assert vf["status"] == 0 and tab["status"] == 0, (vf, tab)
        e, f, d = edit_rows(edit, None, [(0, number, tab["file_bytes"], vf["smallest_off"], vf["smallest_len"],
                                          vf["largest_off"], vf["largest_len"])], [])
        src = bounds[:used].tobytes()
        rec, off, ln, t = VE.encode_host(src, e, f, [0, 1], d, [0, 0], np.zeros(0, dtype=VE.POINTER_DTYPE), [0, 0])
        assert t["status"] == 0, t
        return image, self.frame(rec, off, ln, dest_length)

    def manifest(self, log):
        records, dropped = self.read_log(log)
        out, last_has = [], [0] * 5
        for r, rec in enumerate(records):
            st, e, f, d, _, _ = VE.decode_host(rec)
            e["status"] = st
            out += decoded_edits(rec, e, f, d, [0, len(f)], [0, len(d)])
            for b in range(5):
                if st == VE.OK and int(e[0]["has"]) >> b & 1:
                    last_has[b] = r + 1
        return out, last_has, dropped

    def open_version(self, images, files):
        """files: [(level, number, off, size)] in the version's order."""
        img = np.frombuffer(images, dtype=np.uint8) if images else np.zeros(0, dtype=np.uint8)
        bounds = np.zeros(max(1, sum(2 * 256 for _ in files)), dtype=np.uint8)
        rows, tabs, blooms, meta, ok, used = [], [], [], [], [], 0
        for level, number, off, size in files:
            image = images[off: off + size]
            tab, handles = T.open_host(image)
            bl = T.bloom_open_host(image, tab)
            vf, used = V.file_host(img, off, size, tab, number, level, bounds, used)
            rows.append(tuple(vf[n] for n in V.FILE_DTYPE.names))
            tabs.append(tab)
            blooms.append(bl)
            meta.append((tab["file_bytes"], bytes(bounds[vf["smallest_off"]: vf["smallest_off"] + vf["smallest_len"]]),
                         bytes(bounds[vf["largest_off"]: vf["largest_off"] + vf["largest_len"]])))
            ok.append(tab["status"] == 0 and vf["status"] == 0 and bl["present"] == 1 and blocks_ok(image, handles))
        hv = V.HostVersion(img, np.array(rows, dtype=V.FILE_DTYPE), V.tables_array(tabs).reshape(-1, 8),
                           V.blooms_array(blooms).reshape(-1, 8), bounds[: max(used, 1)], bounds_bytes=used)
        st = hv.open()
        return SimpleNamespace(host=hv, status=st["status"], state=st, meta=meta, blocks_ok=ok, files=files,
                               images=images)

    def get(self, mem, ver, queries):
        out = []
        fn = V._bind().lv_version_get_host
        r = np.zeros(1, dtype=V.GET_DTYPE)
        hv = None if ver is None or ver.host.n == 0 else ver.host
        if hv is not None:  # the pointers once, a lookup is then one C call
            head = (V._ptr(hv.images), hv.images_bytes, V._ptr(hv.files), V._ptr(hv.tables), V._ptr(hv.blooms), hv.n,
                    V._ptr(hv.bounds), hv.bounds_bytes, hv.version.ctypes.data)
            rp, row = r.ctypes.data, r[0]
        for key, seq in queries:
            if mem is not None:
                m = mem.get(key, seq)
                if m.status != MT.GET_ABSENT:
                    out.append((STATUS.get(m.status, m.status),
                                mem.payload[m.val_off: m.val_off + m.val_len] if m.status == MT.GET_FOUND else None, "mem"))
                    continue
            if hv is None:
                out.append((ABSENT, None, None))
                continue
            assert fn(*head, key, len(key), seq, rp) == 0
            st = int(row["status"])
            if st == T.GET_ABSENT:
                out.append((ABSENT, None, None))
                continue
            off, ln = int(row["val_off"]), int(row["val_len"])
            out.append((STATUS.get(st, st), ver.images[off: off + ln] if st == T.GET_FOUND else None,
                        (int(row["level"]), ver.files[int(row["file"])][1]) if st in (1, 2) else None))
        return out

    def merged(self, mem, images, files):
        """The merged view: the memtable's ops, then every table scanned behind
        them (d_prev), sorted by one memtable build.  files: [(off, size)]."""
        parts = []
        for off, size in files:
            image = images[off: off + size]
            tab, _ = T.open_host(image, handles=False)
            parts.append((image, tab) + scan_size(image, tab))
        n0, b0 = (len(mem.ops), len(mem.payload)) if mem is not None else (0, 0)
        ocap, acap = n0 + sum(p[2] for p in parts), b0 + sum(p[3] for p in parts)
        if not ocap:
            return None
        if not parts:
            return mem
        arena = np.frombuffer(mem.payload, dtype=np.uint8) if b0 else None
        ops = mem.ops if n0 else None
        prev = dict.fromkeys(T.SCAN_TOTALS, 0)
        prev["entries"], prev["arena_bytes"] = n0, b0
        prev = prev if mem is not None else None
        for image, tab, _, _ in parts:
            prev, ops, arena, _ = T.scan_host(image, tab, prev, arena=arena, ops=ops, arena_cap=acap, op_cap=ocap)
            assert prev["status"] == 0, prev
        assert prev["entries"] == ocap and prev["arena_bytes"] == acap
        payload = arena.tobytes()
        order, tot = MT.build_host(payload, ops)
        assert tot["status"] == 0, tot
        return HostTable(payload, ops, order, tot)

    def ranges(self, view, rows, qkeys, limit, max_scan):
        if view is None:
            return [([], dict(status=MT.RANGE_DONE, next_pos=0, seen=0, count=0)) for _ in rows]
        return [view.range(qkeys, row, limit, max_scan) for row in rows]

    def compact(self, images, inputs, snapshot, ranges, level, first_number, images_off, edit, deleted, dest_length):
        view = self.merged(None, images, inputs)
        f = CP.filter_host(view.payload, view.ops, view.order, view.totals, snapshot, ranges, CP.BASE_LEVEL)
        assert f.totals["status"] == 0, f.totals
        out = CP.output_host(view.payload, view.ops, f.order(), f.mt_totals, MAX_FILE_BYTES, bits_per_key=BITS_PER_KEY,
                             first_number=first_number, level=level, images_off=images_off, **OPT)
        t = out.totals
        assert t["status"] == 0, t
        n = t["files"]
        assert (out.arena[t["arena_bytes"]:] == 0xA5).all()
        rows = [(level, int(v["number"]), int(out.tables[k][0]), int(v["smallest_off"]), int(v["smallest_len"]),
                 int(v["largest_off"]), int(v["largest_len"])) for k, v in enumerate(out.version_files[:n])]
        e, fr, d = edit_rows(edit, None, rows, deleted)
        rec, off, ln, et = VE.encode_host(out.bounds[: out.bound_used].tobytes(), e, fr, [0, n], d, [0, len(deleted)],
                                          np.zeros(0, dtype=VE.POINTER_DTYPE), [0, 0])
        assert et["status"] == 0, et
        bounds = out.bounds.tobytes()
        files = [(int(x["file_off"]), int(x["file_bytes"]), bounds[r[3]: r[3] + r[4]], bounds[r[5]: r[5] + r[6]])
                 for x, r in zip(out.files[:n], rows)]
        return out.arena[: t["arena_bytes"]].tobytes(), files, f.totals, self.frame(rec, off, ln, dest_length)


class HostTable:
    """A sorted memtable quadruple in host memory with buffers that stay put,
    so that a lookup is one C call."""

    def __init__(self, payload, ops, order, totals, **kw):
        self.payload, self.ops, self.order, self.totals = payload, np.ascontiguousarray(ops), np.ascontiguousarray(order), totals
        self.__dict__.update(kw)
        self._buf = ctypes.create_string_buffer(payload, max(len(payload), 1))
        self._tot = MT.Totals(totals["entries"], totals["user_keys"], totals["status"])
        self._res = MT.GetResult()
        self._L = MT._bind()
        self._head = (self._buf, len(payload), self.ops.ctypes.data if self.ops.size else None,
                      self.order.ctypes.data if self.order.size else None, ctypes.byref(self._tot))

    def get(self, key, seq):
        assert self._L.lv_memtable_get_host(*self._head, key, len(key), seq, ctypes.byref(self._res)) == 0
        return self._res

    def range(self, qkeys, row, limit, max_scan):
        hits = np.zeros(limit, dtype=np.uint32)
        res = np.zeros(1, dtype=MT.RANGE_RESULT_DTYPE)
        q = np.ascontiguousarray(np.asarray(row, dtype=MT.RANGE_QUERY_DTYPE).reshape(1))
        rc = self._L.lv_memtable_range_host(*self._head, self.ops.size, qkeys, len(qkeys), q.ctypes.data, limit, max_scan,
                                            hits.ctypes.data, res.ctypes.data)
        assert rc == 0
        r = {k: int(res[0][k]) for k in ("next_pos", "count", "status", "seen")}
        return hits[: r["count"]].tolist(), r

    def entry(self, i):
        o = self.ops[i]
        ko, kl, vo, vl = int(o["key_off"]), int(o["key_len"]), int(o["val_off"]), int(o["val_len"])
        return self.payload[ko: ko + kl], int(o["tag"]), self.payload[vo: vo + vl]

    def entries(self):
        """(user key, sequence, type) in memtable order."""
        return [(k, t >> 8, t & 0xFF) for k, t, _ in (self.entry(int(i)) for i in self.order)]


# ---- the device backend ----------------------------------------------------------
class DeviceBackend:
    """The *_device entry points.  Every output is canary-filled with a guard
    behind it and every workspace dirty; the tails are checked where the used
    length is known."""
    name = "device"

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev

    # -- plumbing --
    def up(self, b, align=16):
        """bytes on the device, 16-byte aligned (allocations are), 16 spare bytes behind."""
        torch = self.torch
        t = torch.full(((len(b) + 31) & ~15,), 0x3C, dtype=torch.uint8, device=self.dev)
        if len(b):
            t[: len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
        return t[: len(b)]

    def i64(self, a):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64)
        return self.torch.from_numpy(a.copy()).to(self.dev)

    def rows(self, a):
        return self.torch.from_numpy(np.frombuffer(a.tobytes() + bytes(16), dtype=np.uint8).copy()).to(self.dev)

    def dirty(self, nbytes):
        return self.torch.full((max(int(nbytes), 16),), 0x5A, dtype=self.torch.uint8, device=self.dev)

    def canary_behind(self, t, used):
        assert bool((t.view(self.torch.uint8)[used:] == CANARY).all()), "a write behind the used part of an output"

    def frame(self, payload_t, rec_off, rec_len, dest_length):
        return LW.encode_device(payload_t, rec_off, rec_len, dest_length).cpu().numpy().tobytes()

    def log_chain(self, log_t):
        """lv_wal_scan_device -> lv_wal_decode_device of a whole log in HBM."""
        nbytes = log_t.numel()
        cap = nbytes // LW.HEADER_SIZE + 2
        hdr, crc, info, count = LW.scan_device(log_t, cap, workspace=self.dirty(LW.scan_workspace_bytes(nbytes, cap)))
        dec = LW.decode_device(log_t, hdr, crc, info, count, workspace=self.dirty(LW.decode_workspace_bytes(cap)),
                               fill=CANARY)
        return dec, cap

    # -- the operations --
    def write(self, arena, ops, rec_op, first_sequence, dest_length):
        n_rec, n_ops = len(rec_op) - 1, len(ops)
        e = WB.encode_device(self.up(arena), self.rows(ops), self.i64(rec_op), self.i64([n_rec]),
                             first_sequence=first_sequence, rec_cap=n_rec, op_cap=n_ops,
                             out_cap=12 * n_rec + 11 * n_ops + len(arena),
                             workspace=self.dirty(WB.encode_workspace_bytes(n_rec, n_ops)), fill=CANARY, guard=GUARD,
                             want_ops=False)
        t = e.sync_totals()
        self.canary_behind(e.out_t, t["out_bytes"])
        return self.frame(e.out_t, e.rec_off(), e.rec_len(), dest_length), t["last_sequence"]

    def recover_chain(self, log_t):
        """scan -> WAL decode -> WriteBatch decode -> memtable build, the
        counts and statuses handed on in device memory; no copy from or to the
        host, so the chain can be captured."""
        dec, cap = self.log_chain(log_t)
        op_cap = log_t.numel() // 2 + 1
        ops = WB.decode_device(dec.payload, dec.rec_off, dec.rec_len, dec.totals[0:1], dec.totals[4:5], rec_cap=cap,
                               op_cap=op_cap, workspace=self.dirty(WB.decode_workspace_bytes(cap)), fill=CANARY,
                               guard=GUARD)
        table = MT.build_device(dec.payload, ops.ops_t, ops.totals[1:2], ops.totals[6:7], op_cap=op_cap,
                                workspace=self.dirty(MT.build_workspace_bytes(op_cap)), fill=CANARY, guard=GUARD)
        return dec, ops, table

    def recover(self, log):
        dec, ops, table = self.recover_chain(self.up(log))
        wt, ot, mt = dec.sync_totals(), ops.sync_totals(), table.sync_totals()
        self.canary_behind(ops.ops_t, 32 * ot["ops"])
        self.canary_behind(table.order_t, 4 * mt["entries"])
        payload = dec.payload[: wt["payload_bytes"]].cpu().numpy().tobytes()
        return DeviceTable(self, table, payload, ops.ops(), table.order(), mt, last_sequence=ot["last_sequence"],
                           dropped=wt["dropped_bytes"], bad_records=ot["bad_records"], wb_totals=ops.totals,
                           wal_totals=dec.totals)

    def flush_chain(self, table, number, edit_t, dest=None):
        """Bloom build -> open -> bloom open -> version file -> NewFile row -> edit encode."""
        torch = self.torch
        cap = table.op_cap
        built = T.build_bloom_device(table, BITS_PER_KEY, workspace=self.dirty(T.build_bloom_workspace_bytes(cap, cap)),
                                     fill=CANARY, guard=GUARD, **OPT)
        opened = T.open_device(built.file_t[: built.file_cap], built.totals[2:3], built.totals[7:8], handles=False)
        bloom = T.bloom_open_device(opened)
        bounds_t = torch.full((2 * table.payload.numel() + 64,), CANARY, dtype=torch.uint8, device=self.dev)
        used = torch.zeros(1, dtype=torch.int64, device=self.dev)
        vf = torch.full((64,), CANARY, dtype=torch.uint8, device=self.dev)
        V.file_device(built.file_t, built.file_cap, 0, built.file_cap, opened.table, number, 0, bounds_t,
                      bounds_t.numel(), used, vf)
        files_t, rec_file, status = VE.files_device(vf, opened.table.view(torch.uint8), self.i64([1]), files_cap=1)
        none16 = torch.zeros(16, dtype=torch.uint8, device=self.dev)
        zeros2 = torch.zeros(2, dtype=torch.int64, device=self.dev)
        enc = VE.encode_device(bounds_t, edit_t, files_t, rec_file, none16, zeros2, none16, zeros2, self.i64([1]), status,
                               rec_cap=1, caps=(1, 0, 0), fill=CANARY, guard=GUARD)
        return built, opened, bloom, enc

    def flush(self, mem, number, edit, dest_length):
        e, _, _ = edit_rows(edit, None, [], [])
        built, opened, bloom, enc = self.flush_chain(mem.table, number, self.rows(e))
        t = built.sync_totals()
        self.canary_behind(built.file_t, t["file_bytes"])
        assert T.bloom_dict(bloom)["present"] == 1
        et = enc.sync_totals()
        self.canary_behind(enc.out_t, et["out_bytes"])
        return built.file(), self.frame(enc.out_t, enc.rec_off(), enc.rec_len(), dest_length)

    def manifest(self, log):
        dec, cap = self.log_chain(self.up(log))
        d = VE.decode_device(dec.payload, dec.rec_off, dec.rec_len, dec.totals[0:1], dec.totals[4:5], rec_cap=cap,
                             workspace=self.dirty(VE.decode_workspace_bytes(cap)), fill=CANARY, guard=GUARD)
        wt, t = dec.sync_totals(), d.sync_totals()
        bf, bd, _ = d.bounds()
        pay = dec.payload.cpu().numpy().tobytes()
        return (decoded_edits(pay, d.edits(), d.files(), d.deleted(), bf, bd), [t["last_has%d" % b] for b in range(5)],
                wt["dropped_bytes"])

    def open_version(self, images, files):
        torch = self.torch
        n = len(files)
        img_t = self.up(images)
        files_t = torch.full((64 * n + GUARD,), CANARY, dtype=torch.uint8, device=self.dev)
        tables_t = torch.zeros(8 * max(n, 1), dtype=torch.int64, device=self.dev)
        blooms_t = torch.zeros(8 * max(n, 1), dtype=torch.int64, device=self.dev)
        bounds_t = torch.full((512 * max(n, 1),), CANARY, dtype=torch.uint8, device=self.dev)
        used = torch.zeros(1, dtype=torch.int64, device=self.dev)
        opens = []
        for i, (level, number, off, size) in enumerate(files):
            op = T.open_device(img_t[off: off + size], self.i64([size]), block_cap=size // 13 + 1,
                               table=tables_t[8 * i: 8 * i + 8], fill=CANARY, guard=GUARD)
            T.bloom_open_device(op, bloom=blooms_t[8 * i: 8 * i + 8])
            V.file_device(img_t, len(images), off, size, tables_t[8 * i: 8 * i + 8], number, level, bounds_t,
                          bounds_t.numel(), used, files_t[64 * i: 64 * i + 64])
            opens.append(op)
        opened = V.open_device(img_t if n else torch.zeros(16, dtype=torch.uint8, device=self.dev), files_t, tables_t, n,
                               bounds_t, blooms_t=blooms_t, images_bytes=len(images), bounds_bytes=bounds_t.numel())
        st = opened.sync(check=False)
        self.canary_behind(files_t, 64 * n)
        self.canary_behind(bounds_t, int(used.cpu()[0]))
        rows = opened.files() if n else []
        bounds = bounds_t.cpu().numpy().tobytes()
        tabs = tables_t.cpu().numpy().view(np.uint64).reshape(-1, 8)
        blooms = blooms_t.cpu().numpy().view(np.uint64).reshape(-1, 8)
        meta, ok = [], []
        for i, (vf, op) in enumerate(zip(rows, opens)):
            so, sl, lo, ll = (int(vf[k]) for k in ("smallest_off", "smallest_len", "largest_off", "largest_len"))
            meta.append((int(tabs[i][0]), bounds[so: so + sl], bounds[lo: lo + ll]))
            good = int(tabs[i][7]) == 0 and int(vf["status"]) == 0 and int(blooms[i][5]) == 1
            if good:
                st_b = T.verify_blocks(op.file_t, op.handles_view()).cpu().tolist()
                good = st_b == [T.BLOCK_OK] * (int(tabs[i][5]) + 2)
            ok.append(good)
        return SimpleNamespace(opened=opened, status=st["status"], state=st, meta=meta, blocks_ok=ok, files=files,
                               images=images)

    def get(self, mem, ver, queries):
        torch = self.torch
        qk, off, ln, sq = pack_queries(queries)
        nq = len(queries)
        dq = (self.up(qk), torch.from_numpy(off).to(self.dev), torch.from_numpy(ln).to(self.dev),
              torch.from_numpy(sq).to(self.dev))
        m = v = None
        if mem is not None:
            res = MT.get_device(mem.table, *dq, nq=nq, fill=CANARY, guard=GUARD)
            m = MT.results(res, nq)
            self.canary_behind(res, 24 * nq)
        if ver is not None and ver.opened.n_files:
            g = V.get_device(ver.opened, *dq, nq=nq, fill=CANARY, guard=GUARD)
            v = g.sync()
            self.canary_behind(g.res, 48 * nq)
        out = []
        for i in range(nq):
            if m is not None and int(m[i]["status"]) != MT.GET_ABSENT:
                st, o, n = int(m[i]["status"]), int(m[i]["val_off"]), int(m[i]["val_len"])
                out.append((STATUS.get(st, st), mem.payload[o: o + n] if st == MT.GET_FOUND else None, "mem"))
            elif v is None:
                out.append((ABSENT, None, None))
            else:
                st, o, n = int(v[i]["status"]), int(v[i]["val_off"]), int(v[i]["val_len"])
                out.append((STATUS.get(st, st), ver.images[o: o + n] if st == T.GET_FOUND else None,
                            (int(v[i]["level"]), ver.files[int(v[i]["file"])][1]) if st in (1, 2) else None))
        return out

    def merged_chain(self, mem, images, files):
        torch = self.torch
        parts = []
        for off, size in files:
            image = images[off: off + size]
            tab, _ = T.open_host(image, handles=False)  # a capacity: the host's sizing pass
            parts.append(scan_size(image, tab))
        n0, b0 = (len(mem.ops), len(mem.payload)) if mem is not None else (0, 0)
        ocap, acap = n0 + sum(p[0] for p in parts), b0 + sum(p[1] for p in parts)
        if not ocap:
            return None
        if not parts:
            return mem.table
        img_t = self.up(images)
        arena_t = torch.full(((acap + 15 + GUARD) & ~15,), CANARY, dtype=torch.uint8, device=self.dev)
        ops_t = torch.full((32 * ocap + GUARD,), CANARY, dtype=torch.uint8, device=self.dev)
        prev = None
        if mem is not None:  # the memtable's ops lead; the scans append behind them by d_prev
            arena_t[:b0].copy_(mem.table.payload[:b0])
            ops_t[: 32 * n0].copy_(mem.table.ops_t[: 32 * n0])
            totals = torch.zeros(8, dtype=torch.int64, device=self.dev)
            totals[0:1].copy_(mem.wb_totals[1:2])   # the op count, device to device
            totals[1:2].copy_(mem.wal_totals[1:2])  # the payload's bytes
            prev = SimpleNamespace(arena_t=arena_t, arena_cap=acap, ops_t=ops_t, op_cap=ocap, totals=totals)
        for off, size in files:
            op = T.open_device(img_t[off: off + size], self.i64([size]), handles=False)
            bcap = size // 13 + 1
            prev = T.scan_device(op, prev, arena_cap=acap, op_cap=ocap, block_cap=bcap, arena_t=arena_t, ops_t=ops_t,
                                 workspace=self.dirty(T.scan_workspace_bytes(ocap, bcap)))
        table = MT.build_device(arena_t[:acap], ops_t, prev.totals[0:1], prev.totals[7:8], op_cap=ocap,
                                workspace=self.dirty(MT.build_workspace_bytes(ocap)), fill=CANARY, guard=GUARD)
        table.scan_totals = prev
        return table

    def _host_view(self, table):
        """A device quadruple with its host copy."""
        if isinstance(table, DeviceTable):
            return table
        mt = table.sync_totals()
        if getattr(table, "scan_totals", None) is not None:
            st = table.scan_totals.sync()
            assert st["entries"] == table.op_cap and st["arena_bytes"] == table.payload.numel(), st
            self.canary_behind(table.ops_t, 32 * st["entries"])
        self.canary_behind(table.order_t, 4 * mt["entries"])
        payload = table.payload.cpu().numpy().tobytes()
        ops = table.ops_t[: 32 * table.op_cap].cpu().numpy().view(WB.OP_DTYPE).copy()
        return DeviceTable(self, table, payload, ops, table.order(), mt)

    def merged(self, mem, images, files):
        table = self.merged_chain(mem, images, files)
        if table is None:
            return None
        return mem if table is getattr(mem, "table", None) else self._host_view(table)

    def ranges(self, view, rows, qkeys, limit, max_scan):
        if view is None:
            return [([], dict(status=MT.RANGE_DONE, next_pos=0, seen=0, count=0)) for _ in rows]
        r = MT.range_device(view.table, rows, qkeys, limit, max_scan, fill=CANARY, guard=GUARD)
        hits, res = r.hit_lists()
        self.canary_behind(r.results_t, 40 * len(rows))
        return [(h, {k: int(x[k]) for k in MT.RANGE_RESULT_DTYPE.names}) for h, x in zip(hits, res)]

    def compact(self, images, inputs, snapshot, ranges, level, first_number, images_off, edit, deleted, dest_length):
        torch = self.torch
        table = self.merged_chain(None, images, inputs)
        cap = table.op_cap
        f = CP.filter_device(table, snapshot, ranges, CP.BASE_LEVEL, workspace=self.dirty(CP.filter_workspace_bytes(cap)),
                             fill=CANARY, guard=GUARD)
        out = CP.output_device(f, MAX_FILE_BYTES, bits_per_key=BITS_PER_KEY, first_number=first_number, level=level,
                               images_off=images_off, block_cap=cap, files_cap=cap,
                               workspace=self.dirty(CP.output_workspace_bytes(cap, cap, cap)), fill=CANARY, guard=GUARD,
                               **OPT)
        files_t, rec_file, status = VE.files_device(out.version_files_t, out.tables_t, out.totals[1:2], files_cap=cap)
        e, _, d = edit_rows(edit, None, [], deleted)
        none16 = torch.zeros(16, dtype=torch.uint8, device=self.dev)
        enc = VE.encode_device(out.bounds_t, self.rows(e), files_t, rec_file, self.rows(d), self.i64([0, len(deleted)]),
                               none16, torch.zeros(2, dtype=torch.int64, device=self.dev), self.i64([1]), status,
                               rec_cap=1, caps=(cap, len(deleted), 0),
                               workspace=self.dirty(VE.encode_workspace_bytes(1, cap, len(deleted), 0)), fill=CANARY,
                               guard=GUARD)
        ct, t = f.sync(), out.sync()
        self.canary_behind(f.order_t, 4 * ct["kept"])
        self.canary_behind(out.arena_t, t["arena_bytes"])
        self.canary_behind(out.files_t, 64 * t["files"])
        et = enc.sync_totals()
        assert et["files"] == t["files"] and int(status.cpu()[0]) == 0
        bounds = out.bounds_t.cpu().numpy().tobytes()
        vfs = out.version_files_t[: 64 * t["files"]].cpu().numpy().view(V.FILE_DTYPE)
        files = [(int(x["file_off"]), int(x["file_bytes"]),
                  bounds[int(v["smallest_off"]): int(v["smallest_off"]) + int(v["smallest_len"])],
                  bounds[int(v["largest_off"]): int(v["largest_off"]) + int(v["largest_len"])])
                 for x, v in zip(out.files(), vfs)]
        arena = out.arena_t[: t["arena_bytes"]].cpu().numpy().tobytes()
        return arena, files, ct, self.frame(enc.out_t, enc.rec_off(), enc.rec_len(), dest_length)


class DeviceTable(HostTable):
    """A device quadruple (`table`) with its host copy: the entries and the
    values are read from the copy, the lookups run on the device."""

    def __init__(self, backend, table, payload, ops, order, totals, **kw):
        self.payload, self.ops, self.order, self.totals, self.table = payload, ops, order, totals, table
        self.__dict__.update(kw)


# ---- the store -------------------------------------------------------------------
class Store:
    def __init__(self, backend, fault=None):
        assert fault is None or fault in FAULTS
        self.b, self.fault = backend, fault
        self.wlog, self.manifest, self.images = bytearray(), bytearray(), bytearray()
        self.groups_in_log = 0
        self.directory = {}          # number -> (offset, size) in the image arena
        self.files = {}              # the applied version: number -> (level, size, smallest, largest)
        self.next_file, self.log_number, self.last_sequence = 1, 0, 0
        self.manifest_last_sequence = 0
        self.mem = self.ver = self.view = None
        self.floor = 0
        self.dropped_deletions = 0
        self.wal_dropped = 0
        self.compactions = []        # (level, snapshot, inputs, outputs, lv_compact_totals)
        self.unsorted_seen = False
        self.open_version()

    # -- writes --
    def write(self, group):
        arena, rows, rec_op = bytearray(b"\xee" * 3), [], [0]
        for batch in group:
            for typ, key, value in batch:
                ko = len(arena)
                arena += key
                vo = len(arena)
                if typ == VALUE:
                    arena += value
                rows.append((typ, ko, vo, len(key), len(value) if typ == VALUE else 0))
                if len(rows) % 3 == 0:
                    arena += b"\xee"
            rec_op.append(len(rows))
        ops = np.array(rows, dtype=WB.OP_DTYPE)
        first, dest = self.last_sequence + 1, len(self.wlog)
        if self.fault == "first_sequence_off_by_one" and self.groups_in_log == 1:
            first += 1
        if self.fault == "dest_length_zero" and self.groups_in_log >= 1:
            dest = 0
        appended, last = self.b.write(bytes(arena), ops, rec_op, first, dest)
        self.wlog += appended
        self.last_sequence = last
        self.groups_in_log += 1

    def recover(self):
        """The live memtable is what recovery of the whole log gives."""
        self.mem = self.b.recover(bytes(self.wlog)) if self.wlog else None
        self.wal_dropped = self.mem.dropped + self.mem.bad_records if self.mem is not None else 0
        self.view = None
        return self.recovered_last_sequence()

    def recovered_last_sequence(self):
        return max(self.manifest_last_sequence, self.mem.last_sequence if self.mem is not None else 0)

    # -- the version --
    def ordered(self, files=None):
        """The version's order: level ascending; level 0 newest first; levels
        >= 1 by smallest internal key (user key ascending, tag descending)."""
        files = self.files if files is None else files
        l0 = sorted((n for n, f in files.items() if f[0] == 0), reverse=self.fault != "level0_oldest_first")
        rest = sorted((n for n, f in files.items() if f[0] > 0),
                      key=lambda n: (files[n][0], user(files[n][2]), -tag_of(files[n][2])))
        return l0 + rest

    def open_version(self):
        order = self.ver_numbers = self.ordered()
        rows = [(self.files[n][0], n) + self.directory[n] for n in order]
        self.ver = self.b.open_version(bytes(self.images), rows)
        n0 = sum(1 for n in order if self.files[n][0] == 0)
        if self.fault == "level0_oldest_first" and n0 > 1:
            # oldest first is refused; numbered as if it were newest first it opens, and a stale value wins
            self.unsorted_seen |= self.ver.status == V.OPEN_UNSORTED
            top = max(order)
            rows = [(r[0], top - i if i < n0 else r[1]) + r[2:] for i, r in enumerate(rows)]
            self.ver = self.b.open_version(bytes(self.images), rows)
        self.view = None
        return self.ver

    def add_image(self, image):
        off = (len(self.images) + 15) & ~15
        self.images += bytes(off - len(self.images)) + image
        return off

    def edit(self):
        return dict(log_number=self.log_number, next_file_number=self.next_file, last_sequence=self.last_sequence)

    def flush(self):
        assert self.mem is not None, "nothing to flush"
        number = self.next_file
        self.next_file += 1
        self.log_number = self.next_file  # the log that follows the flushed one
        self.next_file += 1
        image, appended = self.b.flush(self.mem, number, self.edit(), len(self.manifest))
        self.manifest += appended
        self.manifest_last_sequence = self.last_sequence
        self.directory[number] = (self.add_image(image), len(image))
        self.files[number] = (0, len(image), None, None)
        self.wlog, self.groups_in_log, self.mem = bytearray(), 0, None
        self.open_version()
        self.take_bounds()
        return number

    def take_bounds(self):
        """The bounds and sizes the open read from the images, for files new to the version."""
        for number, (size, smallest, largest) in zip(self.ver_numbers, self.ver.meta):
            if self.files[number][2] is None:
                self.files[number] = (self.files[number][0], size, smallest, largest)

    def level_files(self, level):
        return [n for n in self.ordered() if self.files[n][0] == level]

    def overlapping(self, level, lo, hi):
        return [n for n in self.level_files(level)
                if not (user(self.files[n][3]) < lo or user(self.files[n][2]) > hi)]

    def span(self, numbers):
        return min(user(self.files[n][2]) for n in numbers), max(user(self.files[n][3]) for n in numbers)

    def compact(self, level, snapshot, pick=None):
        """Level 0: every level-0 file; else one file of `level` (the middle
        one, or `pick`) and the files behind it that begin with the user key it
        ends with (a cut may fall inside a user key: upstream's
        AddBoundaryInputs); plus the files of level + 1 whose bounds overlap."""
        if level == 0:
            picked = self.level_files(0)
        else:
            mine = self.level_files(level)
            at = len(mine) // 2 if pick is None else mine.index(pick)
            picked = [mine[at]]
            while at + 1 < len(mine) and user(self.files[mine[at + 1]][2]) == user(self.files[mine[at]][3]):
                at += 1  # the older versions of the input's last user key must not stay above it
                picked.append(mine[at])
        assert picked, "nothing to compact"
        below = self.overlapping(level + 1, *self.span(picked))
        inputs = picked + below
        ranges = [(user(f[2]), user(f[3])) for f in self.files.values() if f[0] > level + 1]
        if self.fault == "ranges_omitted":
            ranges = []
        removed = [] if self.fault == "compaction_inputs_not_removed" else inputs
        deleted = sorted((self.files[n][0], n) for n in removed)  # a BTreeSet's order (version_edit.rs)
        first, images_off = self.next_file, (len(self.images) + 15) & ~15
        arena, outs, totals, appended = self.b.compact(bytes(self.images), [self.directory[n] for n in inputs], snapshot,
                                                       ranges, level + 1, first, images_off, self.edit(), deleted,
                                                       len(self.manifest))
        # the edit's next_file_number is the one before the outputs took theirs: a recovery takes the maximum
        assert self.add_image(arena) == images_off or not arena
        self.manifest += appended
        for n in removed:
            del self.files[n]
        numbers = []
        for k, (off, size, smallest, largest) in enumerate(outs):
            self.directory[first + k] = (images_off + off, size)
            self.files[first + k] = (level + 1, size, smallest, largest)
            numbers.append(first + k)
        self.next_file = first + len(outs)
        self.floor = max(self.floor, snapshot)
        self.dropped_deletions += totals["dropped_deletions"]
        self.compactions.append(dict(level=level, snapshot=snapshot, picked=picked, below=below, outputs=numbers,
                                     totals=totals, ranges=len(ranges),
                                     untouched=len(self.level_files(level + 1)) - len(numbers)))
        self.open_version()
        return numbers

    def reopen(self):
        """Forget the version; rebuild it from the MANIFEST and the directory."""
        before = dict(self.files)
        self.files, self.ver, self.mem = {}, None, None
        edits, last_has, dropped = self.b.manifest(bytes(self.manifest))
        assert dropped == 0 and all(e["status"] == VE.OK for e in edits), (dropped, edits)
        top = 0
        for e in edits:
            for level, number in e["deleted"]:
                del self.files[number]
            for level, number, size, smallest, largest in e["files"]:
                self.files[number] = (level, size, smallest, largest)
                top = max(top, number)
        # last_has[b]: 1 + the record that carries the bit last (log number, next file, last sequence: bits 1, 3, 4)
        self.log_number = edits[last_has[1] - 1]["log_number"]
        self.next_file = max(edits[last_has[3] - 1]["next_file_number"], top + 1, self.log_number + 1)
        self.manifest_last_sequence = edits[last_has[4] - 1]["last_sequence"]
        self.open_version()
        self.last_sequence = self.recover()
        return before

    # -- reads --
    def get(self, queries):
        return self.b.get(self.mem, self.ver, queries)

    def merged(self):
        if self.view is None:
            self.view = self.b.merged(self.mem, bytes(self.images), [self.directory[n] for n in self.ordered()])
        return self.view

    def range(self, queries, limit, max_scan=1 << 40):
        """queries: (lo, hi | None, seq).  One shot: the visible (key, value) pairs."""
        view = self.merged()
        qkeys, rows = MT.pack_range_queries(queries)
        out = []
        for hits, res in self.b.ranges(view, rows, qkeys, limit, max_scan):
            if res["status"] not in (MT.RANGE_DONE, MT.RANGE_MORE_LIMIT):
                out.append([("status", res["status"])])
                continue
            out.append([(k, v) for k, _, v in (view.entry(h) for h in hits)])
        return out

    def range_resumed(self, queries, limit, max_scan):
        """The same walk as a resume chain of (limit, max_scan) steps."""
        view = self.merged()
        out = [[] for _ in queries]
        live = list(range(len(queries)))
        qs = list(queries)
        while live:
            qkeys, rows = MT.pack_range_queries([qs[i] for i in live])
            nxt = []
            for i, (hits, res) in zip(live, self.b.ranges(view, rows, qkeys, limit, max_scan)):
                out[i] += [(k, v) for k, _, v in (view.entry(h) for h in hits)]
                if res["status"] in (MT.RANGE_MORE_LIMIT, MT.RANGE_MORE_SCAN):
                    qs[i] = ("resume", res["next_pos"], res["seen"], queries[i][1], queries[i][2])
                    nxt.append(i)
            live = nxt
        return out

    def file_entries(self, number):
        """(user key, sequence, type) of one live file, in its order."""
        view = self.b.merged(None, bytes(self.images), [self.directory[number]])
        return view.entries()

    def state(self):
        """What two backends must agree on byte for byte."""
        mem = None if self.mem is None else (self.mem.payload, self.mem.ops.tobytes(), self.mem.order.tobytes())
        view = None if self.view is None else (self.view.payload, self.view.ops.tobytes(), self.view.order.tobytes())
        return dict(wlog=bytes(self.wlog), manifest=bytes(self.manifest), images=bytes(self.images), mem=mem, view=view,
                    files=dict(self.files), directory=dict(self.directory), version=self.ver.state,
                    counters=(self.next_file, self.log_number, self.last_sequence, self.floor))


# ---- the check -------------------------------------------------------------------
def check(store, model, floor=None, *, ranges=True):
    """Every answer of the store against the model's.  Returns a report:
    asked / found / deleted / absent count the (key, snapshot) pairs by the
    model's answer, sources the places FOUND answers came from, mismatches
    what differs (empty for a sound store)."""
    floor = store.floor if floor is None else floor
    if store.fault == "floor_ignored":
        floor = 0
    rep = SimpleNamespace(asked=0, found=0, deleted=0, absent=0, sources=set(), mismatches=[], ranges=0)
    bad = rep.mismatches
    if store.ver.status != 0:
        bad.append(("version open status", store.ver.state))
    if not all(store.ver.blocks_ok):
        bad.append(("blocks", store.ver.blocks_ok))
    if store.recovered_last_sequence() != model.last_sequence:
        bad.append(("last_sequence", store.recovered_last_sequence(), model.last_sequence))
    if store.wal_dropped:
        bad.append(("the log lost records", store.wal_dropped))
    last = model.last_sequence
    pairs = set()
    for key, versions in model.history.items():
        snaps = {0, floor, last, MAX}
        for seq, _, _ in versions:
            snaps |= {seq - 1, seq, seq + 1}
        snaps = [s for s in snaps if floor <= s <= MAX]
        for k in {key, key + b"\0", key[:-1]}:
            pairs |= {(k, s) for s in snaps}
    pairs = sorted(pairs)
    newest_l0 = max((n for n, f in store.files.items() if f[0] == 0), default=None)
    for (key, snap), (st, value, src) in zip(pairs, store.get(pairs)):
        want, wv = model.get(key, snap)
        rep.asked += 1
        rep.found += want == FOUND
        rep.deleted += want == DELETED
        rep.absent += want == ABSENT
        if st == want and value == wv:
            if st == FOUND:
                rep.sources.add("mem" if src == "mem" else "level0 older" if src[0] == 0 and src[1] != newest_l0
                                else "level0 newest" if src[0] == 0 else "deeper")
            continue
        e = model.newest(key, snap)
        if want == DELETED and st == ABSENT and store.dropped_deletions and e[0] <= store.floor:
            continue  # LV_COMPACT_BASE_LEVEL dropped the tombstone: nothing lies beneath it
        bad.append(("get", key, snap, (st, value), (want, wv), src))
    if ranges:
        keys = sorted(model.history)
        cuts = [(b"", None)]
        if keys:
            step = max(1, len(keys) // 15)
            for i in range(0, len(keys), step):
                cuts.append((keys[i], keys[min(i + 7, len(keys) - 1)]))
                cuts.append((keys[i] + b"\0", None if i % (2 * step) else keys[-1]))
        snaps = sorted({floor, max(floor, (floor + last) // 2), MAX})
        for snap in snaps:
            qs = [(lo, hi, snap) for lo, hi in cuts]
            for limit in (1, 7, 1000):
                for q, got in zip(qs, store.range(qs, limit)):
                    rep.ranges += 1
                    want = model.range(q[0], q[1], snap, limit)
                    if got != want:
                        bad.append(("range", q, limit, got[:3], want[:3]))
        qs = [(lo, hi, snaps[-1]) for lo, hi in cuts]
        for q, got, want in zip(qs, store.range_resumed(qs, 3, 5), store.range(qs, 1000)):
            if got != want:
                bad.append(("resume chain", q, got[:3], want[:3]))
    return rep


def add(total, rep):
    for k in ("asked", "found", "deleted", "absent", "ranges"):
        setattr(total, k, getattr(total, k) + getattr(rep, k))
    total.sources |= rep.sources
    total.mismatches += rep.mismatches
    return total


def new_report():
    return SimpleNamespace(asked=0, found=0, deleted=0, absent=0, sources=set(), mismatches=[], ranges=0)


def life(store, model, seed, *, n_ops=1500, generations=4, per_group=True, checkpoint=None, stop_at_mismatch=False,
         checking=True):
    """The life of a store: four generations of three groups each.  Generations
    1 and 2 end with a flush, 2 also with compact(0, S = mid); 3 with a flush
    and a compaction of one level-1 file into level 2; 4 with a flush, compact(0,
    S = last_sequence) and a reopen.  checkpoint(store, model, name) runs after
    every group (per_group False: every generation's last group), flush,
    compaction and the reopen, in front of the check (checking False: in its
    place); the summed report is returned."""
    rng = np.random.default_rng(seed)
    keys = universe()
    total = new_report()

    def point(name):
        if checkpoint is not None:
            checkpoint(store, model, name)
        if checking:
            add(total, check(store, model))
        return bool(total.mismatches) and stop_at_mismatch

    for g in range(generations):
        groups = generation(rng, keys, g, n_ops, big=g == 0)
        for i, group in enumerate(groups):
            store.write(group)
            for batch in group:
                model.apply(batch)
            store.recover()
            if (per_group or i == len(groups) - 1) and point(f"g{g} group {i}"):
                return total
        mid = (store.floor + model.last_sequence) // 2
        store.flush()
        if point(f"g{g} flush"):
            return total
        if g == 1:
            store.compact(0, mid)
        elif g == 2:
            store.compact(1, mid)
        elif g == 3:
            store.compact(0, model.last_sequence)
        if g >= 1 and point(f"g{g} compaction"):
            return total
        if g == 3:
            before = store.reopen()
            if before != store.files:
                total.mismatches.append(("the reopened version", sorted(before), sorted(store.files)))
            if point(f"g{g} reopen"):
                return total
    return total


def tombstone_story(store, model, check_=check):
    """A tombstone above a deeper value, written out: k is put and compacted
    down to level 2; k and j are deleted and flushed, and level 0 is compacted
    into level 1 above the deletions; then level 1 goes into level 2.  Returns
    the facts the tests assert, and the summed report."""
    total = new_report()
    facts = {}

    def write(*ops):
        store.write([list(ops)])
        model.apply(list(ops))
        store.recover()

    def get(key):
        return store.get([(key, MAX)])[0][0]

    write((VALUE, b"a", b"a1"), (VALUE, b"k", b"old"), (VALUE, b"z", b"z1"))
    store.flush()
    store.compact(0, model.last_sequence)
    store.compact(1, model.last_sequence)
    facts["k lies on level 2"] = [store.files[n][0] for n in store.files] == [2]
    add(total, check_(store, model))
    write((VALUE, b"~j", b"j1"))
    write((DELETION, b"k", b""), (DELETION, b"~j", b""), (VALUE, b"m", b"m1"))
    k_seq = model.history[b"k"][-1][0]
    store.flush()
    add(total, check_(store, model))
    out = store.compact(0, model.last_sequence)
    entries = [e for n in out for e in store.file_entries(n)]
    facts["k's tombstone is kept"] = (b"k", k_seq, DELETION) in entries
    facts["j's tombstone is dropped"] = not any(e[0] == b"~j" for e in entries)
    facts["dropped_deletions"] = store.compactions[-1]["totals"]["dropped_deletions"]
    facts["get k"], facts["get j"] = get(b"k"), get(b"~j")
    add(total, check_(store, model))
    out = store.compact(1, model.last_sequence, pick=out[0])
    entries = [e for n in store.files for e in store.file_entries(n)]
    facts["levels after the last compaction"] = sorted({f[0] for f in store.files.values()})
    facts["no entry of k is left"] = not any(e[0] == b"k" for e in entries)
    facts["get k at the end"] = get(b"k")
    add(total, check_(store, model))
    return facts, total
