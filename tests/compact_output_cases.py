"""lv_compact_output_* (include/lvgpu/compact.h): the serial model, the cases
and the comparisons the CPU and GPU tests share.

The model runs upstream's loop with the table builders of sst_build_cases /
sst_bloom_cases: a fresh builder per file, closed after the add that brought
len(tb.file), upstream's FileSize(), to max_file_bytes.  The records come from
model_bloom_open and version_cases.model_file over the model's own images.
"""
import functools
import json
import os
import struct

import numpy as np

import memtable_cases as M
import sst_bloom_cases as B
import sst_build_cases as S
import version_cases as V
from memtable_cases import make_table, tag
from write_batch_cases import CANARY, GUARD, tail_is_canary

TOTALS = ("entries", "files", "data_blocks", "arena_bytes", "handle_pairs", "bound_bytes", "reserved", "status")
FILE_FIELDS = ("first_entry", "entries", "file_off", "file_bytes", "data_blocks", "first_handle", "filter_keys",
               "reserved")
TABLE_FIELDS = ("file_bytes", "metaindex_offset", "metaindex_size", "index_offset", "index_size", "data_blocks",
                "reserved", "status")
NO_TABLE, HANDLE_OVER, ARENA_OVER, BLOCK_LARGE, FILES_OVER, BOUND_OVER = 1, 2, 4, 8, 16, 32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compact_output_example.json")
TILE = 1024  # csrc/lvk/knobs.h: LVK_SB_TILE
NO_LIMIT = 1 << 63


def align16(x):
    return (x + 15) & ~15


class Want:
    """The model's output: totals, files / tables / blooms / vfiles (lists of
    dicts), images and offs (arena offsets), handles (flat (offset, size)
    list), bounds (bytes behind the cursor's start) and used (the cursor)."""

    def flushed(self, k):
        """FileSize() when file k was closed: its data blocks' raw + 5."""
        f = self.files[k]
        hs = self.handles[f["first_handle"]: f["first_handle"] + f["data_blocks"]]
        return sum(sz + 5 for _, sz in hs)


def model_output(payload, ops, max_file_bytes, bpk=None, block_size=S.BLOCK_SIZE, restart_interval=S.RESTART_INTERVAL,
                 *, order=None, first_number=1, level=1, images_off=0, bound_used=0, version_files=True):
    ents = S.entries_of(payload, ops, order)
    w = Want()
    w.extra = 3 if bpk else 2
    w.files, w.tables, w.blooms, w.vfiles, w.images, w.offs, w.handles = [], [], [], [], [], [], []
    tb, first = None, 0

    def close(i_end):
        nonlocal tb
        fin = tb.finish()
        meta, index = fin[-2], fin[-1]
        off = align16(w.offs[-1] + len(w.images[-1])) if w.offs else 0
        w.files.append(dict(first_entry=first, entries=i_end - first, file_off=off, file_bytes=len(tb.file),
                            data_blocks=len(tb.handles), first_handle=len(w.handles),
                            filter_keys=i_end - first if bpk else 0, reserved=0))
        w.tables.append(dict(file_bytes=len(tb.file), metaindex_offset=meta[0], metaindex_size=meta[1],
                             index_offset=index[0], index_size=index[1], data_blocks=len(tb.handles), reserved=0,
                             status=0))
        w.handles += tb.handles + list(fin)
        w.images.append(bytes(tb.file))
        w.offs.append(off)
        tb = None

    for i, (k, v) in enumerate(ents):
        if tb is None:
            tb = B.BloomTableBuilder(bpk, block_size, restart_interval) if bpk else S.TableBuilder(block_size,
                                                                                                   restart_interval)
            first = i
        tb.add(k, v)
        if len(tb.file) >= max_file_bytes:
            close(i + 1)
    w.last_by_cut = tb is None  # the last file was closed by the threshold, not by the end of the input
    if tb is not None:
        close(len(ents))
    arena_bytes = w.offs[-1] + len(w.images[-1]) if w.offs else 0
    arena = bytearray(arena_bytes)
    for off, img in zip(w.offs, w.images):
        arena[off:off + len(img)] = img
    bounds, used = bytearray(bound_used + sum(len(ents[f["first_entry"]][0]) + len(ents[f["first_entry"] + f["entries"] - 1][0])
                                              for f in w.files)), bound_used
    for k, f in enumerate(w.files):
        w.blooms.append(B.model_bloom_open(w.images[k], w.tables[k]))
        if version_files:
            vf, used = V.model_file(bytes(arena), len(arena), f["file_off"], f["file_bytes"], w.tables[k],
                                    first_number + k, level, bounds, len(bounds), used)
            vf["file_off"] += images_off
            w.vfiles.append(vf)
    w.bounds, w.used = bytes(bounds[bound_used:]), used
    w.totals = dict(entries=len(ents), files=len(w.files), data_blocks=sum(f["data_blocks"] for f in w.files),
                    arena_bytes=arena_bytes, handle_pairs=len(w.handles), bound_bytes=used - bound_used, reserved=0,
                    status=0)
    return w


# ---- cases ----
def example_items():
    return [(b"k", tag(1), b"v"), (b"m", tag(2), b"w")]


def block_bytes(items, block_size, restart_interval, bpk=None):
    """The model's flushed bytes after each data block of the one-file build."""
    payload, ops = make_table(items)
    hs = S.model_build(payload, ops, block_size, restart_interval)[1][:-2]
    out, at = [], 0
    for _, sz in hs:
        at += sz + 5
        out.append(at)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (items, block_size, restart_interval, bpk, max_file_bytes)."""
    c = {}
    sc = S.cases()
    c["example"] = (example_items(), 1, 16, None, 1)
    c["empty"] = ([], 64, 4, None, 100)
    for bpk in (None, 10):
        items, bs, ri = sc["random_small_blocks"]
        c[f"one_file_{bpk}"] = (items, bs, ri, bpk, NO_LIMIT)
        c[f"small_files_{bpk}"] = (items, bs, ri, bpk, 200)
        c[f"tile_files_{bpk}"] = (S.tile_items(300), 32, 2, bpk, 100)
    for name in sc:
        if name.startswith("sep_") or name.startswith("succ_"):
            c[f"each_{name}"] = (sc[name][0], 1, 16, None, 1)
            c[f"each_bloom_{name}"] = (sc[name][0], 1, 16, 10, 1)
    # the cut threshold: B = the flushed bytes at the second block of file 0
    items = S.seq_items(60, klen=5, vlen=7)
    bb = block_bytes(items, 48, 3)
    for d in (-1, 0, 1):
        c[f"cut_{d:+d}"] = (items, 48, 3, None, bb[1] + d)
    c["end_on_flush"] = end_on_flush_case()
    c["end_open"] = (S.seq_items(61, klen=5, vlen=7), 48, 3, 10, 150)
    c["corner_keys"] = (M.corner_items(), 256, 3, 10, 700)
    c["tags"] = (M.tag_items(), 48, 2, None, 90)
    c["duplicates"] = (sc["duplicates"][0], 1, 16, 10, 1)
    c["filter_windows"] = (B.window_items(1500), 32, 16, 10, 5000)
    # the default options: 4 KiB blocks of many entries, a few blocks to a file
    c["default_options"] = (sc["random_default"][0], S.BLOCK_SIZE, S.RESTART_INTERVAL, 10, 9000)
    return c


def end_on_flush_case():
    """The last entry flushes a block that also reaches the threshold: at
    least two files and no empty last one.  Searched for, so that the shape is
    the model's own and not a guess."""
    for n in range(40, 80):
        items = S.seq_items(n, klen=5, vlen=7)
        payload, ops = make_table(items)
        bb = block_bytes(items, 48, 3)
        for j in range(len(bb) - 1):
            mf = bb[-1] - bb[j]
            w = model_output(payload, ops, mf, 10, 48, 3)
            if w.last_by_cut and len(w.files) >= 2:
                return items, 48, 3, 10, mf
    raise AssertionError("no input ends on a flushed block at the threshold")


BIG = (1 << 32) - 1  # a value of this many bytes makes its block LARGE (raw >= 2^32 - 1)


def block_large_case(vlen=BIG):
    """(payload, ops, order, mt totals, claimed payload_bytes, block_size,
    restart_interval, max_file_bytes): entries a, b, c, where b's value is an
    extent of `vlen` bytes claimed inside a payload of 2^32 + 16 bytes that
    nobody allocates.  A status is decided from sizes alone, and nothing is
    emitted, so no byte of the value is read.  Under the default options a and
    b share block 0, whose size closes file 0 behind b; c is file 1: with a
    small value instead the three entries are one block of one file."""
    payload, ops = make_table([(b"a", tag(2), b"x"), (b"b", tag(1), b"y"), (b"c", tag(3), b"z")])
    ops = ops.copy()
    ops[1]["val_off"], ops[1]["val_len"] = 16, vlen
    payload = payload + bytes(16 - len(payload))
    return (payload, ops, np.arange(3, dtype=np.uint32), dict(entries=3, user_keys=3, status=0), (1 << 32) + 16,
            S.BLOCK_SIZE, S.RESTART_INTERVAL, 1000)


def golden_dict():
    items, bs, ri, bpk, mf = cases()["example"]
    payload, ops = make_table(items)
    w = model_output(payload, ops, mf, bpk, bs, ri)
    arena = bytearray([0xEE]) * w.totals["arena_bytes"]  # the gap is never written: any bytes
    for off, img in zip(w.offs, w.images):
        arena[off:off + len(img)] = img
    return dict(entries=[[k.decode(), t >> 8, v.decode()] for k, t, v in items], block_size=bs, restart_interval=ri,
                max_file_bytes=mf, totals=w.totals, files=w.files, handles=[list(h) for h in w.handles],
                images=[img.hex() for img in w.images], bounds=w.bounds.hex(), tables=w.tables)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- the host twin ----
def host_output(payload, ops, max_file_bytes, bpk=None, block_size=S.BLOCK_SIZE, restart_interval=S.RESTART_INTERVAL,
                *, order=None, **kw):
    import lvgpu.compact as C
    if order is None:
        order, mt = M.model_totals(payload, ops)
    else:
        mt = dict(entries=len(order), user_keys=0, status=0)
    return C.output_host(payload, ops, order, mt, max_file_bytes, bits_per_key=bpk, block_size=block_size,
                         restart_interval=restart_interval, **kw)


def _rows(arr, fields, n):
    return [{f: int(arr[k][f]) for f in fields} for k in range(n)]


def compare_host(out, w, tag_="", fill=0xA5):
    """Every output of a host call with status 0 against the model: the
    arena with its gaps and guard, the handles, the four record arrays, the
    bound keys and the cursor."""
    from lvgpu.version import FILE_DTYPE
    assert out.totals == w.totals, (tag_, out.totals, w.totals)
    nf = len(w.files)
    want = np.full(out.arena.size, fill, dtype=np.uint8)
    for off, img in zip(w.offs, w.images):
        want[off:off + len(img)] = np.frombuffer(img, dtype=np.uint8)
    diff = np.nonzero(out.arena != want)[0]
    assert diff.size == 0, (tag_, "arena differs at", int(diff[0]))
    hs = [(int(out.handles[2 * i]), int(out.handles[2 * i + 1])) for i in range(len(w.handles))]
    assert hs == w.handles, (tag_, hs[:6], w.handles[:6])
    word = fill * 0x0101010101010101
    assert (out.handles[2 * len(w.handles):] == word).all(), (tag_, "handles written beyond their count")
    assert _rows(out.files, FILE_FIELDS, nf) == w.files, (tag_, "files")
    assert [dict(zip(TABLE_FIELDS, map(int, out.tables[k]))) for k in range(nf)] == w.tables, (tag_, "tables")
    assert [dict(zip(B.BLOOM_FIELDS, map(int, out.blooms[k]))) for k in range(nf)] == w.blooms, (tag_, "blooms")
    assert _rows(out.version_files, FILE_DTYPE.names, nf) == w.vfiles, (tag_, "version files")
    assert (out.tables[nf:] == word).all() and (out.blooms[nf:] == word).all(), (tag_, "records beyond files")
    assert out.files[nf:].tobytes() == bytes([fill]) * (64 * (len(out.files) - nf)), (tag_, "files beyond files")
    assert out.version_files[nf:].tobytes() == bytes([fill]) * (64 * (len(out.version_files) - nf)), tag_
    start = out.bound_used - w.totals["bound_bytes"]
    assert out.bound_used == w.used, (tag_, out.bound_used, w.used)
    assert out.bounds[start:out.bound_used].tobytes() == w.bounds, (tag_, "bound keys")
    assert (out.bounds[:start] == fill).all() and (out.bounds[out.bound_used:] == fill).all(), (tag_, "bounds guard")


def untouched_host(out, bound_used=0, fill=0xA5):
    """A host call with a status wrote nothing but the totals."""
    word = fill * 0x0101010101010101
    assert (out.arena == fill).all() and (out.handles == word).all() and (out.bounds == fill).all()
    assert (out.tables == word).all() and (out.blooms == word).all()
    assert set(out.files.tobytes()) <= {fill} and set(out.version_files.tobytes()) <= {fill}
    assert out.bound_used == bound_used


# ---- one device call ----
def run_device(torch, dev, payload, ops, max_file_bytes, bpk=None, block_size=S.BLOCK_SIZE,
               restart_interval=S.RESTART_INTERVAL, *, want=None, shift=0, op_cap=None, arena_cap=None, block_cap=None,
               files_cap=None, bound_cap=None, bound_used=5, mt_status=0, stream=None, **kw):
    """lv_memtable_build_device, then lv_compact_output_device over its outputs
    with every output canary-filled and guarded and a dirty workspace; the
    capacities default to exactly the model's counts.  Returns (Output, model)."""
    import lvgpu.compact as C
    table, buf = M.run_build(torch, dev, payload, ops, shift=shift, op_cap=op_cap, stream=stream)
    if mt_status:
        table.totals[2] = mt_status
    w = want or model_output(payload, ops, max_file_bytes, bpk, block_size, restart_interval, bound_used=bound_used,
                             first_number=kw.get("first_number", 1), level=kw.get("level", 1),
                             images_off=kw.get("images_off", 0))
    ac = w.totals["arena_bytes"] if arena_cap is None else arena_cap
    bc = w.totals["data_blocks"] if block_cap is None else block_cap
    fc = w.totals["files"] if files_cap is None else files_cap
    kc = w.used if bound_cap is None else bound_cap
    ws = torch.full((max(C.output_workspace_bytes(table.op_cap, bc, fc), 16),), 0x5A, dtype=torch.uint8, device=dev)
    used_t = M.dev_i64(torch, dev, [bound_used])
    out = C.output_device(table, max_file_bytes, bits_per_key=bpk, block_size=block_size,
                          restart_interval=restart_interval, arena_cap=ac, block_cap=bc, files_cap=fc, bound_cap=kc,
                          used_t=used_t, workspace=ws, stream=stream, fill=CANARY, guard=GUARD, **kw)
    out._buf = buf
    return out, w


def _cpu(t):
    import torch
    return t.view(torch.uint8).cpu().numpy()


def compare_device(out, w, tag_="", verify=True):
    """Every output of a device call with status 0 against the model, canaries
    included; every file's handles through lv_sst_verify_blocks_device."""
    import lvgpu.table as T
    from lvgpu.version import FILE_DTYPE
    t = out.sync()
    assert t == w.totals, (tag_, t, w.totals)
    nf = len(w.files)
    arena = _cpu(out.arena_t)
    want = np.full(arena.size, CANARY, dtype=np.uint8)
    for off, img in zip(w.offs, w.images):
        want[off:off + len(img)] = np.frombuffer(img, dtype=np.uint8)
    diff = np.nonzero(arena != want)[0]
    assert diff.size == 0, (tag_, "arena differs at", int(diff[0]), arena[diff[0]:diff[0] + 8], want[diff[0]:diff[0] + 8])
    hs = _cpu(out.handles_t).view(np.uint64)
    got = [(int(hs[2 * i]), int(hs[2 * i + 1])) for i in range(len(w.handles))]
    assert got == w.handles, (tag_, got[:6], w.handles[:6])
    assert tail_is_canary(out.handles_t, 16 * len(w.handles)), (tag_, "d_handles written beyond its count")
    assert _rows(_cpu(out.files_t)[:64 * nf].view(np.dtype([(n, "<u8") for n in FILE_FIELDS])), FILE_FIELDS, nf) == w.files, tag_
    tb = _cpu(out.tables_t)[:64 * nf].view(np.uint64).reshape(nf, 8)
    assert [dict(zip(TABLE_FIELDS, map(int, r))) for r in tb] == w.tables, (tag_, "tables")
    bl = _cpu(out.blooms_t)[:64 * nf].view(np.uint64).reshape(nf, 8)
    assert [dict(zip(B.BLOOM_FIELDS, map(int, r))) for r in bl] == w.blooms, (tag_, "blooms")
    vf = _cpu(out.version_files_t)[:64 * nf].view(FILE_DTYPE)
    assert _rows(vf, FILE_DTYPE.names, nf) == w.vfiles, (tag_, "version files", _rows(vf, FILE_DTYPE.names, nf)[:2], w.vfiles[:2])
    for t_ in (out.files_t, out.tables_t, out.blooms_t, out.version_files_t):
        assert tail_is_canary(t_, 64 * nf), (tag_, "records written beyond files")
    used = int(out.used_t.cpu().numpy().view(np.uint64)[0])
    assert used == w.used, (tag_, used, w.used)
    start = w.used - w.totals["bound_bytes"]
    bk = _cpu(out.bounds_t)
    assert bk[start:used].tobytes() == w.bounds, (tag_, "bound keys")
    assert (bk[:start] == CANARY).all() and (bk[used:] == CANARY).all(), (tag_, "bound keys' guards")
    if verify:
        for k in range(nf):
            f = w.files[k]
            file_t = out.arena_t[f["file_off"]: f["file_off"] + f["file_bytes"]]
            st = T.verify_blocks(file_t, out.file_handles_view(k))
            assert int(st.abs().sum()) == 0, (tag_, "verify", k)


def untouched_device(out, bound_used=5):
    for t_ in (out.arena_t, out.handles_t, out.files_t, out.tables_t, out.blooms_t, out.version_files_t, out.bounds_t):
        assert tail_is_canary(t_, 0)
    assert int(out.used_t.cpu().numpy().view(np.uint64)[0]) == bound_used


def check_device(torch, dev, items, block_size, restart_interval, bpk, max_file_bytes, *, tag_="", gaps=None, **kw):
    payload, ops = make_table(items, gaps)
    out, w = run_device(torch, dev, payload, ops, max_file_bytes, bpk, block_size, restart_interval, **kw)
    compare_device(out, w, tag_)
    return out, w


# ---- the dump tools/compact_output_hostcheck.cc replays ----
def dump_cases():
    """(name, payload, ops, order, mt status, payload_bytes, bs, ri, bpk, mf,
    caps or None): the CPU / GPU inputs, caps one short of the counts for
    every status, and hostile ops whose extents lie outside the payload."""
    out = []
    for name, (items, bs, ri, bpk, mf) in cases().items():
        payload, ops = make_table(items)
        order = M.model_order(payload, ops)
        out.append((name, payload, ops, order, 0, len(payload), bs, ri, bpk or 0, mf, None))
    items, bs, ri, bpk, mf = cases()["small_files_10"]
    payload, ops = make_table(items)
    order = M.model_order(payload, ops)
    w = model_output(payload, ops, mf, bpk, bs, ri)
    t = w.totals
    full = (t["arena_bytes"], t["data_blocks"], t["files"], t["bound_bytes"])
    for i, nm in enumerate(("arena", "blocks", "files", "bounds")):
        caps = list(full)
        caps[i] -= 1
        out.append((f"short_{nm}", payload, ops, order, 0, len(payload), bs, ri, bpk, mf, tuple(caps)))
    out.append(("upstream", payload, ops, order, 1, len(payload), bs, ri, bpk, mf, full))
    for field, val in (("key_off", len(payload) + 1), ("val_len", 0xFFFFFFFF), ("key_len", 0xFFFFFFFF),
                       ("val_off", (1 << 64) - 1)):
        bad = ops.copy()
        bad[len(bad) // 2][field] = val
        out.append((f"hostile_{field}", payload, bad, order, 0, len(payload), bs, ri, bpk, mf, full))
    bad_order = list(order)
    bad_order[3] = len(ops)
    out.append(("hostile_order", payload, ops, bad_order, 0, len(payload), bs, ri, bpk, mf, full))
    # BLOCK_LARGE, with ARENA_OVER (an arena that held the files would be 4 GiB): the claimed payload is not dumped
    payload, ops, order, _, claimed, bs, ri, mf = block_large_case()
    for bpk in (0, 10):
        out.append((f"block_large_{bpk}", payload, ops, list(order), 0, claimed, bs, ri, bpk, mf, (64, 2, 2, 36)))
    return out


def dump(path):
    """Little-endian: u32 cases; per case u32 name length, name, u64 payload
    bytes, payload, u32 ops, the ops, u32 entries, the order (u32 each), u64
    mt status, u64 payload_bytes (the dumped bytes, or a larger claim whose
    rest is never read: block_large), u32 block_size, restart_interval, bpk, u64
    max_file_bytes, u32 has_caps, 4 u64 caps (arena, blocks, files, bounds)."""
    cs = dump_cases()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cs)))
        for name, payload, ops, order, st, pb, bs, ri, bpk, mf, caps in cs:
            nm = name.encode()
            f.write(struct.pack("<I", len(nm)) + nm)
            f.write(struct.pack("<Q", len(payload)) + bytes(payload))
            f.write(struct.pack("<I", len(ops)) + np.ascontiguousarray(ops).tobytes())
            f.write(struct.pack("<I", len(order)) + np.asarray(order, dtype="<u4").tobytes())
            f.write(struct.pack("<QQIIIQ", st, pb, bs, ri, bpk, mf))
            f.write(struct.pack("<I4Q", 1 if caps else 0, *(caps or (0, 0, 0, 0))))
    return len(cs)
