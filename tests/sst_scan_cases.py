"""The SSTable scan in Python, written straight from the "Scan" section of
include/lvgpu/table.h over bytes, with keys as Python bytes objects (the
product never holds one): model_scan is the model every output of
lv_sst_scan_host and lv_sst_scan_device is compared with.  On well-formed
images sst_build_cases.read_table, written for the build, is the independent
cross-check.  Also the hand-made damaged blocks, the dump the host check
program (tools/sst_scan_host_check.cc) replays, and the device helpers shared
by test_gpu_sst_scan_device.py and test_gpu_sst_scan_stress.py."""
import numpy as np

import memtable_cases as M
import sst_build_cases as S
import sst_get_cases as G
from memtable_cases import make_table, tag
from sst_get_cases import decode, handle_at, in_range, le32, restarts
from write_batch_cases import CANARY, GUARD, M64, tail_is_canary

UPSTREAM, NO_TABLE, CORRUPT, BLOCK_OVER, OP_OVER, ARENA_OVER = 1, 2, 4, 8, 16, 32
MT_UNORDERED, MT_UPSTREAM = 8, 1
TOTALS = ("entries", "arena_bytes", "table_entries", "table_bytes", "data_blocks", "runs", "reserved", "status")


class Corrupt(Exception):
    pass


def block_runs(raw):
    """[[(internal key, value)] per restart run] of a data block; Corrupt."""
    r = restarts(raw)
    if r is None:
        raise Corrupt
    n, arr = r
    if n == 0:
        return []
    if n == 1 and arr == 0:
        return [[]]  # the empty BlockBuilder: one run, no entry
    rs = [le32(raw, arr + 4 * i) for i in range(n)]
    if rs[0] != 0 or any(a >= b for a, b in zip(rs, rs[1:])) or rs[-1] >= arr:
        raise Corrupt
    runs = []
    for i, at in enumerate(rs):
        end = rs[i + 1] if i + 1 < n else arr
        key, ents = b"", []
        while at < end:
            e = decode(raw, at, end)
            if e is None or e[0] > len(key) or e[0] + e[1] < 8:  # (the first: shared > 0 = len(b""))
                raise Corrupt
            shared, ns, vl, key_at = e
            key = key[:shared] + raw[key_at:key_at + ns]
            ents.append((key, raw[key_at + ns:key_at + ns + vl]))
            at = key_at + ns + vl
        runs.append(ents)
    return runs


def table_runs(file, table):
    """(data_blocks, [[(key, value)] per run]) of the image by the table dict;
    Corrupt (data_blocks is known once the index header is sound: the
    exception carries it, or None)."""
    fb, io, isz = table["file_bytes"], table["index_offset"], table["index_size"]
    if not in_range(io, isz, fb) or file[io + isz] != 0:
        raise Corrupt(None)
    idx = file[io:io + isz]
    r = restarts(idx)
    if r is None or r[0] != table["data_blocks"]:
        raise Corrupt(None)
    n, arr = r
    runs = []
    try:
        for i in range(n):
            e = decode(idx, le32(idx, arr + 4 * i), arr)
            if e is None or e[0] != 0 or e[1] < 8:
                raise Corrupt
            hd = handle_at(idx, e[3] + e[1], e[3] + e[1] + e[2])
            if hd is None or not in_range(hd[0], hd[1], fb) or file[hd[0] + hd[1]] != 0:
                raise Corrupt
            runs += block_runs(file[hd[0]:hd[0] + hd[1]])
    except Corrupt:
        raise Corrupt(n)
    return n, runs


def compare(a, a_tag, b, b_tag):
    """lv_internal_key_compare."""
    if a != b:
        return -1 if a < b else 1
    return -1 if a_tag > b_tag else (1 if a_tag < b_tag else 0)


def model_scan(image, table, prev=None, *, arena_cap=None, op_cap=None, block_cap=None, file_cap=None, order=False):
    """(totals dict, ops [(tag, key_off, val_off, key_len, val_len)], this
    table's arena bytes (they belong at prev's arena_bytes), mt_totals dict or
    None).  A cap of None is large enough.  On any status no op and no byte."""
    base_e, base_b = (prev["entries"], prev["arena_bytes"]) if prev else (0, 0)
    t = dict.fromkeys(TOTALS, 0)
    t["entries"], t["arena_bytes"] = base_e, base_b
    mt = dict(entries=0, user_keys=0, status=MT_UPSTREAM) if order else None
    st = 0
    if prev and prev["status"]:
        st |= UPSTREAM
    fb = table["file_bytes"]
    if table["status"] or (file_cap is not None and fb > file_cap):
        st |= NO_TABLE
    ents = []
    if not st and fb:
        try:
            if block_cap is not None:  # the header alone decides BLOCK_OVER
                io, isz = table["index_offset"], table["index_size"]
                if in_range(io, isz, fb) and image[io + isz] == 0:
                    r = restarts(image[io:io + isz])
                    if r is not None and r[0] == table["data_blocks"] and r[0] > block_cap:
                        t["data_blocks"] = r[0]
                        st = BLOCK_OVER
            if not st:
                t["data_blocks"], runs = table_runs(image, table)
                t["runs"] = len(runs)
                ents = [e for run in runs for e in run]
        except Corrupt as c:
            st = CORRUPT
            t["data_blocks"] = c.args[0] or 0
    ops, arena = [], bytearray()
    if not st:
        at = base_b
        for key, value in ents:
            ops.append((int.from_bytes(key[-8:], "little"), at, at + len(key) - 8, len(key) - 8, len(value)))
            arena += key[:-8] + value
            at += len(key) - 8 + len(value)
        t["table_entries"], t["table_bytes"] = len(ents), len(arena)
        t["entries"], t["arena_bytes"] = base_e + len(ents), at
        if op_cap is not None and t["entries"] > op_cap:
            st |= OP_OVER
        if arena_cap is not None and t["arena_bytes"] > arena_cap:
            st |= ARENA_OVER
    t["status"] = st
    if st:
        return t, [], b"", mt
    if order:
        keys = [(k[:-8], int.from_bytes(k[-8:], "little")) for k, _ in ents]
        bad = any(compare(*a, *b) > 0 for a, b in zip(keys, keys[1:]))
        users = sum(1 for i, k in enumerate(keys) if i == 0 or k[0] != keys[i - 1][0])
        mt = dict(entries=len(ents), user_keys=0 if bad else users, status=MT_UNORDERED if bad else 0)
    return t, ops, bytes(arena), mt


def model_entries(ops, arena, base_b=0):
    """[(internal key, value)] of a model_scan result."""
    out = []
    for t, ko, vo, kl, vl in ops:
        out.append((arena[ko - base_b:ko - base_b + kl] + t.to_bytes(8, "little"), arena[vo - base_b:vo - base_b + vl]))
    return out


def ops_array(ops):
    return np.array(ops, dtype=M.op_dtype()) if ops else np.zeros(0, dtype=M.op_dtype())


def open_table(image):
    return G.model_open(image)[0]


# ---- hand-made tables ----
def one_block_table(raw, typ=0):
    """An image whose only data block is `raw`."""
    return G.assemble([raw], [S.ikey(b"zzzz", tag(1))], types=[typ])[0]


def block_rule_cases():
    """name -> (image, expected status): every block rule by a hand-made block
    (sst_get_cases' twelve keys at restart interval 4)."""
    hp, rb = G.hand_parts, G.raw_block
    good = rb(hp(), 4)
    c = {"good": (good, 0)}
    c["restart0_not_0"] = (rb(hp(), 4, restarts_=lambda rs, end: [1] + rs[1:]), CORRUPT)
    c["equal_restarts"] = (rb(hp(), 4, restarts_=lambda rs, end: [rs[0], rs[1], rs[1]]), CORRUPT)
    c["decreasing_restarts"] = (rb(hp(), 4, restarts_=lambda rs, end: [rs[0], rs[2], rs[1]]), CORRUPT)
    c["run_overruns_into_next"] = (rb(hp(), 4, restarts_=lambda rs, end: [rs[0], rs[1] - 1, rs[2]]), CORRUPT)
    c["run_stops_short"] = (rb(hp(), 4, restarts_=lambda rs, end: [rs[0], rs[1] + 1, rs[2]]), CORRUPT)
    c["last_restart_at_arr"] = (rb(hp(), 4, restarts_=lambda rs, end: [rs[0], rs[1], end]), CORRUPT)
    c["restart_beyond_arr"] = (rb(hp(), 4, restarts_=lambda rs, end: [rs[0], rs[1], end + 9]), CORRUPT)
    c["shared_on_restart"] = (rb(hp({4: dict(shared=1)}), 4), CORRUPT)
    c["shared_beyond_previous_key"] = (rb(hp({5: dict(shared=100)}), 4), CORRUPT)
    c["key_of_7_bytes"] = (rb(hp({8: dict(suffix=b"key08\x01\x00")}), 4), CORRUPT)
    c["scanned_key_of_7_bytes"] = (rb(hp({1: dict(shared=2, suffix=b"x" * 5)}), 4), CORRUPT)
    c["n_0"] = (rb(hp(), 4, count=0, restarts_=lambda rs, end: []), 0)
    c["empty_block"] = (S.BlockBuilder(16).finish(), 0)
    c["n_1_arr_0_restart_7"] = (S.fixed32(7) + S.fixed32(1), 0)  # no entries: the restart is not looked at
    c["n_2_arr_0"] = (S.fixed32(0) + S.fixed32(0) + S.fixed32(2), CORRUPT)
    c["n_too_large"] = (rb(hp(), 4, count=1 << 30), CORRUPT)
    c["size_3"] = (b"\x01\x00\x00", CORRUPT)
    c["trailing_2_bytes"] = (rb(hp() + [b"\x00\x00"], 4), CORRUPT)
    out = {k: (one_block_table(raw), st) for k, (raw, st) in c.items()}
    out["type_byte_1"] = (one_block_table(good, 1), CORRUPT)
    return out


def swapped_table():
    """A sound block but for two entries in the wrong order (MT_UNORDERED)."""
    keys = [S.ikey(b"k%02d" % i, tag(9)) for i in (0, 2, 1, 3)]
    return one_block_table(G.raw_block([G.enc(0, k, b"v") for k in keys], 1))


def twice_table():
    """An index whose two entries name the same block."""
    b = S.BlockBuilder(2)
    for i in range(5):
        b.add(S.ikey(b"k%d" % i, tag(7)), b"v%d" % i)
    raw = b.finish()
    image, hs = G.assemble([raw], [S.ikey(b"k4", tag(7))])
    index = G.index_block([(S.ikey(b"k4", tag(7)), S.handle_encoding(*hs[0])),
                           (S.ikey(b"k5", tag(7)), S.handle_encoding(*hs[0]))])
    return G.assemble([raw], None, index=index)[0]


FOREIGN_PATCHES = (lambda n, s: dict(file_bytes=n + 1), lambda n, s: dict(index_offset=n),
                   lambda n, s: dict(index_size=1 << 40), lambda n, s: dict(index_offset=(1 << 64) - 3),
                   lambda n, s: dict(index_offset=0, index_size=s["index_offset"]),
                   lambda n, s: dict(file_bytes=n - 48), lambda n, s: dict(data_blocks=s["data_blocks"] + 1),
                   lambda n, s: dict(data_blocks=0))


def foreign_tables(image):
    """Tables the open did not write for this image (test_gpu_sst_get_device's
    patches and two on data_blocks)."""
    sound = open_table(image)
    return [dict(sound, **p(len(image), sound)) for p in FOREIGN_PATCHES]


FLIP_SEED, FLIP_COUNT = 78, 200


def flip_cases(count=FLIP_COUNT):
    """[(image, its own table)] of random flips inside the data blocks of
    random_small_blocks; tables the open refuses are left out (NO_TABLE says
    nothing about the walk)."""
    image, data_end, _ = G.flip_source()
    rng = np.random.default_rng(FLIP_SEED)
    out = []
    for bad in G.flips(image, rng, count, 0, data_end):
        t = open_table(bad)
        if not t["status"]:
            out.append((bad, t))
    return out


def damaged_cases():
    """[(name, image, table dict)]: sst_get_cases' damaged images with the
    table their gets go by, the block rules, the two hand-made tables, the
    foreign tables and the flips."""
    out = [(name, image, use) for name, image, _, use, _ in G.damaged_cases(0)]
    out += [("rule/" + k, img, open_table(img)) for k, (img, _) in block_rule_cases().items()]
    out += [("swapped", swapped_table(), open_table(swapped_table())), ("twice", twice_table(), open_table(twice_table()))]
    base = G.base_image()[2]
    out += [(f"foreign/{i}", base, t) for i, t in enumerate(foreign_tables(base))]
    out += [(f"flip/{i}", img, t) for i, (img, t) in enumerate(flip_cases())]
    return out


def host_usable(image, table):
    """The host twin has no file_cap: it may be given only tables whose
    file_bytes the image holds."""
    return table["file_bytes"] <= len(image)


def dump(path):
    """The damaged cases with the model's expected outputs, for
    tools/sst_scan_host_check.cc to replay under a sanitizer (little-endian u64
    fields; see its replay())."""
    u64 = lambda v: int(v).to_bytes(8, "little")
    cases = [c for c in damaged_cases() if host_usable(c[1], c[2])]
    out = bytearray(u64(len(cases)))
    for _, image, table in cases:
        t, ops, arena, mt = model_scan(image, table, order=True)
        out += u64(len(image)) + image + b"".join(u64(table[f]) for f in G.TABLE_FIELDS)
        out += b"".join(u64(t[f]) for f in TOTALS) + b"".join(u64(mt[f]) for f in ("entries", "user_keys", "status"))
        out += u64(len(ops)) + ops_array(ops).tobytes() + u64(len(arena)) + arena
    with open(path, "wb") as f:
        f.write(out)
    return len(cases)


# ---- the device ----
def place(torch, dev, image, shift=0):
    return G.place(torch, dev, image, shift)


def open_on(torch, dev, image, shift=0, table=None, stream=None):
    """The image on the device between canaries and its open (with `table`, a
    table the open did not write, put in its place): (Opened, owner)."""
    owner, file_t = place(torch, dev, image, shift)
    op = G.run_open(torch, dev, file_t, len(image), block_cap=open_table(image)["data_blocks"], stream=stream)
    if table is not None:
        G.set_table(torch, op, table)
    return op, owner


def run_scan(torch, dev, opened, prev=None, *, arena_cap, op_cap, block_cap, arena_shift=0, order=False, stream=None):
    """lv_sst_scan_device with the arena (at arena_shift bytes past a 16-B
    boundary), ops and order canary-filled with guards, and a dirty workspace."""
    import lvgpu.table as T
    kw = {}
    if prev is None:
        buf = torch.full((arena_cap + 2 * GUARD + 32,), CANARY, dtype=torch.uint8, device=dev)
        base = (-buf.data_ptr()) % 16 + arena_shift + GUARD
        kw = dict(arena_t=buf[base:], arena_cap=arena_cap, op_cap=op_cap)
    ws = torch.full((max(T.scan_workspace_bytes(prev.op_cap if prev else op_cap, block_cap), 16),), 0x5A,
                    dtype=torch.uint8, device=dev)
    sc = T.scan_device(opened, prev, block_cap=block_cap, order=order, workspace=ws, stream=stream, fill=CANARY,
                       guard=GUARD, **kw)
    if prev is None:
        sc._buf, sc._base = buf, base
    else:
        sc._buf, sc._base = prev._buf, prev._base
    return sc


def check_scan(sc, want, *, prev_want=None, tag_=""):
    """A Scanned against model_scan's result (and, appended, against what the
    earlier scans left: prev_want = (ops, arena bytes) so far), with every
    canary: (ops so far, arena so far)."""
    import torch
    wt, wops, warena, wmt = want
    got = sc.sync(check=False)
    assert got == wt, (tag_, got, wt)
    pops, parena = prev_want if prev_want else ([], b"")
    ops, arena = (pops + wops, parena + warena) if not wt["status"] else (pops, parena)
    host = sc._buf.cpu().numpy()
    assert (host[:sc._base] == CANARY).all(), (tag_, "the arena's front guard")
    assert host[sc._base:sc._base + len(arena)].tobytes() == arena, (tag_, "arena differs")
    assert (host[sc._base + len(arena):] == CANARY).all(), (tag_, "d_arena written beyond the entries")
    gops = sc.ops_t[: 32 * len(ops)].cpu().numpy().view(M.op_dtype())
    wa = ops_array(ops)
    diff = np.nonzero(gops != wa)[0]
    assert diff.size == 0, (tag_, "ops differ at", int(diff[0]), gops[diff[0]], wa[diff[0]])
    assert tail_is_canary(sc.ops_t, 32 * len(ops)), (tag_, "d_ops written beyond the entries")
    if wmt is not None:
        assert sc.mt() == wmt, (tag_, sc.mt(), wmt)
        n = 0 if wt["status"] else wt["table_entries"]
        assert (sc.order_t[:n].cpu().numpy() == np.arange(n)).all(), (tag_, "d_order")
        assert tail_is_canary(sc.order_t, 4 * n), (tag_, "d_order written beyond the entries")
    return ops, arena


def check_image(torch, dev, image, *, table=None, shift=0, arena_shift=0, caps=None, order=True, tag_="", slack=1):
    """Open and scan of one image on the device against the model.  caps:
    (arena_cap, op_cap, block_cap), by default the model's counts times
    slack."""
    table_d = open_table(image) if table is None else table
    full = model_scan(image, table_d, order=order)
    if caps is None:
        caps = (full[0]["table_bytes"] * slack, full[0]["table_entries"] * slack, max(table_d["data_blocks"], 1) * slack)
    want = model_scan(image, table_d, arena_cap=caps[0], op_cap=caps[1], block_cap=caps[2], file_cap=len(image),
                      order=order)
    op, owner = open_on(torch, dev, image, shift, table)
    sc = run_scan(torch, dev, op, arena_cap=caps[0], op_cap=caps[1], block_cap=caps[2], arena_shift=arena_shift,
                  order=order)
    check_scan(sc, want, tag_=tag_)
    host = owner.cpu().numpy()
    base = (-owner.data_ptr()) % 16 + shift + GUARD
    assert host[base:base + len(image)].tobytes() == image and (host[:base] == CANARY).all() and \
        (host[base + len(image):] == CANARY).all(), (tag_, "the image or its guards changed")
    return sc, want


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "leveldb-rs_amd"))
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        print("wrote", dump(sys.argv[2]), "cases")
    else:
        raise SystemExit("usage: python tests/sst_scan_cases.py dump FILE")
