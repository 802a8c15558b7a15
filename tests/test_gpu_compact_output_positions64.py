"""lv_compact_output_device with positions beyond 4 GiB: an arena of 4.5 GiB
whose last file starts above 2^32, so the file offsets, the seal's absolute
handles, the offsets of the CRC batch, the filter and window places and the
version files' file_off all pass the line.  Three values are one shared extent
of 1.5 GiB of a splitmix arena no host holds; the reference is the sparse
table model of tests/positions64_cases.py, a fresh one per file, cut by
upstream's rule."""
import gc

import numpy as np
import pytest

import compact_output_cases as CO
import lvgpu.compact as C
import lvgpu.table as T
import lvgpu.version as LV
import memtable_cases as M
import positions64_cases as P
import sst_build_cases as S
from positions64_cases import HI
from write_batch_cases import CANARY, GUARD, tail_is_canary

pytestmark = pytest.mark.gpu

SEED = 0x434F3634
BIG = (3 << 29) + 4099
KEY_AREA = 1 << 12
MAX_FILE = 1 << 30
BS, RI, BPK = 4096, 16, 10


def _layout():
    """(key area, ops in log order, payload bytes): small entries, then three
    whose values are one shared extent of BIG bytes, each a block and so the
    end of a file, small entries between and behind them."""
    rng = np.random.default_rng(64)
    items = [(b"a%03d" % i, ((100 + i) << 8) | 1, int(rng.integers(0, 300))) for i in range(40)]
    for j in range(3):
        items.append((b"big%d" % j, ((5 + j) << 8) | 1, BIG))
        items += [(b"big%d-%02d" % (j, i), ((300 + i) << 8) | (0 if i == 3 else 1), int(rng.integers(0, 900))) for i in range(30)]
    keys, ops, at, big_off = bytearray(), [], KEY_AREA + 3, None
    for key, tg, vlen in items:
        ko = len(keys)
        keys += key
        if tg & 0xFF == 0:
            vlen = 0
        if vlen == BIG:
            if big_off is None:
                big_off, at = at, at + vlen
            vo = big_off
        else:
            vo, at = at, at + vlen + int(rng.integers(0, 4))
        ops.append((tg, ko, vo, len(key), vlen))
    assert len(keys) <= KEY_AREA
    ops = np.array(ops, dtype=M.op_dtype())
    return bytes(keys), ops[rng.permutation(len(ops))], at


def _model(keys, ops, crc):
    """Upstream's loop over sparse tables: [(SparseTable, first entry, entries)]."""
    order = sorted(range(len(ops)), key=lambda i: (keys[int(ops[i]["key_off"]):int(ops[i]["key_off"]) + int(ops[i]["key_len"])],
                                                   -int(ops[i]["tag"]), -i))
    files, tb, first = [], None, 0
    for at, i in enumerate(order):
        o = ops[i]
        ko, kl, vo, vl = int(o["key_off"]), int(o["key_len"]), int(o["val_off"]), int(o["val_len"])
        value = ("ext", vo, vl) if vl == BIG else P.splitmix_bytes(vo, vl, SEED)
        if tb is None:
            tb, first = P.SparseTable(BS, RI, BPK, crc), at
        tb.add(S.ikey(keys[ko:ko + kl], int(o["tag"])), value)
        if tb.size >= MAX_FILE:  # (before finish, size is the flushed bytes: upstream's FileSize())
            files.append((tb.finish(), first, at + 1 - first))
            tb = None
    if tb is not None:
        files.append((tb.finish(), first, len(order) - first))
    return files


def test_a_run_beyond_4_gib(gpu):
    import torch
    import lvgpu
    import lvgpu.memtable as MT
    keys, ops, total = _layout()
    files = _model(keys, ops, P.splitmix_crc(SEED))
    offs, at = [], 0
    for tb, _, _ in files:
        offs.append(at)
        at = CO.align16(at + tb.size)
    arena_bytes = offs[-1] + files[-1][0].size
    nb = sum(tb.totals["data_blocks"] for tb, _, _ in files)
    assert len(files) >= 4 and offs[-1] > HI and offs[-2] < HI and arena_bytes > HI + (1 << 28)
    assert sum(1 for tb, _, _ in files if tb.size > MAX_FILE) == 3 and files[-1][0].totals["data_blocks"] >= 2
    payload = torch.empty(total + 64, dtype=torch.uint8, device=gpu)
    lvgpu.fill_splitmix(payload, 0, SEED)
    payload[: len(keys)].copy_(torch.frombuffer(bytearray(keys), dtype=torch.uint8))
    n = len(ops)
    table = MT.build_device(payload[:total], M.dev_bytes(torch, gpu, ops), M.dev_i64(torch, gpu, [n]), op_cap=n)
    bound = sum(len(tb.entries[0][0]) + len(tb.entries[-1][0]) for tb, _, _ in files)
    assert C.output_arena_bound(total, n, BPK) < arena_bytes  # the values share an extent: the bound is not for this input
    out = C.output_device(table, MAX_FILE, bits_per_key=BPK, block_size=BS, restart_interval=RI, level=3, first_number=7,
                          images_off=0, arena_cap=arena_bytes, block_cap=nb, files_cap=len(files), bound_cap=5 + bound,
                          used_t=M.dev_i64(torch, gpu, [5]), fill=CANARY, guard=GUARD)
    t = out.sync()
    assert t == dict(entries=n, files=len(files), data_blocks=nb, arena_bytes=arena_bytes, handle_pairs=nb + 3 * len(files),
                     bound_bytes=bound, reserved=0, status=0)
    got_files = out.files()
    vf = out.version_files_t[: 64 * len(files)].cpu().numpy().view(LV.FILE_DTYPE)
    tabs = out.tables_t[: 64 * len(files)].cpu().numpy().view(np.uint64).reshape(-1, 8)
    blms = out.blooms_t[: 64 * len(files)].cpu().numpy().view(np.uint64).reshape(-1, 8)
    keys_got = out.bounds_t.cpu().numpy()
    pair, cursor, exts = 0, 5, 0
    for k, (tb, first, cnt) in enumerate(files):
        f = got_files[k]
        assert {x: int(f[x]) for x in CO.FILE_FIELDS} == dict(first_entry=first, entries=cnt, file_off=offs[k], file_bytes=tb.size,
                                                             data_blocks=tb.totals["data_blocks"], first_handle=pair,
                                                             filter_keys=cnt, reserved=0), k
        hs = out.handles_t[2 * pair: 2 * (pair + len(tb.handles))].cpu().numpy().view(np.uint64).reshape(-1, 2)
        assert [tuple(map(int, r)) for r in hs] == tb.handles, k
        assert dict(zip(CO.TABLE_FIELDS, map(int, tabs[k]))) == tb.table(), k
        assert dict(zip(T.BLOOM_FIELDS, map(int, blms[k]))) == tb.bloom(), k
        small, large = tb.entries[0][0], tb.entries[-1][0]
        assert {x: int(vf[k][x]) for x in LV.FILE_DTYPE.names} == dict(
            number=7 + k, file_off=offs[k], file_cap=tb.size, smallest_off=cursor, largest_off=cursor + len(small),
            smallest_len=len(small), largest_len=len(large), level=3, status=0, reserved=0), k
        assert keys_got[cursor: cursor + len(small) + len(large)].tobytes() == small + large, k
        cursor += len(small) + len(large)
        for at, seg in tb.placed():  # every bytes segment by read-back, every extent against the payload on the device
            if isinstance(seg, tuple):
                a, b = out.arena_t[offs[k] + at: offs[k] + at + seg[2]], payload[seg[1]: seg[1] + seg[2]]
                assert all(torch.equal(a[i:i + (1 << 28)], b[i:i + (1 << 28)]) for i in range(0, seg[2], 1 << 28)), (k, at)
                exts += 1
            else:
                got = out.arena_t[offs[k] + at: offs[k] + at + len(seg)].cpu().numpy().tobytes()
                assert got == bytes(seg), (k, "file differs in the segment at", at)
        if k:  # the gap behind the file before
            gap = out.arena_t[offs[k - 1] + files[k - 1][0].size: offs[k]]
            assert gap.numel() < 16 and bool((gap == CANARY).all()), k
        st = T.verify_blocks(out.arena_t[offs[k]: offs[k] + tb.size], out.file_handles_view(k))
        assert int(st.abs().sum()) == 0, k
        pair += len(tb.handles)
    assert exts == 3 and int(out.used_t.cpu()[0]) == cursor == 5 + bound
    assert (keys_got[:5] == CANARY).all() and tail_is_canary(out.bounds_t, cursor)
    assert tail_is_canary(out.arena_t, arena_bytes) and tail_is_canary(out.handles_t, 16 * pair)
    for t_ in (out.files_t, out.tables_t, out.blooms_t, out.version_files_t):
        assert tail_is_canary(t_, 64 * len(files))
    del out, table, payload
    gc.collect()
    torch.cuda.empty_cache()
