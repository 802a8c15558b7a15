"""lv_compact_output_device at sizes where the capped kernels it reuses walk
their grid-stride loops more than once (sb_carry, sb_bloom_emit, sb_bloom_big,
sb_bloom_offsets, the seal), sized with tests/loop_trips.py, and over random
tables.  The large input is compared with the host twin, which
tests/test_compact_output.py holds to the model."""
import numpy as np
import pytest

import compact_output_cases as CO
import loop_trips as LT
import lvgpu.compact as C
import lvgpu.table as T
import memtable_cases as M
import sst_build_cases as S
from memtable_cases import make_table

pytestmark = pytest.mark.gpu


def _same(name, got_t, want, used):
    got = got_t.view(__import__("torch").uint8)[:used].cpu().numpy()
    want = np.frombuffer(want.tobytes(), dtype=np.uint8)[:used]
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, (name, "differs at byte", int(diff[0]))
    assert CO.tail_is_canary(got_t, used), (name, "written beyond", used)


def _same_outputs(out, want):
    """Every output of a device call against the host twin's.  The twin's
    buffers were filled with the canary first and it writes no gap between two
    files (tests/test_compact_output.py), so the arenas compare as they are."""
    t = want.totals
    nf = t["files"]
    _same("arena", out.arena_t, want.arena, t["arena_bytes"])
    _same("handles", out.handles_t, want.handles, 16 * t["handle_pairs"])
    _same("files", out.files_t, want.files, 64 * nf)
    _same("tables", out.tables_t, want.tables, 64 * nf)
    _same("blooms", out.blooms_t, want.blooms, 64 * nf)
    _same("version files", out.version_files_t, want.version_files, 64 * nf)
    _same("bound keys", out.bounds_t, want.bounds, want.bound_used)
    assert int(out.used_t.cpu()[0]) == want.bound_used


def test_third_trip_of_every_reused_capped_kernel(gpu):
    """An entry per block and per file (block_size 1, max_file_bytes 1) with a
    filter, so entries = blocks = files = windows = n: sb_carry scans columns
    by entry, by block and by file, the filter kernels walk n blocks and n
    windows, and the seal n data blocks and n metaindex blocks.  n is the
    smallest at which sb_bloom_offsets, the widest of them, takes a third
    trip."""
    import torch
    cus = LT.device_cus(gpu)
    n = LT.size_for("sb_bloom_offsets", 3, cus, 17)
    items = S.seq_items(n)
    payload, ops = make_table(items)
    order = np.arange(n, dtype=np.uint32)  # ascending distinct keys: the memtable order
    mt = dict(entries=n, user_keys=n, status=0)
    want = C.output_host(payload, ops, order, mt, 1, bits_per_key=10, block_size=1, restart_interval=16, bound_used=5,
                         guard=0)
    t = want.totals
    assert t["files"] == t["data_blocks"] == n and t["status"] == 0
    # the units of each launch, as compact_output.hip sizes them
    windows = (t["arena_bytes"] >> 11) + n
    grid, per = LT.grid_of("sb_bloom_offsets", windows, cus)
    assert -(-n // (grid * per)) >= 3  # n windows in all: a lane per window
    for kernel, units in (("sb_carry", n), ("sb_bloom_emit", n), ("sst_blocks_kernel", 2 * n)):
        assert LT.trips(kernel, units, cus) >= 3, kernel
    table, buf = M.run_build(torch, gpu, payload, ops)
    used_t = M.dev_i64(torch, gpu, [5])
    ws = torch.full((C.output_workspace_bytes(n, n, n),), 0x5A, dtype=torch.uint8, device=gpu)
    out = C.output_device(table, 1, bits_per_key=10, block_size=1, restart_interval=16, arena_cap=t["arena_bytes"],
                          block_cap=n, files_cap=n, bound_cap=want.bound_used, used_t=used_t, workspace=ws,
                          fill=CO.CANARY, guard=CO.GUARD)
    assert out.sync() == t
    _same_outputs(out, want)
    for k in (0, n // 2, n - 1):
        f = want.files[k]
        file_t = out.arena_t[int(f["file_off"]): int(f["file_off"] + f["file_bytes"])]
        assert int(T.verify_blocks(file_t, out.file_handles_view(k)).abs().sum()) == 0, k


def test_second_trip_with_files_of_several_blocks(gpu):
    """sb_carry's second round over entries and blocks, the seal's and the
    filter emit's later trips, with a few entries per block and a few blocks
    per file, so that the files' own scans stay in their first round."""
    import torch
    cus = LT.device_cus(gpu)
    n = LT.size_for("sb_carry", 2, cus, 2517) * 3
    items = S.tile_items(n, seed=4)
    payload, ops = make_table(items)
    order, mt = M.model_totals(payload, ops)
    want = C.output_host(payload, ops, order, mt, 100, bits_per_key=10, block_size=32, restart_interval=2, bound_used=5,
                         guard=0)
    t = want.totals
    assert LT.trips("sb_carry", t["data_blocks"], cus) >= 2 and LT.trips("sb_carry", n, cus) >= 3
    assert LT.trips("sb_carry", t["files"], cus) == 1 and t["files"] >= 8
    assert LT.trips("sst_blocks_kernel", t["data_blocks"] + t["files"], cus) >= 3
    table, buf = M.run_build(torch, gpu, payload, ops)
    used_t = M.dev_i64(torch, gpu, [5])
    out = C.output_device(table, 100, bits_per_key=10, block_size=32, restart_interval=2, arena_cap=t["arena_bytes"],
                          block_cap=t["data_blocks"], files_cap=t["files"], bound_cap=want.bound_used, used_t=used_t,
                          fill=CO.CANARY, guard=CO.GUARD)
    assert out.sync() == t
    _same_outputs(out, want)


def test_third_trip_of_the_large_filter_kernel(gpu):
    """sb_bloom_big walks the blocks only when some filter is beyond the LDS
    budget: one block of 2,000 entries (a filter of 2,500 bytes), then blocks
    of one entry each with a value of block_size bytes, enough of them for
    its third trip; every block is a file."""
    import torch
    cus = LT.device_cus(gpu)
    nb = LT.size_for("sb_bloom_big", 3, cus, 7)
    head = [(b"%08d" % i, 1 << 8 | 1, b"") for i in range(2000)]
    payload, ops = make_table(head)
    bs = S.model_build(payload, ops, 1 << 30, 16)[1][0][1]  # the one block's size: its last estimate
    value = b"V" * bs
    items = head + [(b"z%07d" % i, 1 << 8 | 1, value) for i in range(nb)]
    payload, ops = make_table(items)
    order = np.arange(len(items), dtype=np.uint32)  # ascending distinct keys: the memtable order
    mt = dict(entries=len(items), user_keys=len(items), status=0)
    want = C.output_host(payload, ops, order, mt, 1, bits_per_key=10, block_size=bs, restart_interval=16, bound_used=5,
                         guard=0)
    t = want.totals
    assert t["files"] == t["data_blocks"] == nb + 1 and int(want.files[0]["entries"]) == 2000
    assert int(want.blooms[0][2]) > T.SB_BLOOM_LDS and LT.trips("sb_bloom_big", t["data_blocks"], cus) >= 3
    table, buf = M.run_build(torch, gpu, payload, ops)
    used_t = M.dev_i64(torch, gpu, [5])
    out = C.output_device(table, 1, bits_per_key=10, block_size=bs, restart_interval=16, arena_cap=t["arena_bytes"],
                          block_cap=t["data_blocks"], files_cap=t["files"], bound_cap=want.bound_used, used_t=used_t,
                          fill=CO.CANARY, guard=CO.GUARD)
    assert out.sync() == t
    _same_outputs(out, want)


def test_random_tables(gpu):
    """Adversarial tables (tiny and huge keys, empty values, long shared
    prefixes) under every max_file_bytes of the CPU test, against the model."""
    import torch
    rng = np.random.default_rng(91)
    files = 0
    for t, (items, bs, ri) in enumerate(S.adversarial_tables(rng, 40)):
        payload, ops = make_table(items)
        sizes = [sz + 5 for _, sz in S.model_build(payload, ops, bs, ri)[1][:-2]]
        mf = [1, max(sizes[0] - 1, 1), sizes[0] + 1, sum(sizes[:3]), 1 << 63][t % 5]
        out, w = CO.run_device(torch, gpu, payload, ops, mf, 10 if t % 3 else None, bs, ri, shift=t % 8)
        CO.compare_device(out, w, f"trial {t}", verify=t % 4 == 0)
        files += w.totals["files"]
    assert files > 150
