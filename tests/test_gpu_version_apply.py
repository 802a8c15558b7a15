"""lv_version_apply_device against its host twin, byte for byte: the rows, the
directory indices and the totals.  Every output is canary-filled with a guard
behind it, the workspace is dirty, and with a status bit set nothing but the
totals may be written.  The shapes lie around the kernels' tiles
(csrc/version_set.hip: 256 items per workgroup, 1,024 rows per scan tile and
per sort tile, 16 key bytes per sort entry)."""
import numpy as np
import pytest

import lvgpu.version as V
import lvgpu.version_edit as VE
import lvgpu.version_set as VS
import version_apply_cases as C
import version_edit_cases as EC

pytestmark = pytest.mark.gpu
CANARY, GUARD, DIRTY = 0xA5, 64, 0x5A


def up(torch, gpu, b, shift=0):
    """Bytes as a uint8 tensor on the device, `shift` bytes into its buffer."""
    b = bytes(b)
    t = torch.full((shift + max(len(b), 1) + 16,), 0xEE, dtype=torch.uint8, device=gpu)
    if b:
        t[shift: shift + len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return t[shift: shift + len(b)]


def i64(torch, gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(gpu)


def device(torch, gpu, case, *, shift=0, files_cap=None, records=None, upstream=None, rec_cap=None, extra_rec=0, stream=None):
    src, E, F, bf, D, bd, P, bp, dr = case
    n = len(E)
    rec_cap = n + extra_rec if rec_cap is None else rec_cap
    pad = lambda b: np.concatenate([np.asarray(b, dtype=np.uint64), np.full(max(rec_cap + 1 - len(b), 0), 0xEEEEEEEE, dtype=np.uint64)])
    tabs = [up(torch, gpu, np.ascontiguousarray(a).tobytes()) for a in (E, F, D, P)]
    if extra_rec:
        tabs[0] = up(torch, gpu, np.ascontiguousarray(E).tobytes() + b"\xee" * (64 * extra_rec))
    d_dir = up(torch, gpu, VS.placements(dr).tobytes()) if dr else None
    ws_bytes = VS.workspace_bytes(len(F), len(D), len(F) if files_cap is None else files_cap)
    ws = torch.full((max(ws_bytes, 16),), DIRTY, dtype=torch.uint8, device=gpu)
    return VS.apply_device(up(torch, gpu, src, shift), tabs[0], tabs[1], i64(torch, gpu, pad(bf)), tabs[2],
                           i64(torch, gpu, pad(bd)), tabs[3], i64(torch, gpu, pad(bp)),
                           i64(torch, gpu, [n if records is None else records]),
                           None if upstream is None else i64(torch, gpu, [upstream]), directory=d_dir,
                           dir_n=len(dr) if dr else 0, rec_cap=rec_cap, caps=(len(F), len(D), len(P)),
                           files_cap=len(F) if files_cap is None else files_cap, workspace=ws, stream=stream, fill=CANARY,
                           guard=GUARD)


def assert_equal_to_twin(torch, a, want, files_cap):
    """`want` = (rows, index, totals) of the twin (or the model, as dicts)."""
    rows, index, wt = want
    t = a.sync_totals(check=False)
    assert t == wt
    files_t, index_t = a.files_t.cpu().numpy(), a.dir_index_t.cpu().numpy().view(np.uint8)
    n = 0 if wt["status"] else wt["live"]
    if isinstance(rows, np.ndarray):
        assert files_t[: 64 * n].tobytes() == rows.tobytes()
        assert index_t[: 4 * n].tobytes() == np.asarray(index, dtype=np.uint32).tobytes()
    else:
        assert n == 0 and not rows
    assert (files_t[64 * n:] == CANARY).all() and len(files_t) >= 64 * files_cap + GUARD   # untouched, the guard too
    assert (index_t[4 * n:] == CANARY).all() and len(index_t) >= 4 * files_cap + GUARD


def twin(case, **kw):
    src, E, F, bf, D, bd, P, bp, dr = case
    return VS.apply_host(src, E, F, bf, D, bd, P, bp, VS.placements(dr) if dr else None, **kw)


def check(torch, gpu, case, **kw):
    files_cap = kw.get("files_cap", len(case[2]))
    a = device(torch, gpu, case, **kw)
    want = twin(case, files_cap=files_cap)
    assert_equal_to_twin(torch, a, want, files_cap)
    return want


@pytest.mark.parametrize("upto", (0, 1, 3, 6))
def test_zero_records_and_the_worked_example(gpu, upto):
    import torch
    case = C.case_of(C.example_edits(upto))
    rows, index, t = check(torch, gpu, case, extra_rec=3)
    if upto == 6:
        assert [(int(r["level"]), int(r["number"])) for r in rows] == [(0, 12), (0, 9), (1, 7), (2, 10), (2, 8)]
        assert t["level_bytes"][:3] == [900, 1000, 1000] and t["next_file_number"] == 13 and t["compact_pointer"][0] == 1
    if upto == 0:
        assert t["live"] == 0 and t["status"] == 0


def test_no_tables_at_all(gpu):
    """rec_cap 0 and every capacity 0: the call still writes the totals."""
    import torch
    check(torch, gpu, C.case_of([]))


@pytest.mark.parametrize("shift, with_dir", [(0, True), (1, False), (3, True)])
def test_ragged_tiles_over_all_levels(gpu, shift, with_dir):
    """300 records, about 1,500 NewFile and 1,150 deleted rows: ragged across
    the 256-item workgroups and the 1,024-row tiles, all seven levels, a
    directory with gaps or none, d_src at an odd byte."""
    import torch
    edits, directory = C.random_history(21 + shift, 300, per_flush=7, compaction_width=12, level0_share=0.25,
                                        compaction_share=0.55)
    case = C.case_of(edits, directory if with_dir else None, lead=(3, 2, 1))
    rows, index, t = check(torch, gpu, case, shift=shift)
    assert t["status"] == 0 and 1100 < t["new_files"] < 2047 and t["new_files"] % 256 and 1024 < t["deleted"] < 2047
    assert set(int(x) for x in case[2]["level"][3:]) == set(range(7)) and t["live"] > 100
    assert sum(1 for x in t["level_files"] if x) >= 4
    assert (0 < t["unplaced"] < t["live"]) == with_dir


def test_more_than_one_merge_pass(gpu):
    """About 2,500 live files, many of them on level 0: three sort tiles, two
    merge passes, the last tile ragged."""
    import torch
    edits, directory = C.random_history(33, 1100, per_flush=4, compaction_width=2, compaction_out=3, level0_share=0.6)
    case = C.case_of(edits, directory)
    rows, index, t = check(torch, gpu, case, shift=1)
    assert 2048 < t["live"] < 3072 and t["level_files"][0] > 1024 and sum(1 for x in t["level_files"] if x) >= 3


def test_keys_that_stress_the_compare(gpu):
    """Deeper levels only see the key compare: 8- and 9-byte internal keys,
    keys over 200 bytes that share more than 16 bytes, equal user keys that
    differ in the tag only."""
    import torch
    edits, directory = C.random_history(44, 700, per_flush=3, level0_share=0.12, compaction_share=0.6, compaction_width=2,
                                        compaction_out=6, styles=(0, 1, 2, 3))
    case = C.case_of(edits, None)
    rows, index, t = check(torch, gpu, case, shift=5)
    src = case[0]
    deep = [r for r in rows if r["level"] >= 1]
    lens = [int(r["smallest_len"]) for r in deep]
    assert len(deep) > 300 and 8 in lens and 9 in lens and max(lens) > 200 + 8
    users = [src[int(r["smallest_off"]): int(r["smallest_off"]) + int(r["smallest_len"]) - 8] for r in deep]
    same = [(a, b) for a, b, x, y in zip(users, users[1:], deep, deep[1:]) if a == b and x["level"] == y["level"]]
    assert len(same) > 20                                       # neighbours the tag alone orders
    assert any(len(a) > 16 and a[:16] == b[:16] and a != b for a, b in zip(users, users[1:]))


def test_file_over_then_one_retry(gpu):
    import torch
    edits, directory = C.random_history(5, 200, per_flush=3)
    case = C.case_of(edits, directory)
    live = twin(case)[2]["live"]
    assert live > 40
    rows, index, t = check(torch, gpu, case, files_cap=live - 1)
    assert t["status"] == VS.FILE_OVER and t["live"] == live and t["level_files"] != [0] * 7
    assert check(torch, gpu, case, files_cap=live)[2]["status"] == 0


@pytest.mark.parametrize("name, case, kw, want", C.damaged_cases(), ids=[c[0] for c in C.damaged_cases()])
def test_each_damaged_input(gpu, name, case, kw, want):
    import torch
    rows, index, t = check(torch, gpu, case, **kw)
    assert (t["status"], t["bad_kind"], t["bad_row"]) == want


def test_upstream_and_rec_over(gpu):
    """The two bits the twin cannot raise, against the model."""
    import torch
    edits, directory = C.random_history(8, 40)
    case = C.case_of(edits, directory)
    for kw, mkw in ((dict(upstream=7), dict(upstream=7)),
                    (dict(records=len(edits) + 1), dict(records=len(edits) + 1, rec_cap=len(edits))),
                    (dict(upstream=1, records=len(edits) + 5), dict(upstream=1))):
        a = device(torch, gpu, case, **kw)
        want = C.model(*case, **mkw)
        assert want[2]["status"] in (VS.UPSTREAM, VS.REC_OVER)
        assert_equal_to_twin(torch, a, want, len(case[2]))
    a = device(torch, gpu, case, upstream=0)                    # a zero upstream status is no status
    assert_equal_to_twin(torch, a, twin(case), len(case[2]))


def test_argument_checks(gpu):
    import torch
    case = C.case_of(C.example_edits())
    src, E, F, bf, D, bd, P, bp, _ = case
    with pytest.raises(VS.LvError, match="files_cap"):
        device(torch, gpu, case, files_cap=V.MAX_FILES + 1)
    t = [up(torch, gpu, np.ascontiguousarray(a).tobytes()) for a in (E, F, D, P)]
    b = [i64(torch, gpu, x) for x in (bf, bd, bp)]
    n = i64(torch, gpu, [len(E)])
    s = up(torch, gpu, src)
    with pytest.raises(VS.LvError, match="flag"):
        VS.apply_device(s, t[0], t[1], b[0], t[2], b[1], t[3], b[2], n, flags=1)
    with pytest.raises(VS.LvError, match="workspace too small"):
        VS.apply_device(s, t[0], t[1], b[0], t[2], b[1], t[3], b[2], n, workspace=torch.empty(64, dtype=torch.uint8, device=gpu))
    with pytest.raises(VS.LvError, match="aligned"):
        VS.apply_device(s, t[0], up(torch, gpu, F.tobytes(), 8), b[0], t[2], b[1], t[3], b[2], n)
    with pytest.raises(VS.LvError, match="aligned"):
        VS.apply_device(s, t[0], t[1], b[0], t[2], b[1], t[3], b[2], n, directory=up(torch, gpu, bytes(64), 4), dir_n=1)


def test_decode_apply_open_in_a_graph(gpu):
    """The chain lv_version_edit_decode_device -> apply -> lv_version_open_device
    captured once and replayed over a second manifest in the same buffers: the
    payload is the apply's d_src and the open's bound keys, the decode's
    bad_records the apply's upstream status, the apply's status the open's, and
    the tables reach the open through d_dir_index."""
    import torch
    live = 1500
    sets = []
    for seed in (0, 1):
        edits, directory = C.consistent_history(60 + seed, live, level0=5 + 40 * seed)
        payload, off, ln = EC.lay_out([EC.encode_to(e) for e in edits])
        sets.append((payload, off, ln, directory, C.case_of(edits, directory)))
    rcap, pcap = max(len(s[1]) for s in sets) + 7, max(len(s[0]) for s in sets) + 16
    dcap = max(len(s[3]) for s in sets)
    caps = (pcap // 6, pcap // 3, pcap // 3)
    files_cap = 2048
    d_pay = torch.zeros(pcap, dtype=torch.uint8, device=gpu)
    d_off = torch.zeros(rcap, dtype=torch.int64, device=gpu)
    d_len = torch.zeros(rcap, dtype=torch.int64, device=gpu)
    d_n = torch.zeros(1, dtype=torch.int64, device=gpu)
    d_dir = torch.zeros(dcap * 32, dtype=torch.uint8, device=gpu)
    d_tabs = torch.zeros((dcap, 8), dtype=torch.int64, device=gpu)   # lv_sst_table per directory entry
    dws = torch.empty(VE.decode_workspace_bytes(rcap), dtype=torch.uint8, device=gpu)
    aws = torch.empty(VS.workspace_bytes(caps[0], caps[1], files_cap), dtype=torch.uint8, device=gpu)
    assert all(len(s[3]) == dcap == live for s in sets)
    images_bytes = max(s[3][-1][1] + s[3][-1][2] for s in sets)

    def load(k):
        payload, off, ln, directory, _ = sets[k]
        d_pay.fill_(0x11)
        d_pay[: len(payload)].copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
        d_off[: len(off)].copy_(i64(torch, gpu, off))
        d_len[: len(ln)].copy_(i64(torch, gpu, ln))
        d_n.fill_(len(off))
        pl = VS.placements(directory)
        d_dir.copy_(torch.frombuffer(bytearray(pl.tobytes()), dtype=torch.uint8))
        tabs = np.zeros((dcap, 8), dtype=np.uint64)
        tabs[:, 0] = pl["file_cap"] - 7                          # file_bytes: what lv_version_open_device looks at
        d_tabs.copy_(i64(torch, gpu, tabs))

    def run(stream=None):
        d = VE.decode_device(d_pay, d_off, d_len, d_n, rec_cap=rcap, caps=caps, workspace=dws, stream=stream)
        a = VS.apply_device(d_pay, d.edits_t, d.files_t, d.rec_file, d.deleted_t, d.rec_deleted, d.pointers_t,
                            d.rec_pointer, d.totals[0:1], d.totals[4:5], directory=d_dir, dir_n=dcap, rec_cap=rcap,
                            caps=caps, files_cap=files_cap, workspace=aws, stream=stream)
        tabs = d_tabs.index_select(0, a.dir_index_t[:live].to(torch.int64))
        o = V.open_device(d_pay, a.files_t, tabs, live, d_pay, images_bytes=images_bytes,
                          upstream_status=a.totals[35:36], stream=stream)
        return d, a, o

    def verify(k, d, a, o):
        payload, off, ln, directory, case = sets[k]
        torch.cuda.synchronize()
        d._tot = a._tot = None
        assert d.sync_totals()["bad_records"] == 0
        # the device's tables are the model decode's with offsets into the payload: the twin over them
        E, F, D, P, (bf, bd, bp), _ = EC.decode_batch(payload, off, ln)
        rows, index, t = VS.apply_host(payload, E, F, bf, D, bd, P, bp, VS.placements(directory), files_cap=files_cap)
        assert t["status"] == 0 and t["live"] == live and t["unplaced"] == 0
        assert a.sync_totals() == t and a.files().tobytes() == rows.tobytes() and a.dir_index().tobytes() == index.tobytes()
        v = o.sync()
        starts = [int(x) for x in np.concatenate([[0], np.cumsum(t["level_files"])])]
        assert v["status"] == 0 and v["files"] == live and v["level_start"] == starts
        assert t["level_files"][0] == 5 + 40 * k and t["pointers"] > 100

    load(0)
    verify(0, *run())
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            d, a, o = run(s)
    torch.cuda.synchronize()
    for k in (1, 0):
        load(k)
        dws.fill_(0x33)
        aws.fill_(0x44)
        a.files_t.fill_(0)
        torch.cuda.synchronize()
        g.replay()
        verify(k, d, a, o)
