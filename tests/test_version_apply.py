"""lv_version_apply_host (include/lvgpu/version_set.h) against the serial model
of tests/version_apply_cases.py, the worked example, a round trip through a
snapshot record, and the store of tests/store_cases.py, whose own Python
bookkeeping of the version predates the entry point.  No GPU."""
import numpy as np
import pytest

import lvgpu.table as T
import lvgpu.version as V
import lvgpu.version_edit as VE
import lvgpu.version_set as VS
import store_cases as SC
import version_apply_cases as C
import version_edit_cases as EC


def host(case, **kw):
    src, E, F, bf, D, bd, P, bp, dr = case
    return VS.apply_host(src, E, F, bf, D, bd, P, bp, VS.placements(dr) if dr is not None else None, **kw)


def assert_same(got, want):
    rows, index, t = got
    wrows, windex, wt = want
    assert t == wt
    assert C.rows_as_dicts(rows) == wrows
    assert [int(x) for x in index] == windex


def test_structs_and_constants():
    assert VS.TOTALS_WORDS * 8 == 304 and VS.PLACEMENT_DTYPE.itemsize == 32
    assert (VS.UPSTREAM, VS.REC_OVER, VS.BAD_BOUNDS, VS.BAD_ROW, VS.DUPLICATE, VS.BAD_DIRECTORY, VS.FILE_OVER) == \
        (C.UPSTREAM, C.REC_OVER, C.BAD_BOUNDS, C.BAD_ROW, C.DUPLICATE, C.BAD_DIRECTORY, C.FILE_OVER)
    assert (VE.KIND_POINTER, VE.KIND_DELETED, VE.KIND_FILE, VS.KIND_DIRECTORY) == (1, 2, 3, 4)
    assert VS.workspace_bytes(0, 0, 0) > 0
    assert VS.workspace_bytes(VS.MAX_ROWS + 1, 0, 0) == 0 and VS.workspace_bytes(0, VS.MAX_ROWS + 1, 0) == 0
    assert VS.workspace_bytes(0, 0, V.MAX_FILES + 1) == 0 and VS.workspace_bytes(VS.MAX_ROWS, VS.MAX_ROWS, V.MAX_FILES) > 0
    # the pair table: a power of two of at least 2 x (file_cap + deleted_cap) slots of 16 bytes
    assert VS.workspace_bytes(3000, 1096, 0) - VS.workspace_bytes(0, 0, 0) >= 8192 * 16


@pytest.mark.parametrize("upto", range(0, 7))
def test_worked_example_and_its_prefixes(upto):
    g = C.golden()
    case = C.case_of(C.example_edits(upto))
    rows, index, t = host(case)
    assert_same((rows, index, t), C.model(*case))
    if upto == 0:
        assert t["live"] == 0 and t["status"] == 0 and t["has"] == 0
        return
    want = g["after"][upto - 1]
    assert [(int(r["level"]), int(r["number"])) for r in rows] == [tuple(x) for x in want["files"]]
    for name in ("level_files", "level_bytes", "compact_pointer", "log_number", "next_file_number", "last_sequence",
                 "max_file_number"):
        assert t[name] == want[name], name
    assert t["records"] == upto and t["unplaced"] == 0 and [int(x) for x in index] == [VS.NO_DIR_INDEX] * len(rows)
    src, F = case[0], case[2]
    for r in rows:  # the bounds are the rows' own extents, file_size stays reachable
        f = F[int(r["reserved"])]
        assert (r["number"], r["smallest_off"], r["smallest_len"], r["largest_off"], r["largest_len"]) == \
            (f["number"], f["smallest_off"], f["smallest_len"], f["largest_off"], f["largest_len"])
        assert (r["file_off"], r["file_cap"], r["status"]) == (0, f["file_size"], 0)


def test_worked_example_level_1_order_after_record_2():
    """#8's row comes first, #7's smallest key is the smaller."""
    rows, _, _ = host(C.case_of(C.example_edits(3)))
    assert [int(r["number"]) for r in rows] == [7, 8] and [int(r["reserved"]) for r in rows] == [3, 2]


@pytest.mark.parametrize("seed", range(8))
def test_random_histories_against_the_model(seed):
    edits, directory = C.random_history(seed, 30 + 25 * seed, per_flush=1 + seed % 3)
    case = C.case_of(edits, directory if seed % 3 else None, lead=(seed % 3, seed % 2, 1))
    got = host(case)
    assert_same(got, C.model(*case))
    t = got[2]
    assert t["status"] == 0 and t["live"] > 5 and t["deleted"] > 5 and t["pointers"] > 0
    if seed % 3:
        assert 0 < t["unplaced"] < t["live"]
    if seed >= 4:
        assert sum(1 for x in t["level_files"] if x) >= 3
    levels = [int(r["level"]) for r in got[0]]
    assert levels == sorted(levels)


def test_histories_hold_what_the_contract_allows():
    """The generator produces each pattern the contract calls not an error."""
    edits, _ = C.random_history(3, 120)
    adds = {}
    for r, e in enumerate(edits):
        for f in e["files"]:
            assert (f[0], f[1]) not in adds
            adds[(f[0], f[1])] = r
    dels = [(pair, r) for r, e in enumerate(edits) for pair in e["deleted"]]
    assert any(pair not in adds for pair, r in dels)                                 # nobody added it
    assert any(pair in adds and adds[pair] == r for pair, r in dels)                 # beside its add
    assert any(pair in adds and adds[pair] > r for pair, r in dels)                  # before its add
    assert any(pair in adds and adds[pair] < r for pair, r in dels)                  # the ordinary one
    numbers = [n for _, n in adds]
    assert len(set(numbers)) < len(numbers)                                          # a trivial move: one number, two levels


@pytest.mark.parametrize("name, case, kw, want", C.damaged_cases(), ids=[c[0] for c in C.damaged_cases()])
def test_every_status_bit(name, case, kw, want):
    rows, index, t = host(case, **kw)
    assert (t["status"], t["bad_kind"], t["bad_row"]) == want
    assert_same((rows, index, t), C.model(*case, **kw))
    assert len(rows) == 0
    if want[0] != VS.FILE_OVER:
        assert all(v in (0, [0] * 7) for n, v in t.items() if n not in ("records", "status", "bad_kind", "bad_row"))
    else:
        assert t["live"] > kw["files_cap"]
        again = host(case, files_cap=t["live"])  # one retry suffices
        assert again[2]["status"] == 0 and len(again[0]) == t["live"]


def test_host_argument_checks():
    case = C.case_of(C.example_edits())
    src, E, F, bf, D, bd, P, bp, _ = case
    with pytest.raises(VS.LvError):
        VS.apply_host(src, E, F, bf, D, bd, P, bp, files_cap=V.MAX_FILES + 1)
    with pytest.raises(VS.LvError):
        VS.apply_host(src, E, F, bf, D, bd, P, bp, caps=(VS.MAX_ROWS + 1, len(D), len(P)))
    with pytest.raises(VS.LvError):
        VS.apply_host(src, E, F, bf, D, bd, P, bp, records=VS.MAX_REC_CAP + 1)


def snapshot_of(src, rows, F, t):
    """The version as one record: every file a NewFile row (what
    lv_version_edit_files_device makes of lv_version_file records), with the
    scalars Recover keeps: upstream's WriteSnapshot."""
    e = np.zeros(1, dtype=VE.EDIT_DTYPE)
    e["log_number"], e["prev_log_number"], e["next_file_number"], e["last_sequence"] = (
        t["log_number"], t["prev_log_number"], t["next_file_number"], t["last_sequence"])
    e["has"] = t["has"] & ~VE.HAS_COMPARATOR
    f = np.zeros(len(rows), dtype=VE.FILE_DTYPE)
    for o, r in zip(f, rows):
        for name in ("number", "smallest_off", "smallest_len", "largest_off", "largest_len", "level"):
            o[name] = r[name]
        o["file_size"] = F[int(r["reserved"])]["file_size"]
    return e, f


@pytest.mark.parametrize("seed", (0, 5))
def test_round_trip_through_a_snapshot_record(seed):
    edits, directory = C.random_history(40 + seed, 90)
    case = C.case_of(edits, directory)
    rows, index, t = host(case)
    assert t["status"] == 0 and t["live"] > 10
    e, f = snapshot_of(case[0], rows, case[2], t)
    none_d, none_p = np.zeros(0, dtype=VE.DELETED_DTYPE), np.zeros(0, dtype=VE.POINTER_DTYPE)
    rec, off, ln, et = VE.encode_host(case[0], e, f, [0, len(f)], none_d, [0, 0], none_p, [0, 0])
    assert et["status"] == 0 and len(off) == 1
    E2, F2, D2, P2, (bf2, bd2, bp2), dt = EC.decode_batch(rec, off, ln)
    st, e2, f2, d2, p2, _ = VE.decode_host(rec)
    assert st == VE.OK and f2.tobytes() == F2.tobytes() and dt["bad_records"] == 0
    rows2, index2, t2 = VS.apply_host(rec, e2, f2, bf2, d2, bd2, p2, bp2, VS.placements(directory))
    assert t2["status"] == 0 and [int(x) for x in index2] == [int(x) for x in index]
    key = lambda s, r, which: bytes(s[int(r[which + "_off"]): int(r[which + "_off"]) + int(r[which + "_len"])])
    same = ("number", "level", "file_off", "file_cap", "status")
    assert [[int(r[n]) for n in same] for r in rows2] == [[int(r[n]) for n in same] for r in rows]
    assert [(key(rec, r, "smallest"), key(rec, r, "largest")) for r in rows2] == \
        [(key(case[0], r, "smallest"), key(case[0], r, "largest")) for r in rows]
    for name in ("live", "unplaced", "level_files", "level_bytes", "log_number", "prev_log_number", "next_file_number",
                 "last_sequence", "max_file_number"):
        assert t2[name] == t[name], name


# ---- against the store ----------------------------------------------------------------
def manifest_tables(backend, manifest):
    """The decoded MANIFEST of a store as one payload and the apply's tables."""
    records, dropped = backend.read_log(bytes(manifest))
    assert dropped == 0
    payload = b"".join(records)
    off = np.cumsum([0] + [len(r) for r in records[:-1]], dtype=np.uint64) if records else np.zeros(0, dtype=np.uint64)
    E, F, D, P, (bf, bd, bp), tot = EC.decode_batch(payload, off, [len(r) for r in records])
    assert tot["bad_records"] == 0
    for r, rec in enumerate(records):  # the model's decode is the library's
        st, e, f, d, p, _ = VE.decode_host(rec)
        assert st == VE.OK and len(f) == bf[r + 1] - bf[r] and len(d) == bd[r + 1] - bd[r]
    return payload, E, F, bf, D, bd, P, bp


def test_against_the_store():
    """After every flush and compaction and after the reopen, the decoded
    MANIFEST applied with the store's directory is the store's version."""
    store, model = SC.Store(SC.HostBackend()), SC.StoreModel()
    seen = []

    def checkpoint(store, model, name):
        if "group" in name and seen and seen[-1][1] == len(store.manifest):
            return
        payload, E, F, bf, D, bd, P, bp = manifest_tables(store.b, store.manifest)
        rows, index, t = VS.apply_host(payload, E, F, bf, D, bd, P, bp, VS.placements(store.directory))
        seen.append((name, len(store.manifest), t["live"]))
        assert t["status"] == 0 and t["unplaced"] == 0, (name, t)
        order = store.ordered()
        assert [int(r["number"]) for r in rows] == order and set(order) == set(store.files), name
        key = lambda r, which: payload[int(r[which + "_off"]): int(r[which + "_off"]) + int(r[which + "_len"])]
        for r in rows:
            level, size, smallest, largest = store.files[int(r["number"])]
            assert (int(r["level"]), key(r, "smallest"), key(r, "largest")) == (level, smallest, largest), name
            assert (int(r["file_off"]), int(r["file_cap"])) == store.directory[int(r["number"])]
            assert int(F[int(r["reserved"])]["file_size"]) == size == int(r["file_cap"])
        assert [int(x) for x in index] == [sorted(store.directory).index(n) for n in order]
        if len(E):
            assert t["log_number"] == store.log_number and t["last_sequence"] == store.manifest_last_sequence, name
            assert max(t["next_file_number"], t["max_file_number"] + 1) == store.next_file, name
        assert t["level_files"] == [sum(1 for f in store.files.values() if f[0] == lv) for lv in range(7)]
        assert t["level_bytes"] == [sum(f[1] for f in store.files.values() if f[0] == lv) for lv in range(7)]
        # the rows open as they are, the payload being the bound keys
        images = bytes(store.images)
        tabs = [T.open_host(images[int(r["file_off"]): int(r["file_off"]) + int(r["file_cap"])], handles=False)[0] for r in rows]
        hv = V.HostVersion(np.frombuffer(images, dtype=np.uint8) if images else np.zeros(0, dtype=np.uint8), rows,
                           V.tables_array(tabs), None, np.frombuffer(payload, dtype=np.uint8) if payload else np.zeros(1, dtype=np.uint8),
                           bounds_bytes=len(payload))
        st = hv.open()
        assert st["status"] == 0 and st["level_start"] == store.ver.state["level_start"], (name, st)

    total = SC.life(store, model, 7, per_group=False, checkpoint=checkpoint, checking=False)
    assert not total.mismatches
    names = [s[0] for s in seen]
    assert sum("flush" in n for n in names) == 4 and sum("compaction" in n for n in names) == 3 and "g3 reopen" in names
    assert max(s[2] for s in seen) > 8
