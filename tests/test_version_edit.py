"""The VersionEdit host twins (lv_version_edit_decode_host,
lv_version_edit_encode_host) against the serial model of
tests/version_edit_cases.py, and the model against the known answers: the
worked example of include/lvgpu/version_edit.h
(tests/golden/version_edit_example.json), the one-record quirks and the
reference's own test.  No GPU."""
import ctypes

import numpy as np
import pytest

import lvgpu
import lvgpu.version_edit as VE
import version_edit_cases as C


def _host_equals_model(rec, tag=""):
    st, edit, F, D, P, counts = VE.decode_host(rec)
    m_edit, mF, mD, mP, _, tot = C.decode_batch(rec, [0], [len(rec)])
    assert st == int(m_edit[0]["status"]), (tag, st)
    assert edit.tobytes() == m_edit.tobytes(), (tag, edit, m_edit)
    assert F.tobytes() == mF.tobytes() and D.tobytes() == mD.tobytes() and P.tobytes() == mP.tobytes(), tag
    assert counts == (len(mF), len(mD), len(mP)), tag
    return st, edit[0], F, D, P


def test_the_worked_example():
    g = C.golden()["example"]
    edit = C._from_jsonable(g["edit"])
    assert edit == C.example_edit()
    b = C.encode_to(edit)
    assert b.hex() == g["bytes"] and len(b) == 55
    st, e, F, D, P = _host_equals_model(b)
    assert st == VE.OK and int(e["has"]) == 31 and int(e["flags"]) == 0
    assert [int(e["comparator_off"]), int(e["comparator_len"])] == g["comparator"] == [2, 3]
    assert [int(P[0]["key_off"]), int(P[0]["key_len"])] == g["pointer_key"] == [18, 9]
    assert [int(F[0]["smallest_off"]), int(F[0]["smallest_len"])] == g["smallest"] == [36, 9]
    assert [int(F[0]["largest_off"]), int(F[0]["largest_len"])] == g["largest"] == [46, 9]
    assert (int(e["log_number"]), int(e["prev_log_number"]), int(e["next_file_number"]), int(e["last_sequence"])) == (300, 0, 7, 128)
    assert (int(D[0]["level"]), int(D[0]["number"])) == (2, 9) and int(P[0]["level"]) == 1
    assert (int(F[0]["level"]), int(F[0]["number"]), int(F[0]["file_size"])) == (3, 10, 1000)
    # and back, through the host encoder
    out, ro, rl, tot = VE.encode_host(b, [e], F, [0, 1], D, [0, 1], P, [0, 1])
    assert out == b and list(ro) == [0] and list(rl) == [55]
    assert tot == dict(records=1, files=1, deleted=1, pointers=1, key_bytes=30, out_bytes=55, status=0, bad_record=C.M64,
                       bad_kind=C.M64, bad_row=C.M64)
    # the header shows the same bytes
    with open(lvgpu.HEADER_PATH.replace("crc32c.h", "version_edit.h")) as f:
        text = f.read()
    shown = "".join(c for c in text[text.index("is these 55 bytes:"):text.index("and decodes to the comparator")]
                    if c in "0123456789abcdef ")
    assert "".join(shown.split())[-110:] == b.hex()


def test_the_quirks():
    g = C.golden()["quirks"]
    assert [(q["bytes"], q["status"]) for q in g] == [(h, s) for h, s, _ in C.QUIRKS] and len(g) == 15
    for h, status, extra in C.QUIRKS:
        rec = bytes.fromhex(h)
        st, e, F, D, P = _host_equals_model(rec, h)
        assert st == status, h
        if "comparator" in extra:
            assert (int(e["comparator_off"]), int(e["comparator_len"])) == extra["comparator"]
        if "log_number" in extra:
            assert int(e["log_number"]) == extra["log_number"]
        if "deleted" in extra:
            assert [(int(d["number"]), int(d["level"])) for d in D] == extra["deleted"]
        assert int(e["has"]) == extra.get("has", 0) and int(e["flags"]) == extra.get("flags", 0), h
    assert _host_equals_model(bytes.fromhex("06808080800801"))[1]["flags"] == VE.FLAG_NEG_LEVEL
    assert _host_equals_model(bytes.fromhex("0501037878" + "78"))[1]["flags"] == VE.FLAG_SHORT_KEY


def test_the_references_own_test():
    """version_edit.rs:391-417: each of its five edits re-encodes to the same
    bytes after decode; the final one is the issue's known answer."""
    g = C.golden()["reference_test"]
    edits = C.reference_test_edits()
    assert [C._jsonable(e) for e in edits] == [dict(j, pointers=[tuple(p) for p in j["pointers"]],
                                                    files=[tuple(f) for f in j["files"]]) for j in g["edits"]]
    for e, want in zip(edits, g["bytes"]):
        b = C.encode_to(e)
        assert b.hex() == want
        st, ed, F, D, P = _host_equals_model(b)
        assert st == VE.OK
        assert C.encode_to(C.to_edit(C.decode(b), b)) == b
        out, _, _, tot = VE.encode_host(b, [ed], F, [0, len(F)], D, [0, len(D)], P, [0, len(P)])
        assert out == b and tot["status"] == 0
    assert len(b) == g["final_bytes"] == 288 and C.sha256(b) == g["final_sha256"] == C.REFERENCE_TEST_SHA256


def test_every_status():
    assert sorted(C.STATUS_RECORDS) == list(range(7))
    for status, h in C.STATUS_RECORDS.items():
        assert _host_equals_model(bytes.fromhex(h), h)[0] == status


def test_truncations_and_flips_of_the_example():
    recs = C.damaged_records()
    assert sum(n.startswith("prefix_") for n, _ in recs) == 55 and sum(n.startswith("flip_") for n, _ in recs) == 4 * 55
    seen = set()
    for name, rec in recs:
        seen.add(_host_equals_model(rec, name)[0])
    assert seen == set(range(7))


@pytest.mark.parametrize("seed", range(6))
def test_random_edits_decode_and_encode(seed):
    edits = C.random_edits(seed, 60, max_rows=seed + 2, big=seed % 2 == 1)
    for k, e in enumerate(edits):
        b = C.encode_to(e)
        st, ed, F, D, P = _host_equals_model(b, (seed, k))
        assert st == VE.OK and C.to_edit(C.decode(b), b) == dict(e, deleted=sorted(set(e["deleted"])))
        # random bytes behind a good record: whatever comes, the twin is the model
        _host_equals_model(b + bytes((seed * 31 + k * 7 + i * 13) & 255 for i in range(k % 9)), (seed, k, "tail"))
    t = C.tables_of(edits, lead=(seed, 1, 2))
    out, ro, rl, tot = VE.encode_host(*t)
    mo, mro, mrl, mtot = C.encode_batch(len(t[0]), *t[1:], src=t[0])
    assert tot == mtot and tot["status"] == 0 and out == mo == b"".join(C.encode_to(e) for e in edits)
    assert list(ro) == mro and list(rl) == mrl
    assert tot["out_bytes"] <= VE.encode_bound(tot["records"], tot["pointers"], tot["deleted"], tot["files"], tot["key_bytes"])
    # the decode of the whole batch feeds the encode as it is
    w = C.decode_batch(out, ro, rl)
    again = VE.encode_host(out, w[0], w[1], w[4][0], w[2], w[4][1], w[3], w[4][2])
    assert again[0] == out and again[3]["status"] == 0


def test_the_sizing_mode():
    edits = C.random_edits(77, 30)
    t = C.tables_of(edits)
    full = VE.encode_host(*t)
    out, ro, rl, tot = VE.encode_host(None, *t[1:], sizing=True, src_bytes=len(t[0]))
    assert out is None and tot == full[3] and list(ro) == list(full[1]) and list(rl) == list(full[2])
    # the source is bounds-checked all the same
    assert VE.encode_host(None, *t[1:], sizing=True, src_bytes=len(t[0]) - 1)[3]["status"] == 8
    # OUT_OVER reports the true size, and a retry with it fits
    short = VE.encode_host(*t, out_cap=tot["out_bytes"] - 1)
    assert short[3] == dict(tot, status=16) and short[0] == b""
    assert VE.encode_host(*t, out_cap=short[3]["out_bytes"])[0] == full[0]


def test_refused_inputs():
    seen = set()
    for name, t, _, _ in C.damaged_encode_inputs():
        out, _, _, tot = VE.encode_host(*t)
        want = C.encode_batch(len(t[0]), *t[1:], src=t[0])[3]
        assert tot == want and tot["status"] in (4, 8), name
        seen.add((tot["status"], tot["bad_kind"]))
    assert seen == {(4, 1), (4, 2), (4, 3), (8, 0), (8, 1), (8, 2), (8, 3)}
    # a level of 7 in a deleted row; a deleted row below its predecessor
    t = list(C.tables_of([C.new_edit(deleted=[(1, 5), (1, 6)])]))
    t[4] = t[4].copy()
    t[4][1]["number"] = 4
    assert VE.encode_host(*t)[3] == C.encode_batch(len(t[0]), *t[1:])[3]
    t[4][1]["number"], t[4][1]["level"] = 6, 7
    got = VE.encode_host(*t)[3]
    assert got == C.encode_batch(len(t[0]), *t[1:])[3] and (got["status"], got["bad_kind"], got["bad_row"]) == (8, 2, 1)


def test_argument_errors():
    L = VE._bind()
    i, o, tot = VE.EncodeIn(), VE.EncodeOut(), VE.EncodeTotals()
    one = (ctypes.c_uint64 * 2)(0, 0)
    p = ctypes.addressof(one)
    assert L.lv_version_edit_encode_host(None, 0, None, 0, ctypes.byref(o)) == -1
    assert L.lv_version_edit_encode_host(None, 0, ctypes.byref(i), 0, None) == -1
    assert L.lv_version_edit_encode_host(None, 0, ctypes.byref(i), 0, ctypes.byref(o)) == -1  # no totals
    o.d_totals = ctypes.addressof(tot)
    assert L.lv_version_edit_encode_host(None, 0, ctypes.byref(i), 0, ctypes.byref(o)) == -1  # no bounds
    i.d_rec_file = i.d_rec_deleted = i.d_rec_pointer = p
    assert L.lv_version_edit_encode_host(None, 0, ctypes.byref(i), 0, ctypes.byref(o)) == 0 and tot.status == 0
    assert L.lv_version_edit_encode_host(None, 0, ctypes.byref(i), 1, ctypes.byref(o)) == -1  # records without arrays
    i.file_cap = 1
    assert L.lv_version_edit_encode_host(None, 0, ctypes.byref(i), 0, ctypes.byref(o)) == -1  # a capacity without a table
    i.file_cap = 0
    o.out_cap = 1
    assert L.lv_version_edit_encode_host(None, 0, ctypes.byref(i), 0, ctypes.byref(o)) == -1  # out_cap without d_out
    o.out_cap = 0
    i.deleted_cap, i.d_deleted = (1 << 30) + 1, p
    assert L.lv_version_edit_encode_host(None, 0, ctypes.byref(i), 0, ctypes.byref(o)) == -1
    assert VE.encode_workspace_bytes(1, 1 << 30, 0, 0) > 0 and VE.encode_workspace_bytes(1, (1 << 30) + 1, 0, 0) == 0
    assert VE.encode_workspace_bytes(VE.MAX_REC_CAP + 1, 0, 0, 0) == 0
    # the workspaces grow with the capacities: 64 + 24 bytes per record, 24 + 48 per tile in 16-B aligned
    # regions (24 -> 32, 48 -> 48 for one tile; 48 and 96 for two); 8 bytes per slot in whole tiles
    assert VE.decode_workspace_bytes(2 * VE.VD_TILE) - VE.decode_workspace_bytes(VE.VD_TILE) == VE.VD_TILE * 88 + 16 + 48
    a, b = VE.encode_workspace_bytes(10, 0, 0, 0), VE.encode_workspace_bytes(10, 0, VE.VE_TILE, 0)
    assert b - a == VE.VE_TILE * 8 + 2 * 16  # one more tile: 8 bytes in each of two 16-B aligned columns
    # the device entry points refuse before they touch a GPU
    vp = ctypes.c_void_p
    fake = vp(0x1000)
    d = VE.DecodeOut()
    assert L.lv_version_edit_decode_device(fake, 8, fake, fake, fake, None, 1, None, 0, fake, 1 << 20, None) == -1
    assert L.lv_version_edit_decode_device(fake, 8, fake, fake, fake, None, 1, ctypes.byref(d), 0, fake, 1 << 20, None) == -1
    assert b"d_totals" in lvgpu.lib().lv_last_error()
    d.d_totals = d.d_edits = d.d_rec_file = d.d_rec_deleted = d.d_rec_pointer = 0x1000
    assert L.lv_version_edit_decode_device(fake, 8, fake, fake, fake, None, 1, ctypes.byref(d), 1, fake, 1 << 20, None) == -1
    assert b"flag" in lvgpu.lib().lv_last_error()
    assert L.lv_version_edit_decode_device(fake, 8, fake, fake, fake, None, 1, ctypes.byref(d), 0, fake, 16, None) == -1
    assert b"workspace" in lvgpu.lib().lv_last_error()
    d.d_files, d.file_cap = 0x1008, 1
    assert L.lv_version_edit_decode_device(fake, 8, fake, fake, fake, None, 1, ctypes.byref(d), 0, fake, 1 << 20, None) == -1
    assert b"aligned" in lvgpu.lib().lv_last_error()
    assert L.lv_version_edit_files_device(fake, fake, None, 1, fake, None, fake, None) == -1
    assert L.lv_version_edit_files_device(fake, fake, fake, 1, vp(0x1008), None, fake, None) == -1
