"""lv_version_file_host / lv_version_open_host / lv_version_get_host against the
serial Python model of include/lvgpu/version.h (tests/version_cases.py), the
worked example and its golden file, the union rule against
lv_memtable_get_host, and the argument checks of the three device entry
points.  No GPU."""
import ctypes
import json

import numpy as np
import pytest

import lvgpu
import lvgpu.version as V
import sst_get_cases as G
import version_cases as C
from memtable_cases import MAX_SEQUENCE

INVALID = -1  # LV_ERR_INVALID


def host_file(images, file_off, file_cap, table, number, level, cap, used, images_bytes=None):
    """lv_version_file_host over an exact-size bounds array with a canary
    behind its capacity: (file dict, cursor, bounds bytes)."""
    buf = np.full(cap + 16, 0xA5, dtype=np.uint8)
    img = np.frombuffer(bytes(images), dtype=np.uint8)
    f, used = V.file_host(img, file_off, file_cap, table, number, level, buf, used, bound_cap=cap,
                          images_bytes=len(images) if images_bytes is None else images_bytes)
    assert (buf[cap:] == 0xA5).all(), "lv_version_file_host wrote at or beyond bound_keys_cap"
    return f, used, buf[:cap].tobytes()


def answers(ver, queries, *, bloom=True, version=None):
    """(model results, host results) of one Ver."""
    version = C.model_open(ver) if version is None else version
    h = ver.host(bloom)
    assert h.open() == C.model_open(ver)
    want = [C.model_get(ver, version, k, s, bloom=bloom) for k, s in queries]
    got = [h.get(k, s, version) for k, s in queries]
    for q, g, w in zip(queries, got, want):
        assert g == w, (q, g, w)
    return want, got


def test_symbols_and_constants():
    names = lvgpu.declared_symbols()
    for n in ("lv_version_file_device", "lv_version_open_device", "lv_version_get_device", "lv_version_file_host",
              "lv_version_open_host", "lv_version_get_host"):
        assert n in names, n
    text = open(lvgpu.HEADER_PATH.replace("crc32c.h", "version.h")).read()
    assert "#define LV_NUM_LEVELS 7u" in text and V.NUM_LEVELS == C.NUM_LEVELS == 7
    assert "#define LV_VERSION_MAX_FILES (1u << 20)" in text and V.MAX_FILES == 1 << 20
    import re
    assert {int(v): k for k, v in re.findall(r"#define LV_VERSION_FILE_(\w+)\s+(\d+)u", text)} == V.FILE_STATUS
    assert {int(v): k for k, v in re.findall(r"#define LV_VERSION_OPEN_(\w+)\s+(\d+)u", text)} == V.OPEN_STATUS
    assert "UNPINNED" in text


def test_worked_example():
    """The model, the header's table, the golden file and the host twins agree
    field for field."""
    ver = C.example()
    version = C.model_open(ver)
    assert version == dict(files=5, level_start=[0, 2, 4, 4, 5, 5, 5, 5], first_bad=5, status=0)
    queries = [(k, s) for k, s, *_ in C.EXAMPLE_ANSWERS]
    want, _ = answers(ver, queries)
    for (k, s, status, value, file, level, files_read, seek_file), w in zip(C.EXAMPLE_ANSWERS, want):
        assert (w["status"], w["file"], w["level"], w["files_read"], w["seek_file"]) == \
            (status, file, level, files_read, seek_file), (k, s, w)
        if status == G.FOUND:
            assert ver.images[w["val_off"]:w["val_off"] + w["val_len"]] == value, (k, s, w)
        else:
            assert (w["val_off"], w["val_len"]) == (0, 0)
    # (c,3): a FindFile by user key would have read f2 and answered from it
    assert want[6]["files_read"] == 3 and want[6]["status"] == G.ABSENT
    gver, gversion, gq = C.load_golden()
    assert json.loads(json.dumps(C.golden_dict())) == json.load(open(C.GOLDEN)), \
        "tests/golden/version_get_example.json is stale: python tests/version_cases.py golden"
    assert gversion == version and gver.images == ver.images and gver.bounds == ver.bounds and gver.files == ver.files
    h, h0 = gver.host(True), gver.host(False)
    assert h.open() == gversion
    for (k, s, with_f, without_f), w in zip(gq, want):
        assert with_f == w and h.get(k, s) == with_f and h0.get(k, s) == without_f, (k, s)
    answers(ver, queries, bloom=False)
    C.check_union(ver, queries, want)


@pytest.mark.parametrize("name", sorted(C.shapes()))
def test_shapes(name):
    ver = C.shapes()[name]
    queries = C.queries_for(ver)
    for bloom in (True, False):
        want, _ = answers(ver, queries, bloom=bloom)
        if name != "number_decides":  # (not a consistent version, on purpose)
            C.check_union(ver, queries, want)
    seen = {w["status"] for w in want}
    if ver.files:
        assert {G.FOUND, G.ABSENT, G.BAD_SEQ} <= seen, seen
    else:
        assert seen == {G.ABSENT} and C.model_open(ver)["status"] == 0


def test_one_l0_file_equals_sst_get():
    import lvgpu.table as T
    ver = C.shapes()["one_l0"]
    f, t = ver.files[0], ver.tables[0]
    image = ver.images[f["file_off"]:f["file_off"] + t["file_bytes"]]
    h = ver.host(False)
    for k, s in C.queries_for(ver):
        r, g = h.get(k, s), T.get_host(image, t, k, s)
        assert (r["status"], r["tag"], r["val_len"], r["block"]) == (g["status"], g["tag"], g["val_len"], g["block"])
        assert r["val_off"] == (g["val_off"] + f["file_off"] if g["status"] == G.FOUND else 0)
        searched = g["status"] not in (G.BAD_SEQ,) and t["file_bytes"] and \
            ver.bounds[f["smallest_off"]:f["smallest_off"] + f["smallest_len"] - 8] <= k <= \
            ver.bounds[f["largest_off"]:f["largest_off"] + f["largest_len"] - 8]
        assert r["files_read"] == (1 if searched else 0) and r["seek_file"] == 0


def test_number_decides_not_sequence():
    ver = C.shapes()["number_decides"]
    r = ver.host().get(b"k", MAX_SEQUENCE)
    assert r["status"] == G.FOUND and r["file"] == 0 and r["tag"] >> 8 == 3
    assert ver.images[r["val_off"]:r["val_off"] + r["val_len"]] == b"old-in-new-file"


def test_filters_are_asked():
    """Absent keys inside a file's range are stopped by its filter: filtered
    counts them and they still count as read."""
    ver = C.shapes()["many_small_blocks"]
    h = ver.host()
    absent = [(b"%05d" % i + b"x", MAX_SEQUENCE) for i in range(25, 75)]
    res = [h.get(k, s) for k, s in absent]
    assert all(r["status"] == G.ABSENT and r["files_read"] in (1, 2) for r in res)  # ("00049x" lies between two L1 files)
    reads = sum(r["files_read"] for r in res)
    assert reads >= 99 and sum(r["filtered"] for r in res) >= 0.9 * reads  # about 99 % at 10 bits per key
    assert all(r["filtered"] == 0 for r in [ver.host(False).get(k, s) for k, s in absent])


@pytest.mark.parametrize("seed", range(40))
def test_second_opinion_random_versions(seed):
    """Versions a simulated op stream leaves behind: the host twins equal the
    model, and every answer equals lv_memtable_get_host's over the union of all
    files' entries, with and without filters."""
    ver = C.random_version(seed, bpk=10 if seed % 3 else None)
    queries = C.queries_for(ver)
    if len(queries) > 400:
        queries = queries[::len(queries) // 400 + 1]
    for bloom in (True, False):
        want, _ = answers(ver, queries, bloom=bloom)
        C.check_union(ver, queries, want)


def test_random_versions_cover_the_levels():
    seen_levels, multi = set(), 0
    for seed in range(40):
        ver = C.random_version(seed)
        seen_levels |= {f["level"] for f in ver.files}
        multi += len({f["level"] for f in ver.files}) >= 3
    assert {0, 1, 2, 3} <= seen_levels and multi >= 5, (seen_levels, multi)


@pytest.mark.parametrize("name", sorted(C.open_status_cases()))
def test_open_statuses(name):
    ver, kw, status, first_bad = C.open_status_cases()[name]
    want = C.model_open(ver, **kw)
    assert (want["status"], want["first_bad"]) == (status, first_bad), want
    if status:
        assert want["level_start"] == [0] * 8
    h = V.HostVersion(ver.images, ver.files_array(), ver.tables_array(), ver.blooms_array(), ver.bounds,
                      images_bytes=kw.get("images_bytes"), bounds_bytes=kw.get("bounds_bytes"))
    assert h.open() == want
    for k, s, *_ in C.EXAMPLE_ANSWERS:
        r = h.get(k, s)
        if status:
            assert r == dict(dict.fromkeys(C.GET_FIELDS, 0), status=G.NO_TABLE), (k, s, r)
        else:
            assert r["status"] != G.NO_TABLE


def test_open_status_cases_reach_every_bit():
    seen = 0
    for _, _, status, _ in C.open_status_cases().values():
        seen |= status
    assert seen == C.BAD_FILE | C.BAD_TABLE | C.BAD_BOUND | C.UNSORTED  # UPSTREAM: the device's alone
    assert C.model_open(C.example(), upstream=1) == dict(files=5, level_start=[0] * 8, first_bad=5, status=C.UPSTREAM)


def test_get_refuses_a_version_of_other_arrays():
    """A lv_version_state that does not fit the arrays is NO_TABLE, never a read
    outside them."""
    ver = C.example()
    h = ver.host()
    good = h.open()
    for bad in (dict(good, files=4), dict(good, level_start=[0, 2, 4, 4, 5, 5, 5, 6]),
                dict(good, level_start=[1, 2, 4, 4, 5, 5, 5, 5]), dict(good, level_start=[0, 5, 4, 4, 5, 5, 5, 5]),
                dict(good, level_start=[0, 2, 4, 4, 1 << 40, 5, 5, 5]), dict(good, status=1 << 40)):
        assert bad != good and C.model_get(ver, bad, b"b", 9)["status"] == G.NO_TABLE
        assert h.get(b"b", 9, bad) == dict(dict.fromkeys(C.GET_FIELDS, 0), status=G.NO_TABLE), bad


@pytest.mark.parametrize("name", sorted(C.file_status_cases()))
def test_file_statuses(name):
    images, kw, table, status = C.file_status_cases()[name]
    off, cap = kw.get("file_off", 0), kw.get("file_cap", len(images))
    room = 200
    want_b = bytearray(b"\xa5" * room)
    want, want_used = C.model_file(images, len(images), off, cap, table, 77, 2, want_b, room, 5)
    assert want["status"] == status, want
    got, used, got_b = host_file(images, off, cap, table, 77, 2, room, 5)
    assert (got, used, got_b) == (want, want_used, bytes(want_b))
    if status:
        assert used == 5 and got_b == b"\xa5" * room
        assert all(got[f] == 0 for f in ("smallest_off", "largest_off", "smallest_len", "largest_len"))
    else:
        assert used == 5 + got["smallest_len"] + got["largest_len"]


def test_file_status_cases_reach_every_status():
    assert {c[3] for c in C.file_status_cases().values()} == {0, C.FILE_NO_TABLE, C.FILE_BAD_EXTENT, C.FILE_EMPTY, C.FILE_CORRUPT}


def test_file_bound_over_retry():
    """BOUND_OVER leaves the cursor and the bytes alone and reports the bytes
    needed; one retry with that room succeeds, at every capacity below it."""
    images, _, table, _ = C.file_status_cases()["ok"]
    full, used, keys = host_file(images, 0, len(images), table, 1, 0, 64, 0)
    assert full["status"] == 0 and used == full["smallest_len"] + full["largest_len"]
    need = used
    for start in (0, 3):
        for cap in range(0, start + need):
            f, u, b = host_file(images, 0, len(images), table, 1, 0, cap, start)
            assert f["status"] == C.FILE_BOUND_OVER and f["reserved"] == need and u == start and b == b"\xa5" * cap
        f, u, b = host_file(images, 0, len(images), table, 1, 0, start + need, start)
        assert f["status"] == 0 and u == start + need and b[start:] == keys[:need]
    # a cursor beyond the capacity
    f, u, _ = host_file(images, 0, len(images), table, 1, 0, 10, 11)
    assert f["status"] == C.FILE_BOUND_OVER and u == 11


def test_files_from_the_twin_equal_the_models():
    """Every descriptor of the shapes, made by lv_version_file_host appending
    into one array, is the model's, byte for byte."""
    for name, ver in C.shapes().items():
        used, cap = 0, len(ver.bounds)
        buf = np.full(cap + 8, 0xA5, dtype=np.uint8)
        img = np.frombuffer(ver.images, dtype=np.uint8)
        for f, t in zip(ver.files, ver.tables):
            got, used = V.file_host(img, f["file_off"], f["file_cap"], t, f["number"], f["level"], buf, used, bound_cap=cap)
            assert got == f, (name, got, f)
        assert used == cap and buf[:cap].tobytes() == ver.bounds and (buf[cap:] == 0xA5).all()


def test_corruption_stops_the_search():
    ver, bad = C.corrupt_example()
    assert C.model_open(ver)["status"] == 0
    queries = [(k, s) for k, s, *_ in C.EXAMPLE_ANSWERS]
    want, got = answers(ver, queries)
    by = dict(zip(queries, got))
    r = by[(b"b", 9)]  # f0 is read and absent, f1 is corrupt: the search stops, f2 and f4 are not read
    assert (r["status"], r["file"], r["level"], r["files_read"], r["seek_file"]) == (G.CORRUPT, bad, 0, 2, 1)
    assert (r["val_off"], r["val_len"], r["tag"], r["block"]) == (0, 0, 0, 0)
    assert by[(b"e", MAX_SEQUENCE)]["status"] == G.CORRUPT and by[(b"b", MAX_SEQUENCE)]["status"] == G.FOUND
    # without the filters too; a key f1's filter rules out never touches the block
    answers(ver, queries, bloom=False)


def test_host_twin_argument_checks():
    L = V._bind()
    w = np.zeros(V.VERSION_WORDS, dtype=np.uint64)
    r = np.zeros(1, dtype=V.GET_DTYPE)
    f = np.zeros(1, dtype=V.FILE_DTYPE)
    t = np.zeros(8, dtype=np.uint64)
    cur = ctypes.c_uint64(0)
    assert L.lv_version_open_host(0, None, None, 0, None, 0, None) == INVALID
    assert L.lv_version_open_host(0, None, None, 1, None, 0, w.ctypes.data) == INVALID
    assert L.lv_version_open_host(0, None, None, (1 << 20) + 1, None, 0, w.ctypes.data) == INVALID
    assert L.lv_version_open_host(0, None, None, 0, None, 0, w.ctypes.data) == 0 and w[-1] == 0
    assert L.lv_version_get_host(None, 0, None, None, None, 0, None, 0, w.ctypes.data, None, 0, 1, None) == INVALID
    assert L.lv_version_get_host(None, 0, None, None, None, 0, None, 0, w.ctypes.data, None, 1, 1, r.ctypes.data) == INVALID
    assert L.lv_version_get_host(None, 0, None, None, None, 0, None, 0, w.ctypes.data, None, 0, 1, r.ctypes.data) == 0
    assert int(r[0]["status"]) == G.ABSENT
    assert L.lv_version_file_host(None, 0, 0, 0, t.ctypes.data, 1, 7, None, 0, ctypes.byref(cur), f.ctypes.data) == INVALID
    assert L.lv_version_file_host(None, 0, 0, 0, None, 1, 0, None, 0, ctypes.byref(cur), f.ctypes.data) == INVALID
    assert L.lv_version_file_host(None, 0, 0, 0, t.ctypes.data, 1, 0, None, 0, ctypes.byref(cur), f.ctypes.data) == 0
    assert int(f[0]["status"]) == C.FILE_EMPTY


def test_device_argument_checks():
    """Every argument error of the three device entry points is found on the
    host, before any device call: LV_ERR_INVALID and a message, with pointers
    that are never dereferenced and no GPU in the machine."""
    L = V._bind()
    vp = ctypes.c_void_p
    err = lambda: lvgpu.lib().lv_last_error()

    def file(images=vp(0x100000), nbytes=4096, table=vp(0x200000), level=0, keys=vp(0x300000), cap=64, used=vp(0x400000),
             out=vp(0x500000), flags=0):
        return L.lv_version_file_device(images, nbytes, 0, nbytes, table, 1, level, keys, cap, used, out, flags, None)
    assert file(images=None) == INVALID and b"null d_images" in err()
    assert file(table=None) == INVALID and b"null d_table" in err()
    assert file(keys=None) == INVALID and b"null d_bound_keys" in err()
    assert file(used=None) == INVALID and b"null d_bound_used" in err()
    assert file(out=None) == INVALID and b"null d_out" in err()
    assert file(table=vp(0x200004)) == INVALID and b"d_table must be 8-byte" in err()
    assert file(used=vp(0x400004)) == INVALID and b"d_bound_used must be 8-byte" in err()
    assert file(out=vp(0x500004)) == INVALID and b"d_out must be 8-byte" in err()
    assert file(level=7) == INVALID and b"level" in err()
    assert file(flags=1) == INVALID and b"flag" in err()

    def open_(files=vp(0x100000), tables=vp(0x200000), n=3, keys=vp(0x300000), kb=64, up=None, version=vp(0x500000),
              flags=0):
        return L.lv_version_open_device(4096, files, tables, n, keys, kb, up, version, flags, None)
    assert open_(files=None) == INVALID and b"null d_files" in err()
    assert open_(tables=None) == INVALID and b"null d_tables" in err()
    assert open_(keys=None) == INVALID and b"null d_bound_keys" in err()
    assert open_(version=None) == INVALID and b"null d_version" in err()
    assert open_(files=vp(0x100004)) == INVALID and b"d_files must be 8-byte" in err()
    assert open_(tables=vp(0x200004)) == INVALID and b"d_tables must be 8-byte" in err()
    assert open_(version=vp(0x500004)) == INVALID and b"d_version must be 8-byte" in err()
    assert open_(up=vp(0x600004)) == INVALID and b"d_upstream_status must be 8-byte" in err()
    assert open_(n=(1 << 20) + 1) == INVALID and b"n_files" in err()
    assert open_(flags=2) == INVALID and b"flag" in err()

    def get(images=vp(0x1000000), nbytes=4096, files=vp(0x100000), tables=vp(0x200000), blooms=None, n=3,
            keys=vp(0x300000), kb=64, version=vp(0x500000), qkeys=vp(0x600000), qb=100, off=vp(0x700000),
            ln=vp(0x800000), seq=vp(0x900000), nq=10, res=vp(0xA00000), flags=0):
        return L.lv_version_get_device(images, nbytes, files, tables, blooms, n, keys, kb, version, qkeys, qb, off, ln,
                                       seq, nq, res, flags, None)
    assert get(images=None) == INVALID and b"null d_images" in err()
    assert get(files=None) == INVALID and b"null d_files" in err()
    assert get(tables=None) == INVALID and b"null d_tables" in err()
    assert get(keys=None) == INVALID and b"null d_bound_keys" in err()
    assert get(version=None) == INVALID and b"null d_version" in err()
    assert get(qkeys=None) == INVALID and b"null d_qkeys" in err()
    for a in ("off", "ln", "seq"):
        assert get(**{a: None}) == INVALID and b"null query array" in err(), a
    assert get(res=None) == INVALID and b"null d_results" in err()
    assert get(files=vp(0x100004)) == INVALID and b"d_files must be 8-byte" in err()
    assert get(tables=vp(0x200004)) == INVALID and b"d_tables must be 8-byte" in err()
    assert get(blooms=vp(0xB00004)) == INVALID and b"d_blooms must be 8-byte" in err()
    assert get(version=vp(0x500004)) == INVALID and b"d_version must be 8-byte" in err()
    assert get(off=vp(0x700004)) == INVALID and b"8-byte" in err()
    assert get(seq=vp(0x900004)) == INVALID and b"8-byte" in err()
    assert get(ln=vp(0x800002)) == INVALID and b"d_q_len must be 4-byte" in err()
    assert get(res=vp(0xA00004)) == INVALID and b"d_results must be 8-byte" in err()
    assert get(flags=4) == INVALID and b"flag" in err()
    assert get(nq=0xFFFFFFFF) == INVALID and b"2^32 - 2" in err()
    assert get(n=(1 << 20) + 1) == INVALID and b"n_files" in err()
    # d_results inside / straddling the images, at either end
    assert get(res=vp(0x1000000 + 4088)) == INVALID and b"overlaps" in err()
    assert get(res=vp(0x1000000 - 480 + 8)) == INVALID and b"overlaps" in err()
    # what passes the checks goes on to the device: with no GPU an error of another kind
    import torch
    if not torch.cuda.is_available():
        assert file() not in (0, INVALID)
        assert open_() not in (0, INVALID) and open_(n=0, files=None, tables=None) not in (0, INVALID)
        assert get() not in (0, INVALID) and get(res=vp(0x1000000 - 480)) not in (0, INVALID)
