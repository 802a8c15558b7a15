"""lv_sst_open_host / lv_sst_get_host (include/lvgpu/table.h, "Open" and
"Get") against the Python model of sst_get_cases.py, the model against
sst_build_cases.index_seek, and the table get against lv_memtable_get_host on
the same op table.  No GPU."""
import ctypes

import numpy as np
import pytest

import lvgpu.memtable as MT
import lvgpu.table as T
import memtable_cases as M
import sst_build_cases as S
import sst_get_cases as G
from memtable_cases import MAX_SEQUENCE, make_table, tag

CASES = S.cases()


def open_both(image, **kw):
    """open_host against model_open: the table dict and the handles."""
    want_t, want_h = G.model_open(image, **kw)
    got_t, got_h = T.open_host(image, **kw)
    assert got_t == want_t, (got_t, want_t)
    if not kw.get("handles", True):
        assert got_h == []
    elif want_h is None:
        assert (got_h == G.HANDLE_CANARY).all(), "handles written on a status"
    else:
        assert got_h == want_h
    return got_t, want_h


def get_both(image, table, queries, tag_=""):
    seen = {}
    for key, seq in queries:
        want = G.model_get(image, table, key, seq)
        got = T.get_host(image, table, key, seq)
        assert got == want, (tag_, key[:40], seq, got, want)
        seen[(key, seq)] = got
    return seen


def check_table(items, bs, ri, tag_=""):
    payload, ops = make_table(items)
    image, handles, _ = S.model_build(payload, ops, bs, ri)
    table, got_h = open_both(image)
    assert got_h == handles
    order, mt = MT.build_host(payload, ops)
    _, host_h, _ = T.build_host(payload, ops, order, mt, bs, ri)
    assert host_h == handles
    queries = G.queries_for(image, payload, ops)
    res = get_both(image, table, queries, tag_)
    index, blocks = S.read_table(image)[1:] if image else ([], [])
    for (key, seq), r in res.items():
        if seq > MAX_SEQUENCE:
            assert r["status"] == G.BAD_SEQ
            continue
        # the independent reader of the build's tests
        hit = S.index_seek(index, blocks, S.ikey(key, tag(seq, 1)))
        if hit is None or hit[0][:-8] != key:
            assert r["status"] == G.ABSENT, (tag_, key, seq, r, hit)
        else:
            assert r["status"] == (G.FOUND if hit[0][-8] == 1 else G.DELETED) and \
                r["tag"] == int.from_bytes(hit[0][-8:], "little"), (tag_, key, seq, r, hit)
            if r["status"] == G.FOUND:
                assert image[r["val_off"]:r["val_off"] + r["val_len"]] == hit[1]
        # the memtable over the same ops
        m = MT.get_host(payload, ops, order, mt, key, seq)
        assert m["status"] == r["status"], (tag_, key, seq, m, r)
        if m["status"] in (G.FOUND, G.DELETED):
            assert int(ops[m["op"]]["tag"]) == r["tag"]
            assert payload[m["val_off"]:m["val_off"] + m["val_len"]] == image[r["val_off"]:r["val_off"] + r["val_len"]]
    return image, table


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_as_given_and_one_entry_per_block(name):
    items, bs, ri = CASES[name]
    check_table(items, bs, ri, name)
    check_table(items, 1, 1, name + "/1,1")


def test_shortened_separators_are_absent():
    items, _, _ = CASES["sep_shortened"]
    payload, ops = make_table(items)
    image, _, _ = S.model_build(payload, ops, 1, 16)
    table, _ = open_both(image)
    seps = [k for k, _ in S.read_table(image)[1]]
    assert S.ikey(b"abd", int.from_bytes(S.MAXTAG, "little")) in seps
    assert T.get_host(image, table, b"abd", MAX_SEQUENCE)["status"] == G.ABSENT


def test_versions_across_a_block_boundary():
    items = [(b"same", tag(s), b"v%d" % s) for s in range(2, 40, 3)] + [(b"same", tag(20, 0), b"")]
    payload, ops = make_table(items)
    image, handles, _ = S.model_build(payload, ops, 1, 16)
    assert len(handles) == len(items) + 2
    table, _ = open_both(image)
    res = get_both(image, table, [(b"same", s) for s in range(0, 45)])
    assert res[(b"same", 1)]["status"] == G.ABSENT
    assert res[(b"same", 20)]["status"] == G.FOUND and res[(b"same", 20)]["tag"] == tag(20)
    assert res[(b"same", 21)]["tag"] == tag(20) and res[(b"same", 19)]["tag"] == tag(17)
    assert len({r["block"] for r in res.values()}) > 10


@pytest.mark.parametrize("ri", [1, 2, 16, 1024])
def test_restart_intervals(ri):
    rng = np.random.default_rng(ri)
    check_table(M.random_items(rng, 200, alphabet=3, maxlen=10, seqs=8), 300, ri, f"ri{ri}")


@pytest.mark.parametrize("name", ["tag_into_key", "tag_high_byte"])
@pytest.mark.parametrize("opt", [(4096, 16), (4096, 1), (1, 16)])
def test_prefix_across_the_key_tag_edge(name, opt):
    items, _, _ = CASES[name]
    payload, ops = make_table(items)
    image, _, _ = S.model_build(payload, ops, *opt)
    table, _ = open_both(image)
    seqs = sorted({t >> 8 for _, t, _ in items})
    between = sorted({s + d for s in seqs for d in (-1, 0, 1) if 0 <= s + d <= MAX_SEQUENCE} | {0, MAX_SEQUENCE})
    keys = sorted({k for k, _, _ in items})
    keys += [k + b"\x00" for k in keys] + [k[:-1] for k in keys] + [k + b"\x01" for k in keys]
    res = get_both(image, table, [(k, s) for k in keys for s in between], name)
    assert {r["status"] for r in res.values()} >= {G.ABSENT, G.FOUND}


def test_long_shared_stem():
    stem = bytes(range(256)) * 20
    stem = stem[:4999]
    items = [(stem + bytes([c]), tag(10 + c), b"v%d" % c) for c in range(1, 40)]
    items += [(stem, tag(5), b"stem"), (stem[:-1], tag(6, 0), b"")]
    for opt in ((4096, 16), (1 << 20, 16), (1 << 20, 1024)):
        payload, ops = make_table(items)
        image, _, _ = S.model_build(payload, ops, *opt)
        table, _ = open_both(image)
        qs = [(k, s) for k, t, _ in items for s in ((t >> 8) - 1, t >> 8, MAX_SEQUENCE)]
        qs += [(stem + b"\x00", 99), (stem + b"\x28\x00", 99), (stem[:2500] + b"\xff" + stem[2501:], 99)]
        res = get_both(image, table, qs, str(opt))
        assert res[(stem + b"\x07", MAX_SEQUENCE)]["status"] == G.FOUND
        assert len(qs[0][0]) == 5000


OPEN_CASES = G.open_cases()


@pytest.mark.parametrize("name", sorted(OPEN_CASES))
def test_open_statuses(name):
    image, kw, status = OPEN_CASES[name]
    table, _ = open_both(image, **kw)
    assert table["status"] == status, (name, table)
    if name == "handle_over":
        assert table["data_blocks"] == kw["block_cap"] + 1
    _, _, base, _ = G.base_image()
    payload, ops, _, _ = G.base_image()
    for (key, seq), r in get_both(image, table, G.queries_for(base, payload, ops)[:60], name).items():
        if status:
            assert r["status"] == G.NO_TABLE
        elif not image:
            assert r["status"] in (G.ABSENT, G.BAD_SEQ)


def test_file_bytes_beyond_file_cap_is_the_models():
    """The host twin takes no file_cap: the rule is the device's, and the
    model's for it."""
    _, _, image, _ = G.base_image()
    t, h = G.model_open(image, file_cap=len(image) - 1)
    assert t["status"] == G.NOT_A_TABLE and h is None


GET_CASES = G.get_corruption_cases()


@pytest.mark.parametrize("name", sorted(GET_CASES))
def test_get_corruption(name):
    image, queries, must = GET_CASES[name]
    table, _ = open_both(image)
    assert table["status"] == (G.BAD_INDEX if name == "index_handles" else 0)
    table = G.get_table(name, image)  # index_handles: the open refuses it, the gets go by a table it did not write
    res = get_both(image, table, queries, name)
    seen = {r["status"] for r in res.values()}
    assert (G.CORRUPT in seen) == must, (name, seen)
    if name == "good":
        assert seen == {G.ABSENT, G.FOUND}
    if name == "varint_5_bytes_high_bits":  # the bits beyond 2^32 are dropped: the sound block's answers
        good = get_both(GET_CASES["good"][0], G.model_open(GET_CASES["good"][0])[0], queries)
        assert [r["status"] for r in res.values()] == [r["status"] for r in good.values()]


def test_random_flips_in_data_blocks():
    items, bs, ri = CASES["random_small_blocks"]
    payload, ops = make_table(items)
    image, handles, _ = S.model_build(payload, ops, bs, ri)
    queries = G.queries_for(image, payload, ops)[::7]
    rng = np.random.default_rng(77)
    seen = set()
    for i, bad in enumerate(G.flips(image, rng, 500, 0, handles[-3][0] + handles[-3][1] + 5)):
        table, _ = open_both(bad)
        assert table["status"] == 0
        seen |= {r["status"] for r in get_both(bad, table, queries, f"flip{i}").values()}
    assert G.CORRUPT in seen and G.FOUND in seen


def test_foreign_table_never_reads_outside_the_file():
    """A table dict that the open did not write for this image: every result
    is the model's (the sanitizer build of tools/sst_get_host_check.cc is where
    a read outside would show)."""
    _, _, image, _ = G.base_image()
    table = G.model_open(image)[0]
    for patch in (dict(index_offset=len(image)), dict(index_size=1 << 40), dict(index_offset=(1 << 64) - 3),
                  dict(index_offset=0, index_size=table["index_offset"]), dict(file_bytes=len(image) - 48)):
        get_both(image, dict(table, **patch), [(b"0005", 200), (b"", 0), (b"9", 5)], str(patch))


def test_argument_checks_before_any_device_call():
    L = T._bind_get()
    vp = ctypes.c_void_p
    fake, odd = vp(0x1000), vp(0x1004)
    bad_open = [
        ((fake, 64, fake, None, fake, 4, fake, 1, None), b"flag"),
        ((fake, 64, fake, None, fake, 4, None, 0, None), b"d_table"),
        ((fake, 64, fake, None, fake, 4, odd, 0, None), b"aligned"),
        ((fake, 64, None, None, fake, 4, fake, 0, None), b"d_file_bytes"),
        ((fake, 64, odd, None, fake, 4, fake, 0, None), b"aligned"),
        ((fake, 64, fake, odd, fake, 4, fake, 0, None), b"aligned"),
        ((None, 64, fake, None, fake, 4, fake, 0, None), b"d_file"),
        ((fake, 64, fake, None, None, 4, fake, 0, None), b"d_handles"),
        ((fake, 64, fake, None, odd, 4, fake, 0, None), b"aligned"),
        ((fake, 64, fake, None, fake, (1 << 32) - 3, fake, 0, None), b"2^32"),
        ((fake, 64, fake, None, vp(0x1020), 4, fake, 0, None), b"overlaps"),
    ]
    for args, word in bad_open:
        assert L.lv_sst_open_device(*args) == -1, args
        assert word in L.lv_last_error(), (args, L.lv_last_error())
    far = vp(0x100000)
    bad_get = [
        ((fake, 64, far, far, 8, far, far, far, 1, far, 2, None), b"flag"),
        ((fake, 64, None, far, 8, far, far, far, 1, far, 0, None), b"d_table"),
        ((fake, 64, vp(0x100004), far, 8, far, far, far, 1, far, 0, None), b"aligned"),
        ((None, 64, far, far, 8, far, far, far, 1, far, 0, None), b"d_file"),
        ((fake, 64, far, None, 8, far, far, far, 1, far, 0, None), b"d_qkeys"),
        ((fake, 64, far, far, 8, None, far, far, 1, far, 0, None), b"query"),
        ((fake, 64, far, far, 8, far, far, far, 1, None, 0, None), b"d_results"),
        ((fake, 64, far, far, 8, vp(0x100004), far, far, 1, far, 0, None), b"aligned"),
        ((fake, 64, far, far, 8, far, vp(0x100002), far, 1, far, 0, None), b"aligned"),
        ((fake, 64, far, far, 8, far, far, vp(0x100004), 1, far, 0, None), b"aligned"),
        ((fake, 64, far, far, 8, far, far, far, 1, vp(0x100004), 0, None), b"aligned"),
        ((fake, 64, far, far, 8, far, far, far, (1 << 32) - 1, far, 0, None), b"2^32"),
        ((fake, 64, far, far, 8, far, far, far, 1, vp(0x1008), 0, None), b"overlaps"),
    ]
    for args, word in bad_get:
        assert L.lv_sst_get_device(*args) == -1, args
        assert word in L.lv_last_error(), (args, L.lv_last_error())
    # the host twins
    t = T.SstTable()
    r = T.SstGetResult()
    assert L.lv_sst_open_host(None, 48, None, 0, ctypes.byref(t)) == -1
    assert L.lv_sst_open_host(b"x" * 48, 48, None, 1, ctypes.byref(t)) == -1
    assert L.lv_sst_open_host(b"x" * 48, 48, None, 0, None) == -1
    assert L.lv_sst_get_host(None, None, b"k", 1, 0, ctypes.byref(r)) == -1
    assert L.lv_sst_get_host(None, ctypes.byref(t), None, 1, 0, ctypes.byref(r)) == -1
    assert L.lv_sst_get_host(None, ctypes.byref(t), b"k", 1, 0, None) == -1


def test_without_a_gpu_a_well_formed_call_fails_with_the_runtimes_error():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = T._bind_get()
    fake = ctypes.c_void_p(0x1000)
    far = ctypes.c_void_p(0x100000)
    assert L.lv_sst_open_device(fake, 64, far, None, None, 0, far, 0, None) not in (0, -1)
    assert L.lv_last_error()
    assert L.lv_sst_get_device(fake, 64, far, far, 8, far, far, far, 1, far, 0, None) not in (0, -1)
