"""lv_version_file_device / lv_version_open_device / lv_version_get_device on the
GPU against the serial model of tests/version_cases.py, field for field: every
CPU case with the images at byte shifts 0, 1, 5 and 8 inside the arena; query
counts around the wave and the workgroup; file counts around the workgroup and
a level 12 FindFile probes deep; filters on and off; canaries behind d_results
and d_bound_keys; every open and file status; the device chain on one stream
with no synchronisation, and the same chain captured into a graph; descriptors
that were not written for each other; an arena beyond 4 GiB."""
import ctypes
import gc

import numpy as np
import pytest

import lvgpu.memtable as MT
import lvgpu.table as T
import lvgpu.version as V
import memtable_cases as M
import positions64_cases as P
import sst_bloom_cases as B
import sst_get_cases as G
import version_cases as C
from lvgpu import _dev_ptr, _stream_ptr
from memtable_cases import MAX_SEQUENCE, make_table, tag
from write_batch_cases import CANARY, GUARD, tail_is_canary

pytestmark = pytest.mark.gpu

NO_TABLE = dict(dict.fromkeys(C.GET_FIELDS, 0), status=G.NO_TABLE)


@pytest.mark.parametrize("shift", [0, 1, 5, 8])
def test_cases_at_every_shift(gpu, shift):
    """Every shape of the CPU suite, filters on and off."""
    import torch
    seen = set()
    for name, ver in C.shapes(shift).items():
        assert all(f["file_off"] % 16 == shift for f in ver.files)
        queries = C.queries_for(ver)
        for bloom in (True, False):
            seen |= C.check_device(torch, gpu, ver, queries, bloom=bloom, tag_=f"{name} shift {shift} bloom {bloom}")[0]
    assert seen == {G.ABSENT, G.FOUND, G.DELETED, G.BAD_SEQ, G.BAD_QUERY}


def test_worked_example_from_the_golden_file(gpu):
    import torch
    ver, version, gq = C.load_golden()
    d = C.Dev(torch, gpu, ver)
    assert d.opened.sync() == version
    queries = [(k, s) for k, s, _, _ in gq]
    qk, off, ln, sq, _ = G.pack_queries(queries, bad_query=False)
    C.compare_results(d.get(torch, gpu, qk, off, ln, sq), [w for _, _, w, _ in gq], "golden")
    C.compare_results(d.get(torch, gpu, qk, off, ln, sq, bloom=False), [w for _, _, _, w in gq], "golden, no filters")


@pytest.fixture(scope="module")
def leveled():
    """A version with files on four levels and its queries with the model's
    answers, ordered so that neighbouring lanes end on different levels."""
    ver = next(v for v in (C.random_version(s) for s in range(100, 200))
               if len({f["level"] for f in v.files}) >= 4 and len(v.files) >= 8)
    version = C.model_open(ver)
    queries = [q for q in C.queries_for(ver) if q[1] <= MAX_SEQUENCE]
    wants = [C.model_get(ver, version, k, s) for k, s in queries]
    by_level = {}
    for q, w in zip(queries, wants):
        by_level.setdefault((w["status"], w["level"]), []).append((q, w))
    assert len({lv for (st, lv) in by_level if st == G.FOUND}) >= 3
    mixed, groups = [], list(by_level.values())
    for i in range(max(len(g) for g in groups)):
        mixed += [g[i % len(g)] for g in groups]
    return ver, mixed


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 256, 257, 1000])
def test_query_counts(gpu, leveled, nq):
    import torch
    ver, mixed = leveled
    pairs = [mixed[i % len(mixed)] for i in range(nq)]
    d = C.Dev(torch, gpu, ver)
    qk, off, ln, sq, _ = G.pack_queries([q for q, _ in pairs], bad_query=False)
    got = d.get(torch, gpu, qk, off, ln, sq)  # (asserts the canary behind result nq)
    C.compare_results(got, [w for _, w in pairs], f"nq {nq}")
    if nq >= 63:
        assert len({(w["status"], w["level"]) for _, w in pairs[:64]}) >= 4  # one wave, several endings


@pytest.mark.parametrize("n_files", [0, 1, 255, 256, 257, 3000])
def test_file_counts(gpu, n_files):
    """One-entry tables on level 1: the validate grid around a workgroup, and a
    FindFile ceil(log2 3000) = 12 probes deep."""
    import torch
    ver = C.l1_singles(n_files)
    rng = np.random.default_rng(n_files)
    pick = sorted(set(rng.integers(0, max(n_files, 1), size=120).tolist()) | {0, max(n_files - 1, 0)})
    queries = [(b"", MAX_SEQUENCE), (b"key", 5), (b"kez", MAX_SEQUENCE)]
    for i in pick:
        queries += [(b"key%06d" % (2 * i), MAX_SEQUENCE), (b"key%06d" % (2 * i), i + 1), (b"key%06d" % (2 * i), i),
                    (b"key%06d" % (2 * i + 1), MAX_SEQUENCE)]
    for bloom in (True, False):
        seen, d, wants = C.check_device(torch, gpu, ver, queries, bloom=bloom, tag_=f"n_files {n_files}")
    v = d.opened.sync()
    assert v["level_start"] == [0, 0] + [n_files] * 6 and v["first_bad"] == n_files
    if n_files:
        assert G.FOUND in seen and max(w["files_read"] for w in wants) == 1
    # one file out of order among them: found by its own lane alone
    if n_files >= 255:
        bad = ver.copy()
        at = n_files - 2
        bad.files[at], bad.files[at + 1] = bad.files[at + 1], bad.files[at]
        bad.tables[at], bad.tables[at + 1] = bad.tables[at + 1], bad.tables[at]
        d = C.Dev(torch, gpu, bad)
        want = C.model_open(bad)
        assert want["status"] == C.UNSORTED and want["first_bad"] == at + 1
        assert d.opened.sync(check=False) == want


@pytest.mark.parametrize("name", sorted(C.open_status_cases()) + ["upstream"])
def test_open_statuses(gpu, name):
    import torch
    if name == "upstream":
        ver, kw, status, first_bad = C.example(), dict(upstream=3), C.UPSTREAM, 5
    else:
        ver, kw, status, first_bad = C.open_status_cases()[name]
    queries = [(k, s) for k, s, *_ in C.EXAMPLE_ANSWERS]
    _, d, wants = C.check_device(torch, gpu, ver, queries, tag_=name, **kw)
    v = d.opened.sync(check=False)
    assert (v["status"], v["first_bad"]) == (status, first_bad)
    if status:
        assert v["level_start"] == [0] * 8 and all(w == NO_TABLE or w["status"] == G.BAD_QUERY for w in wants)


@pytest.mark.parametrize("name", sorted(C.file_status_cases()))
def test_file_statuses(gpu, name):
    import torch
    images, kw, table, status = C.file_status_cases()[name]
    off, cap = kw.get("file_off", 0), kw.get("file_cap", len(images))
    want_b = bytearray(bytes([CANARY]) * 200)
    want, want_used = C.model_file(images, len(images), off, cap, table, 77, 2, want_b, 200, 5)
    assert want["status"] == status
    got = C.run_file(torch, gpu, images, table, file_off=off, file_cap=cap)
    assert got == (want, want_used, bytes(want_b)), name


def test_file_bound_over_retry(gpu):
    import torch
    images, _, table, _ = C.file_status_cases()["ok"]
    f, used, keys = C.run_file(torch, gpu, images, table, cap=64, used=0)
    need = f["smallest_len"] + f["largest_len"]
    assert f["status"] == 0 and used == need
    for cap in (0, 1, need - 1, need + 2):
        f, used, b = C.run_file(torch, gpu, images, table, cap=cap, used=3)
        assert (f["status"], f["reserved"], used, b) == (C.FILE_BOUND_OVER, need, 3, bytes([CANARY]) * cap), cap
    f, used, b = C.run_file(torch, gpu, images, table, cap=need + 3, used=3)
    assert f["status"] == 0 and used == need + 3 and b[3:] == keys[:need] and b[:3] == bytes([CANARY]) * 3


def test_corruption_stops_the_search(gpu):
    import torch
    ver, bad = C.corrupt_example()
    queries = [(k, s) for k, s, *_ in C.EXAMPLE_ANSWERS]
    for bloom in (True, False):
        seen, _, wants = C.check_device(torch, gpu, ver, queries, bloom=bloom, tag_="corrupt")
        assert G.CORRUPT in seen
    w = wants[1]  # (b,9)
    assert (w["status"], w["file"], w["files_read"], w["seek_file"]) == (G.CORRUPT, bad, 2, 1)


# ---- the device chain ----
def chain_items(seed, sizes=(300, 200, 150)):
    """Three consistent groups of items, oldest first: what goes to level 1,
    to the older and to the newer level-0 file."""
    rng = np.random.default_rng(seed)
    keys = [b"key%03d" % i + b"x" * int(rng.integers(0, 20)) for i in range(80)]
    groups, seq = [], 1
    for n in sizes:
        g = []
        for _ in range(n):
            typ = 0 if rng.random() < 0.2 else 1
            g.append((keys[int(rng.integers(len(keys)))], tag(seq, typ), b"" if typ == 0 else b"value%d" % seq))
            seq += 1
        groups.append(g)
    return groups


def chain_queries(groups, nq):
    qs = []
    for g in groups:
        for key, t, _ in g[::2]:
            qs += [(key, t >> 8), (key, MAX_SEQUENCE), (key, (t >> 8) - 1)]
    qs += [(b"key%03d" % i, MAX_SEQUENCE) for i in range(100)] + [(b"", 3), (b"zzz", MAX_SEQUENCE)]
    return [qs[i % len(qs)] for i in range(nq)]


class Chain:
    """Fixed buffers for: three memtable builds, three lv_sst_build_bloom_device
    calls into one arena, then per image open, bloom open and
    lv_version_file_device, then lv_version_open_device and the get."""
    LEVELS = (1, 0, 0)    # group k -> level, number; d_files order is newest L0, older L0, L1
    NUMBERS = (1, 2, 3)
    SLOT = (2, 1, 0)      # group k -> index into d_files

    def __init__(self, torch, gpu, size, cap, nq, qbytes):
        self.torch, self.gpu, self.cap, self.nq = torch, gpu, cap, nq
        z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device=gpu)
        self.d_pay = [z(size) for _ in range(3)]
        self.d_ops = [z(cap * 32) for _ in range(3)]
        self.d_n = [z(1, torch.int64) for _ in range(3)]
        self.mws = [torch.empty(MT.build_workspace_bytes(cap), dtype=torch.uint8, device=gpu) for _ in range(3)]
        self.sws = [torch.empty(T.build_bloom_workspace_bytes(cap, cap), dtype=torch.uint8, device=gpu) for _ in range(3)]
        self.fcap = (T.bloom_file_bound(size, cap, 10) + 15) & ~15
        self.images_bytes = 3 * self.fcap
        self.arena = torch.full((self.images_bytes + GUARD,), CANARY, dtype=torch.uint8, device=gpu)
        self.handles = [z(2 * (cap + 3), torch.int64) for _ in range(3)]
        self.totals = [z(8, torch.int64) for _ in range(3)]
        self.btotals = [z(4, torch.int64) for _ in range(3)]
        self.tables_t, self.blooms_t, self.files_t = z(24, torch.int64), z(24, torch.int64), z(192)
        self.bcap = 400
        self.bounds_t = torch.full((self.bcap + GUARD,), CANARY, dtype=torch.uint8, device=gpu)
        self.used_t, self.version_t = z(1, torch.int64), z(V.VERSION_WORDS, torch.int64)
        self.d_qk, self.d_off, self.d_len, self.d_seq = z(qbytes), z(nq, torch.int64), z(nq, torch.int32), z(nq, torch.int64)
        self.res = torch.full((nq * 48 + GUARD,), CANARY, dtype=torch.uint8, device=gpu)

    def load(self, groups, packed):
        torch = self.torch
        for k, g in enumerate(groups):
            payload, ops = make_table(g)
            self.d_pay[k].zero_()
            self.d_pay[k][: len(payload)].copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
            self.d_ops[k][: len(ops) * 32].copy_(torch.frombuffer(bytearray(ops.tobytes()), dtype=torch.uint8))
            self.d_n[k].fill_(len(ops))
        qk, off, ln, sq = packed
        self.d_qk.zero_()
        self.d_qk[: len(qk)].copy_(torch.frombuffer(bytearray(qk), dtype=torch.uint8))
        self.d_off.copy_(torch.from_numpy(off.view(np.int64).copy()))
        self.d_len.copy_(torch.from_numpy(np.ascontiguousarray(ln).view(np.int32).copy()))
        self.d_seq.copy_(torch.from_numpy(sq.view(np.int64).copy()))
        self.arena.fill_(CANARY)
        self.bounds_t.fill_(CANARY)
        self.res.fill_(CANARY)

    def run(self, stream=None):
        L = T._bind_bloom()
        bopt = T.BloomOptions(10, 0)
        self.used_t.zero_()
        for k in range(3):
            table = MT.build_device(self.d_pay[k], self.d_ops[k], self.d_n[k], op_cap=self.cap, workspace=self.mws[k],
                                    stream=stream)
            slot = self.SLOT[k]
            off = slot * self.fcap
            image = self.arena[off:off + self.fcap]
            rc = L.lv_sst_build_bloom_device(_dev_ptr(table.payload, "payload"), table.payload.numel(),
                                             _dev_ptr(table.ops_t, "ops"), _dev_ptr(table.order_t, "order"),
                                             _dev_ptr(table.totals, "mt_totals"), self.cap, None, ctypes.byref(bopt),
                                             _dev_ptr(image, "file"), self.fcap, _dev_ptr(self.handles[k], "handles"),
                                             self.cap, _dev_ptr(self.totals[k], "totals"),
                                             _dev_ptr(self.btotals[k], "bloom_totals"), 0, _dev_ptr(self.sws[k], "ws"),
                                             self.sws[k].numel(), _stream_ptr(stream))
            assert rc == 0, L.lv_last_error()
            tab = self.tables_t[8 * slot:8 * slot + 8]
            op = T.open_device(image, self.totals[k][2:3], self.totals[k][7:8], handles=False, table=tab, stream=stream)
            T.bloom_open_device(op, bloom=self.blooms_t[8 * slot:8 * slot + 8], stream=stream)
        for slot in range(3):  # in d_files order, so the boundary keys are appended in it
            k = self.SLOT.index(slot)
            V.file_device(self.arena, self.images_bytes, slot * self.fcap, self.fcap, self.tables_t[8 * slot:8 * slot + 8],
                          self.NUMBERS[k], self.LEVELS[k], self.bounds_t, self.bcap, self.used_t,
                          self.files_t[64 * slot:64 * slot + 64], stream=stream)
        opened = V.open_device(self.arena, self.files_t, self.tables_t, 3, self.bounds_t, blooms_t=self.blooms_t,
                               images_bytes=self.images_bytes, bounds_bytes=self.bcap, version=self.version_t,
                               stream=stream)
        gets = V.get_device(opened, self.d_qk, self.d_off, self.d_len, self.d_seq, nq=self.nq, res=self.res, stream=stream)
        return opened, gets

    def verify(self, groups, queries, opened, what):
        torch = self.torch
        torch.cuda.synchronize()
        items = [groups[self.SLOT.index(slot)] for slot in range(3)]
        ver = C.ver_from_device(torch, opened, items)
        used, bounds = 0, bytearray(bytes([CANARY]) * self.bcap)
        for slot in range(3):
            k = self.SLOT.index(slot)
            payload, ops = make_table(groups[k])
            image = B.model_build(payload, ops, 10)[0]
            off = slot * self.fcap
            assert ver.images[off:off + len(image)] == image, (what, "image", slot)
            assert ver.images[off + len(image):off + self.fcap] == bytes([CANARY]) * (self.fcap - len(image))
            assert ver.tables[slot] == G.model_open(image, handles=False)[0] and ver.blooms[slot]["present"] == 1
            f, used = C.model_file(ver.images, self.images_bytes, off, self.fcap, ver.tables[slot], self.NUMBERS[k],
                                   self.LEVELS[k], bounds, self.bcap, used)
            assert f["status"] == 0 and ver.files[slot] == f, (what, ver.files[slot], f)
        assert ver.bounds == bytes(bounds) and tail_is_canary(self.bounds_t, self.bcap), what
        assert int(self.used_t.cpu()[0]) == used
        version = V.version_dict(self.version_t.cpu().numpy().view(np.uint64))
        assert version == C.model_open(ver) == dict(files=3, level_start=[0, 2] + [3] * 6, first_bad=3, status=0), what
        got = self.res[: self.nq * 48].cpu().numpy().view(V.GET_DTYPE)
        wants = [C.model_get(ver, version, k, s) for k, s in queries]
        seen = C.compare_results(got, wants, what)
        assert tail_is_canary(self.res, self.nq * 48), what
        C.check_union(ver, queries, wants)
        assert {G.FOUND, G.DELETED, G.ABSENT} <= seen and {w["file"] for w in wants if w["status"] == G.FOUND} == {0, 1, 2}
        assert sum(w["filtered"] for w in wants) > 0


def chain_sets(seeds, nq):
    sets = []
    for seed, sizes in seeds:
        groups = chain_items(seed, sizes)
        queries = chain_queries(groups, nq)
        sets.append((groups, queries, M.pack_queries(queries)))
    return sets


def chain_for(torch, gpu, sets, nq):
    size = max(len(make_table(g)[0]) for groups, _, _ in sets for g in groups)
    cap = max(len(g) for groups, _, _ in sets for g in groups)
    return Chain(torch, gpu, size, cap, nq, max(len(p[0]) for _, _, p in sets))


def test_chain_with_no_host_sync(gpu):
    """Three memtable builds, three bloom builds into one arena, open, bloom
    open, lv_version_file_device, lv_version_open_device and the get on one
    stream; one synchronisation at the end."""
    import torch
    nq = 700
    sets = chain_sets([(1, (300, 200, 150))], nq)
    ch = chain_for(torch, gpu, sets, nq)
    groups, queries, packed = sets[0]
    ch.load(groups, packed)
    s = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        opened, _ = ch.run(s)
    s.synchronize()
    ch.verify(groups, queries, opened, "chain")


def test_chain_graph_capture(gpu):
    """The same chain captured into one graph after a warm-up; replays over
    other inputs of one capacity."""
    import torch
    nq = 500
    sets = chain_sets([(2, (200, 150, 100)), (3, (260, 90, 140)), (4, (40, 250, 30))], nq)
    ch = chain_for(torch, gpu, sets, nq)
    ch.load(sets[0][0], sets[0][2])
    opened, _ = ch.run()
    ch.verify(sets[0][0], sets[0][1], opened, "warm")
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            opened, _ = ch.run(s)
    torch.cuda.synchronize()
    for k in (1, 2, 0):
        ch.load(sets[k][0], sets[k][2])
        ch.files_t.fill_(CANARY)
        ch.version_t.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        ch.verify(sets[k][0], sets[k][1], opened, f"replay of set {k}")


# ---- descriptors that were not written for each other ----
def test_mismatched_descriptors_end_clean(gpu):
    """The arrays of one version with the files, tables, filters or
    lv_version_state of another: the run ends clean, every result is the host
    twin's (the same core, which the stand-alone check program runs under a
    sanitizer), and nothing but NO_TABLE, CORRUPT or a lookup's own statuses
    comes out."""
    import torch
    a = C.shapes()["many_small_blocks"]
    b = C.random_version(104)
    ex = C.example()
    assert len(b.files) >= 3
    n = min(len(a.files), len(b.files))
    queries = (C.queries_for(a)[::3] + C.queries_for(b)[::3])[:400]
    qk, off, ln, sq, _ = G.pack_queries(queries, bad_query=False)

    def cut(v, **kw):
        c = v.copy(**kw)
        c.files, c.tables, c.blooms = c.files[:n], c.tables[:n], c.blooms[:n]
        return c
    a3, b3 = cut(a), cut(b)
    mixes = {
        "files_of_b": a3.copy(files=b3.files),
        "tables_of_b": a3.copy(tables=b3.tables),
        "blooms_of_b": a3.copy(blooms=b3.blooms),
        "images_of_b": a3.copy(images=b3.images),
        "bounds_of_b": a3.copy(bounds=b3.bounds),
        "images_of_example": a3.copy(images=ex.images),
        "bounds_of_example": a3.copy(bounds=ex.bounds),
    }
    ok = {G.ABSENT, G.FOUND, G.DELETED, G.BAD_SEQ, G.NO_TABLE, G.CORRUPT}
    seen = set()
    for name, mix in mixes.items():
        h = mix.host()
        opened = h.open()
        d = C.Dev(torch, gpu, mix)
        assert d.opened.sync(check=False) == opened, name
        # the open's own verdict, and a state that claims all is well with a's levels
        forged = C.model_open(a3)
        assert forged["status"] == 0
        for what, state in (("own", opened), ("forged", forged)):
            d.opened.version.copy_(torch.from_numpy(V.version_words(state).view(np.int64).copy()))
            got = d.get(torch, gpu, qk, off, ln, sq)
            for i, (k, s) in enumerate(queries):
                g = {f: int(got[i][f]) for f in C.GET_FIELDS}
                assert g == h.get(k, s, state), (name, what, k, s)
                assert g["status"] in ok
                seen.add(g["status"])
                if g["status"] == G.FOUND:
                    assert g["val_off"] + g["val_len"] <= len(mix.images)
    assert {G.NO_TABLE, G.CORRUPT} <= seen, seen
    # a state of another file count is refused whole
    d = C.Dev(torch, gpu, a)
    d.opened.version.copy_(torch.from_numpy(V.version_words(C.model_open(ex)).view(np.int64).copy()))
    assert len(ex.files) != len(a.files)
    got = d.get(torch, gpu, qk, off, ln, sq)
    assert all({f: int(r[f]) for f in C.GET_FIELDS} == NO_TABLE for r in got)


# ---- an arena beyond 4 GiB ----
def test_arena_beyond_4gib(gpu):
    """The example's arena laid across position 2^32 of a larger one, with the
    arena of a second version (same layout, other values) where a position cut
    to 32 bits would land: every file at or above the line answers with val_off
    above 2^32 and the true bytes."""
    import torch
    ver = C.example()
    other = C.build_version([(lv, num, [(k, t, v.upper()) for k, t, v in items]) for lv, num, items in C.example_specs()])
    assert [(f["file_off"], f["file_cap"]) for f in other.files] == [(f["file_off"], f["file_cap"]) for f in ver.files]
    assert other.images != ver.images and len(other.images) == len(ver.images)
    cut = 5  # f0 lies across the line, inside its first entry; everything else above it
    t, base = P.high_window(torch, gpu, ver.images, cut, other.images)
    opened = None
    try:
        assert base < P.HI < base + len(ver.images)
        high = ver.copy()
        for f in high.files:
            f["file_off"] += base
        images_bytes = base + len(ver.images)
        files_t = M.dev_bytes(torch, gpu, high.files_array())
        tables_t = M.dev_i64(torch, gpu, ver.tables_array().reshape(-1))
        blooms_t = M.dev_i64(torch, gpu, ver.blooms_array().reshape(-1))
        bounds_t = M.dev_bytes(torch, gpu, ver.bounds)
        opened = V.open_device(t, files_t, tables_t, 5, bounds_t, blooms_t=blooms_t, images_bytes=images_bytes,
                               bounds_bytes=len(ver.bounds))
        version = C.model_open(ver)
        assert opened.sync() == version
        queries = [(k, s) for k, s, *_ in C.EXAMPLE_ANSWERS]
        qk, off, ln, sq, _ = G.pack_queries(queries, bad_query=False)
        got = V.get_device(opened, *G.dev_queries(torch, gpu, qk, off, ln, sq), nq=len(queries), fill=CANARY,
                           guard=GUARD).sync()
        above = 0
        for i, (k, s, status, value, *_rest) in enumerate(C.EXAMPLE_ANSWERS):
            want = C.model_get(ver, version, k, s)
            if want["status"] == G.FOUND:
                want["val_off"] += base
            g = {f: int(got[i][f]) for f in C.GET_FIELDS}
            assert g == want, (k, s, g, want)
            if status == G.FOUND:
                assert t[g["val_off"]:g["val_off"] + g["val_len"]].cpu().numpy().tobytes() == value
                assert g["val_off"] > 1 << 32
                above += 1
        assert above == 6
        # lv_version_file_device reads its image there too
        out = torch.zeros(64, dtype=torch.uint8, device=gpu)
        used = torch.zeros(1, dtype=torch.int64, device=gpu)
        keys = torch.full((64,), CANARY, dtype=torch.uint8, device=gpu)
        f3 = high.files[3]
        assert f3["file_off"] > 1 << 32
        V.file_device(t, images_bytes, f3["file_off"], f3["file_cap"], tables_t[24:32], 4, 1, keys, 64, used, out)
        torch.cuda.synchronize()
        f = out.cpu().numpy().view(V.FILE_DTYPE)[0]
        n = int(f["smallest_len"]) + int(f["largest_len"])
        s3 = ver.files[3]
        assert int(f["status"]) == 0 and keys[:n].cpu().numpy().tobytes() == \
            ver.bounds[s3["smallest_off"]:s3["smallest_off"] + n]
    finally:
        t = opened = None
        gc.collect()
        torch.cuda.empty_cache()
