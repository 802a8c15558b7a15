"""lv_memtable_range_device on the GPU against the DBIter model
(tests/mt_range_cases.py), field for field, with canaries around d_hits and
d_results and in [count, limit) of every slot: every CPU case at payload shifts
0..7, entry counts around the wave with groups across every window boundary, a
group that covers two whole windows, the limit-th hit on the first and last
lane, max_scan around the window, 4 KiB keys, ragged workgroups with every
status mixed into one launch, damaged quadruples, a resume chain that never
leaves the device, a 5,000-entry table, the merged view of two scanned tables,
a compaction filter's output, graph capture, positions beyond 4 GiB."""
import gc

import numpy as np
import pytest

import lvgpu.memtable as MT
import mt_range_cases as C
from memtable_cases import dev_bytes, make_table, tag
from mt_range_cases import BAD_QUERY, BAD_SEQ, BIG, DONE, HAS_HI, M, MORE_LIMIT, MORE_SCAN, NO_TABLE, RESUME, SEEN
from write_batch_cases import CANARY, GUARD, tail_is_canary

pytestmark = pytest.mark.gpu

CASES = C.cpu_cases()


def statuses(wants):
    return {r["status"] for _, r in wants}


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_cases_at_every_shift(gpu, name):
    import torch
    items, settings = CASES[name]
    payload, ops, order, totals = C.table_of(items, gaps=[(3 * i) % 7 for i in range(len(items))])
    for shift in range(8):
        for k, (queries, limit, max_scan) in enumerate(settings):
            if name.startswith("random") and k != shift % len(settings):
                continue  # every setting at two shifts, every shift with a setting
            C.check_device(torch, gpu, payload, ops, order, totals, queries, limit, max_scan, shift=shift,
                           tag_=(name, shift, k))


def test_worked_example_on_the_device(gpu):
    """The header's table, one launch per row, against the golden file itself."""
    import torch
    g = C.golden()
    payload, ops, order, totals = C.table_of(C.golden_table(g))
    table, _ = C.device_table(torch, gpu, payload, ops, order, totals)
    names = {"DONE": DONE, "MORE_LIMIT": MORE_LIMIT, "MORE_SCAN": MORE_SCAN}
    for q in g["queries"]:
        qkeys, rows = C.pack([C.golden_query(q)])
        hits, res = C.run_device(torch, gpu, table, rows, qkeys, 4, q.get("max_scan", BIG))
        want = dict(seek_pos=q["seek_pos"], next_pos=q["next_pos"], unparsed=q["unparsed"], count=q["count"],
                    status=names[q["status"]], seen=q["seen"], reserved=0)
        C.compare(hits, res, [(q["hits"], want)], 4, q)


def window_queries(items, n):
    """Whole walks, walks from and up to the entries around every multiple of
    64, and resumes at those positions with both carried states."""
    keys = [k for k, _, _ in items]
    qs = []
    for s in (0, 12, 16, M):
        qs.append((b"", None, s))
        for at in (62, 63, 64, 65, 127, 128):
            if at < n:
                qs += [(keys[at], None, s), (b"", keys[at], s), (keys[at], keys[at], s), (keys[at], keys[0], s)]
                qs += [("resume", at, seen, None, s) for seen in (0, 1)]
    qs += [("resume", n, 1, None, M), ("resume", 0, 1, None, M), (b"\xff", None, M), (b"", b"", M)]
    return qs


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129, 200])
def test_entry_counts_and_window_boundaries(gpu, n):
    """A group of 7 versions lies across every multiple of 64 (led by a value,
    a deletion or a type-2 entry); limit 1, 64 and 65 and max_scan 1, 63, 64
    and 65 cut the walk at and around a window's edge."""
    import torch
    items = C.boundary_items(n)
    payload, ops, order, totals = C.table_of(items)
    assert order.tolist() == list(range(n))  # the boundaries are where the generator put them
    if n > 70:
        assert items[61][0] == items[67][0] != items[68][0] and items[60][0] != items[61][0]
    table, _ = C.device_table(torch, gpu, payload, ops, order, totals, shift=n % 8)
    queries = window_queries(items, n)
    seen = set()
    for limit, max_scan in ((BIG, BIG), (1, BIG), (64, BIG), (65, BIG), (BIG, 1), (BIG, 63), (BIG, 64), (BIG, 65), (3, 5)):
        seen |= statuses(C.check_device(torch, gpu, payload, ops, order, totals, queries, limit, max_scan, table=table,
                                        tag_=(n, limit, max_scan)))
    assert seen == ({DONE} if n == 0 else {DONE, MORE_LIMIT} if n == 1 else {DONE, MORE_LIMIT, MORE_SCAN})


def test_a_group_over_two_whole_windows(gpu):
    """130 versions of one key in positions 0..129: with the snapshot above
    them the carried `seen` is 1 across both windows, inside them 0 then 1,
    below them 0 and 0; a deletion inside hides the rest."""
    import torch
    items = C.long_group_items()
    payload, ops, order, totals = C.table_of(items)
    assert order.tolist() == list(range(170))
    table, _ = C.device_table(torch, gpu, payload, ops, order, totals, shift=3)
    queries = [(b"", None, s) for s in (M, 130, 129, 101, 100, 99, 66, 65, 64, 2, 1, 0)]
    queries += [(b"g", b"h", s) for s in (M, 65, 0)] + [(b"g", b"g\x00", 65), (b"", b"h0001", 65)]
    queries += [("resume", p, seen, None, s) for p in (1, 63, 64, 65, 128, 129, 130) for seen in (0, 1) for s in (M, 65, 0)]
    for limit, max_scan in ((BIG, BIG), (1, BIG), (2, BIG), (BIG, 64), (BIG, 128), (BIG, 129), (BIG, 130)):
        wants = C.check_device(torch, gpu, payload, ops, order, totals, queries, limit, max_scan, table=table,
                               tag_=(limit, max_scan))
        if (limit, max_scan) == (BIG, BIG):
            assert wants[0][0][0] == 0 and wants[7][0][0] == 65 and wants[11][0] == []  # g@130, g@65, nothing at 0
            assert wants[4][0][0] == 130  # the deletion at 100 hides g@99 and below: h0000 comes first
        if (limit, max_scan) == (BIG, 128):
            assert [wants[i][1]["seen"] for i in (0, 7, 11)] == [1, 1, 0] and wants[0][1]["status"] == MORE_SCAN


@pytest.mark.parametrize("hidden", [0, 63, 64])
def test_the_limit_th_hit_on_the_first_and_last_lane(gpu, hidden):
    """Every entry behind `hidden` deleted versions is a hit: the limit-th
    lands on lane 0 (limit 1, 65), lane 63 (limit 64, or limit 1 behind 63
    hidden entries) and the first lane of a second window."""
    import torch
    items = (C.run_of(b"a", range(1, hidden + 1), typ=lambda s: 0 if s == hidden else 1) if hidden else []) + \
        C.singles(b"s", 200)
    payload, ops, order, totals = C.table_of(items)
    assert order.tolist() == list(range(hidden + 200))
    table, _ = C.device_table(torch, gpu, payload, ops, order, totals)
    queries = [(b"", None, M), (b"s0001", None, M), (b"", b"s0100", M), ("resume", 1, 0, None, M), (b"", None, 4)]
    for limit in (1, 2, 63, 64, 65, 127, 128, 129):
        wants = C.check_device(torch, gpu, payload, ops, order, totals, queries, limit, BIG, table=table, tag_=limit)
        hits, r = wants[0]
        assert r["status"] == MORE_LIMIT and r["next_pos"] == hidden + limit and hits[-1] == hidden + limit - 1


def test_special_and_big_keys(gpu):
    """Type-2 entries at a group start and between a deletion and the value it
    hides; two 4 KiB keys that differ in the last byte only."""
    import torch
    sp = C.special_items()
    payload, ops, order, totals = C.table_of(sp)
    wants = C.check_device(torch, gpu, payload, ops, order, totals, [(b"", None, M), (b"k", b"l", M), (b"l", b"m", M)],
                           BIG, BIG)
    assert wants[1] == ([], dict(seek_pos=0, next_pos=4, unparsed=2, count=0, status=DONE, seen=1, reserved=0))
    assert wants[2][1]["unparsed"] == 2 and wants[2][1]["seen"] == 0 and wants[0][0] == [7, 11]  # m8, o1
    bk, big = C.big_key_items()
    payload, ops, order, totals = C.table_of(bk)
    qs = [(big + b"\x01", big + b"\x02", M), (big + b"\x02", None, 4), (big + b"\x02", None, M), (big, big + b"\x01", M)]
    for shift in (0, 1, 7):
        wants = C.check_device(torch, gpu, payload, ops, order, totals, qs, BIG, BIG, shift=shift)
        assert [w[0] for w in wants] == [[0], [3, 5], [5], [4]]


def mixed_queries(items, nq, rng):
    """nq rows over `items`: seeks and resumes, and among them rows of every
    refusal: BAD_SEQ, unknown flags, SEEN alone, extents outside the keys."""
    qs = C.queries_over(items, [0, 7, 20, M], rng, some=nq)
    qs = (qs * (nq // len(qs) + 1))[:nq]
    qkeys, rows = C.pack(qs)
    for i in range(nq):
        if i % 7 == 3:
            rows[i]["seq"] = M + 1 + i
        elif i % 11 == 5:
            rows[i]["flags"] |= 8
        elif i % 13 == 6:
            rows[i]["flags"] = SEEN
        elif i % 17 == 8:
            rows[i]["lo_off"] = len(qkeys) - 1
            rows[i]["lo_len"] = 2
        elif i % 19 == 9:
            rows[i]["flags"], rows[i]["hi_off"], rows[i]["hi_len"] = HAS_HI, (1 << 64) - 1, 1
        elif i % 23 == 10:
            rows[i]["flags"], rows[i]["pos"] = RESUME | SEEN, 1 + i % 150
    return qkeys, rows


@pytest.mark.parametrize("nq", [1, 3, 4, 5, 1025])
def test_query_counts_with_every_status_in_one_launch(gpu, nq):
    """Ragged workgroups (four waves, one query each), and a wave's refused
    query does not disturb its neighbours."""
    import torch
    rng = np.random.default_rng(nq)
    items = C.random_items(rng, 200)
    payload, ops, order, totals = C.table_of(items)
    qkeys, rows = mixed_queries(items, nq, rng)
    if nq <= 5:  # the refused query is each wave of the workgroup in turn
        for bad in range(nq):
            r2 = rows.copy()
            r2[bad]["seq"] = M + 1
            wants = C.check_device(torch, gpu, payload, ops, order, totals, (qkeys, r2), 2, 50, tag_=(nq, bad))
            assert wants[bad][1]["status"] == BAD_SEQ
    else:
        wants = C.check_device(torch, gpu, payload, ops, order, totals, (qkeys, rows), 2, 50, shift=5, tag_=nq)
        assert statuses(wants) == {DONE, MORE_LIMIT, MORE_SCAN, BAD_SEQ, BAD_QUERY}


def test_no_table(gpu):
    """A build status, entries > op_cap: every query NO_TABLE before BAD_SEQ
    and BAD_QUERY, every slot untouched."""
    import torch
    rng = np.random.default_rng(9)
    items = C.random_items(rng, 100)
    payload, ops, order, totals = C.table_of(items)
    qkeys, rows = mixed_queries(items, 40, rng)
    for tot, cap in ((dict(totals, status=4), None), (dict(totals, status=1 << 33), None), (dict(totals, entries=101), None),
                     (totals, 99)):
        table, _ = C.device_table(torch, gpu, payload, ops, order, tot)
        if cap is not None:
            table.op_cap = cap
        hits, res = C.run_device(torch, gpu, table, rows, qkeys, 5, BIG)
        C.compare(hits, res, [C._status_only(NO_TABLE)] * 40, 5, (tot, cap))
    # the empty table with null ops and order
    table, _ = C.device_table(torch, gpu, b"", ops[:0], order[:0], dict(entries=0, user_keys=0, status=0))
    table.op_cap = 0
    hits, res = C.run_device(torch, gpu, table, rows, qkeys, 5, BIG)
    wants = C.model_all(b"", ops[:0], order[:0], dict(entries=0, user_keys=0, status=0), qkeys, rows, 5, BIG)
    C.compare(hits, res, wants, 5, "empty")
    assert statuses(wants) == {DONE, BAD_SEQ, BAD_QUERY}


def test_damaged_quadruples(gpu):
    """An order index >= op_cap and a key extent outside the payload: a walk
    that meets one is NO_TABLE with count 0, one that ends before it is
    answered, its neighbours in the launch are not disturbed and nothing
    outside the slots is written.  Searches over such tables (any status,
    contained): only the canaries and the bounds are checked."""
    import torch
    dam, items = C.damaged_cases()
    for name, broken in (("damaged_order_index", (17, 90)), ("damaged_key_extent", (30, 75, 100))):
        payload, ops, order, totals, cap = dam[name]
        table, _ = C.device_table(torch, gpu, payload, ops, order, totals)
        qs = [("resume", p, seen, None, s) for p in (0, 5, broken[0] - 1, broken[0], broken[0] + 1, broken[0] + 2, 101, 120)
              for seen in (0, 1) for s in (M, 0)]
        qkeys, rows = C.pack(qs)
        for limit, max_scan in ((BIG, BIG), (BIG, 3), (1, BIG), (2, 64)):
            wants = C.check_device(torch, gpu, payload, ops, order, totals, (qkeys, rows), limit, max_scan, table=table,
                                   tag_=(name, limit, max_scan), broken=broken)
            assert NO_TABLE in statuses(wants) and len(statuses(wants)) > 1
    seeks = C.queries_over(items, [0, 20, M], np.random.default_rng(3), some=80)
    qkeys, rows = C.pack(seeks)
    for name, (payload, ops, order, totals, cap) in dam.items():
        if name == "damaged_entries_over_cap":
            continue  # (the op table itself is shorter there: test_no_table's op_cap case)
        table, _ = C.device_table(torch, gpu, payload, ops, order, totals)
        for limit, max_scan in ((8, BIG), (1, 3)):
            r = MT.range_device(table, rows, qkeys, limit, max_scan, fill=CANARY, guard=GUARD)
            hits, res = r.sync()
            assert tail_is_canary(r.hits_t, len(rows) * limit * 4) and tail_is_canary(r.results_t, len(rows) * 40), name
            for q in range(len(rows)):
                g = {f: int(res[q][f]) for f in C.FIELDS}
                assert g["status"] <= BAD_QUERY and g["count"] <= limit and g["reserved"] == 0, (name, q, g)
                if g["status"] <= MORE_SCAN:
                    assert g["seek_pos"] <= g["next_pos"] <= g["seek_pos"] + max_scan and g["next_pos"] <= totals["entries"]
                    assert (hits[q, : g["count"]] < cap).all() and (hits[q, g["count"]:] == C.CANARY32).all(), (name, q, g)
                else:
                    assert g == C._status_only(g["status"])[1], (name, q, g)


@pytest.mark.parametrize("limit,max_scan", [(1, 1), (3, 5), (2, 64), (64, 2)])
def test_resume_chain_on_the_device(gpu, limit, max_scan):
    """Each call's queries are made on the device from the result tensor of
    the call before (pos = next_pos, SEEN = seen), on one stream with no
    synchronisation; the host reads nothing until the chain has ended.  The
    concatenated hits and summed unparsed are those of one large call."""
    import torch
    rng = np.random.default_rng(7)
    items = C.random_items(rng, 110) + C.special_items()
    payload, ops, order, totals = C.table_of(items)
    n = len(items)
    queries = C.queries_over(items, C.snapshots_of(items), rng, some=30) + [(b"", None, M), (b"", None, 20)]
    qkeys, rows = C.pack(queries)
    nq = len(rows)
    table, _ = C.device_table(torch, gpu, payload, ops, order, totals)
    calls = -(-n // min(limit, max_scan)) + 1  # every unfinished call examines at least min(limit, max_scan) entries
    d_qk = dev_bytes(torch, gpu, qkeys)[: len(qkeys)]
    s = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(s):
        q64 = torch.from_numpy(np.frombuffer(rows.tobytes(), dtype=np.int64).reshape(nq, 6).copy()).to(gpu)
        has_hi = q64[:, 5] & HAS_HI
        for _ in range(calls):
            r = MT.range_device(table, q64.view(torch.uint8).reshape(-1), d_qk, limit, max_scan, nq=nq, stream=s,
                                fill=CANARY, guard=GUARD)
            outs.append(r)
            res64 = r.results_t[: nq * 40].view(torch.int64).reshape(nq, 5)
            nxt = q64.clone()
            nxt[:, 0] = 0                               # lo is ignored
            nxt[:, 3] = res64[:, 1]                     # pos = next_pos
            nxt[:, 4] = (q64[:, 4] >> 32) << 32         # lo_len 0, hi_len kept
            nxt[:, 5] = has_hi | RESUME | ((res64[:, 4] & 1) * SEEN)
            q64 = nxt
    s.synchronize()
    got = [r.sync() for r in outs]
    wants = C.model_all(payload, ops, order, totals, qkeys, rows, 512, BIG)
    longest = 0
    for q, (wh, wr) in enumerate(wants):
        assert wr["status"] == DONE
        hits, unparsed, active = [], 0, 0
        for hs, res in got:
            st, cnt = int(res[q]["status"]), int(res[q]["count"])
            assert st in (DONE, MORE_LIMIT, MORE_SCAN) and (hs[q, cnt:] == C.CANARY32).all()
            hits += hs[q, :cnt].tolist()
            unparsed += int(res[q]["unparsed"])
            active += st != DONE
        assert hits == wh and unparsed == wr["unparsed"], (q, queries[q])
        last = got[-1][1][q]
        assert int(last["status"]) == DONE and int(last["next_pos"]) == wr["next_pos"] and int(last["seen"]) == wr["seen"]
        assert int(got[0][1][q]["seek_pos"]) == wr["seek_pos"]
        longest = max(longest, active)
    assert 2 < longest < calls


def test_random_table_of_5000(gpu):
    import torch
    rng = np.random.default_rng(5000)
    items = C.random_items(rng, 5000, nkeys=11)
    items += [(b"u%05d" % int(rng.integers(0, 700)), tag(int(rng.integers(1, 40)), int(rng.random() < 0.7)), b"x")
              for _ in range(2500)]
    items = [items[int(i)] for i in rng.permutation(len(items))][:5000]
    payload, ops, order, totals = C.table_of(items)
    keys = sorted({k for k, _, _ in items})
    qs = []
    for _ in range(300):
        a, b = keys[int(rng.integers(len(keys)))], keys[int(rng.integers(len(keys)))]
        qs.append((a, None if rng.random() < 0.3 else b + b"\x00", [0, 5, 20, 39, M][int(rng.integers(5))]))
    for limit, max_scan in ((BIG, BIG), (16, 1000)):
        wants = C.check_device(torch, gpu, payload, ops, order, totals, qs, limit, max_scan, shift=1)
        if limit == BIG:
            assert statuses(wants) == {DONE} and max(r["count"] for _, r in wants) > 100
        else:
            assert statuses(wants) == {DONE, MORE_LIMIT, MORE_SCAN}


def _two_tables():
    rng = np.random.default_rng(21)
    keys = [b"key%03d" % i for i in range(40)]
    parts, seq = [], 1
    for t in range(2):
        items = []
        for _ in range(100):
            k = keys[int(rng.integers(10 * t, 10 * t + 30))]  # keys 10..29 are in both tables
            typ = 0 if rng.random() < 0.3 else 1
            items.append((k, tag(seq, typ), b"" if typ == 0 else b"t%d-s%d" % (t, seq)))
            seq += 1
        parts.append(items)
    return parts, keys, seq - 1


def _merged(torch, gpu, parts, stream):
    """Two table images scanned into one op table (appended) and the memtable
    build over it, on `stream`: (Table, keep-alive)."""
    import sst_build_cases as S
    import sst_scan_cases as SC
    images = [S.model_build(*make_table(items), 64, 4)[0] for items in parts]
    tabs = [SC.open_table(img) for img in images]
    fulls = [SC.model_scan(img, t)[0] for img, t in zip(images, tabs)]
    acap, ocap = sum(f["table_bytes"] for f in fulls), sum(f["table_entries"] for f in fulls)
    bcap = max(t["data_blocks"] for t in tabs)
    prev, owners = None, []
    with torch.cuda.stream(stream):
        for i, img in enumerate(images):
            op, owner = SC.open_on(torch, gpu, img, shift=i, stream=stream)
            owners.append(owner)
            prev = SC.run_scan(torch, gpu, op, prev, arena_cap=acap, op_cap=ocap, block_cap=bcap, arena_shift=3,
                               stream=stream)
        table = MT.build_device(prev.arena_t[: prev.arena_cap], prev.ops_t, prev.totals[0:1], prev.totals[7:8],
                                op_cap=prev.op_cap, stream=stream, fill=CANARY, guard=GUARD)
    return table, (prev, owners)


def _merged_model(table, keep, parts):
    """The read-back op table of the merged view: (payload, ops, order,
    totals), after checking that it holds exactly the union of the parts."""
    from memtable_cases import key_of, model_order
    payload = table.payload.cpu().numpy().tobytes()
    tot = table.sync_totals()
    ops = keep[0].ops()[: tot["entries"]]
    have = sorted((key_of(payload, o), int(o["tag"]), payload[int(o["val_off"]):int(o["val_off"]) + int(o["val_len"])])
                  for o in ops)
    assert have == sorted(it for p in parts for it in p)
    order = np.array(model_order(payload, ops), dtype=np.uint32)
    assert table.order().tolist() == order.tolist()
    return payload, ops, order, tot


def test_the_merged_view_of_two_tables(gpu):
    """scan + scan (appended) + memtable build + range reads on one stream,
    one synchronisation; the ranges equal the model over the union."""
    import torch
    parts, keys, top = _two_tables()
    qs = [(b"", None, s) for s in (0, 50, 100, 150, top, M)]
    qs += [(keys[a], keys[b], s) for a, b, s in ((0, 39, M), (5, 15, 120), (12, 28, 90), (25, 26, M), (30, 10, M))]
    qs += [(k, k + b"\x00", s) for k in keys[8:32:3] for s in (60, 130, M)]
    qkeys, rows = C.pack(qs)
    s = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    table, keep = _merged(torch, gpu, parts, s)
    with torch.cuda.stream(s):
        r = MT.range_device(table, rows, qkeys, 64, BIG, stream=s, fill=CANARY, guard=GUARD)
        r1 = MT.range_device(table, rows, qkeys, 1, 7, stream=s, fill=CANARY, guard=GUARD)
    s.synchronize()
    payload, ops, order, tot = _merged_model(table, keep, parts)
    assert tot["entries"] == 200
    for out, limit, max_scan in ((r, 64, BIG), (r1, 1, 7)):
        hits, res = out.sync()
        wants = C.model_all(payload, ops, order, tot, qkeys, rows, limit, max_scan)
        C.compare(hits, res, wants, limit, (limit, max_scan))
        assert tail_is_canary(out.hits_t, len(rows) * limit * 4) and tail_is_canary(out.results_t, len(rows) * 40)
    # the newest visible version of a key both tables hold comes from the second table
    hits, res = r.sync()
    assert int(res[5]["count"]) > 20 and any(int(ops[h]["tag"]) >> 8 > 100 for h in hits[5, : int(res[5]["count"])])


def test_over_a_filtered_table(gpu):
    """A lvgpu.compact.Filtered is a Table: range reads over the kept order."""
    import torch
    import lvgpu.compact as CP
    rng = np.random.default_rng(33)
    items = C.random_items(rng, 180, type2=False)
    payload, ops, order, totals = C.table_of(items)
    table, _ = C.device_table(torch, gpu, payload, ops, order, totals)
    f = CP.filter_device(table, 15, None, 0, fill=CANARY, guard=GUARD)
    kept = f.order()
    ftot = f.sync_totals()
    assert f.sync()["status"] == 0 and 0 < len(kept) < 180 and ftot["entries"] == len(kept)
    pos = {int(i): at for at, i in enumerate(order)}
    assert [pos[int(i)] for i in kept] == sorted(pos[int(i)] for i in kept)  # a subsequence of the order
    qs = C.queries_over(items, [0, 15, 16, 30, M], rng, some=80)
    for limit, max_scan in ((BIG, BIG), (2, 9)):
        wants = C.check_device(torch, gpu, payload, ops, kept, ftot, qs, limit, max_scan, table=f, tag_=(limit, max_scan))
        # at and above the filter's snapshot the filtered table shows what the whole table shows
        whole = C.model_all(payload, ops, order, totals, *C.pack(qs, gaps=[i % 5 for i in range(len(qs))]),
                            C.clamp(limit), BIG)
        if max_scan == BIG and limit == BIG:
            for q, (w, k) in zip(qs, zip(whole, wants)):
                if q[2] >= 15:
                    assert w[0] == k[0], q


def test_graph_capture_and_one_replay(gpu):
    """The call captured into a graph after a warm-up; the replay runs over
    other queries laid into the same tensors."""
    import torch
    rng = np.random.default_rng(44)
    items = C.random_items(rng, 200)
    payload, ops, order, totals = C.table_of(items)
    table, _ = C.device_table(torch, gpu, payload, ops, order, totals)
    all_q = C.queries_over(items, [0, 9, 25, M], rng, some=120)
    sets = [C.pack(all_q[:60]), C.pack(all_q[60:])]
    nq = 60
    qsize = max(len(k) for k, _ in sets)
    d_qk = torch.zeros(max(qsize, 16), dtype=torch.uint8, device=gpu)
    d_q = torch.zeros(nq * 48, dtype=torch.uint8, device=gpu)

    def load(k):
        qk, rows = sets[k]
        d_qk.zero_()
        d_qk[: len(qk)].copy_(torch.frombuffer(bytearray(qk), dtype=torch.uint8))
        d_q.copy_(torch.frombuffer(bytearray(rows.tobytes()), dtype=torch.uint8))

    def verify(k, out, what):
        qk, rows = sets[k]
        hits, res = out.sync()
        wants = C.model_all(payload, ops, order, totals, bytes(qk) + bytes(qsize - len(qk)), rows, 4, 50)
        C.compare(hits, res, wants, 4, what)
        assert tail_is_canary(out.hits_t, nq * 16) and tail_is_canary(out.results_t, nq * 40)

    load(0)
    warm = MT.range_device(table, d_q, d_qk[:qsize], 4, 50, fill=CANARY, guard=GUARD)
    verify(0, warm, "warm")
    s = torch.cuda.Stream(device=gpu)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = MT.range_device(table, d_q, d_qk[:qsize], 4, 50, stream=s, fill=CANARY, guard=GUARD)
    torch.cuda.synchronize()
    load(1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    verify(1, out, "replay")


def test_positions_beyond_4_gib(gpu):
    """key_off beyond 2^32 in a high window of the payload and lo_off / hi_off
    beyond 2^32 in a high window of d_qkeys (positions64_cases): a position
    cut to 32 bits would read the decoy's other bytes."""
    import torch
    import positions64_cases as P
    from memtable_cases import model_totals
    HI = P.HI
    case = P.table_case(300)
    order, mt = model_totals(case.payload, case.ops)
    t, base = P.high_window(torch, gpu, case.payload, case.cut, case.decoy)
    pay = t[: base + len(case.payload)]
    hops = P.rebase(case.ops, base)
    assert int(hops["key_off"].max()) > HI > int(hops["key_off"].min())
    d_ops = dev_bytes(torch, gpu, hops)
    d_order = dev_bytes(torch, gpu, np.asarray(order, dtype=np.uint32)).view(torch.int32)
    from memtable_cases import dev_i64
    table = MT.Table(pay, d_ops, len(hops), d_order, dev_i64(torch, gpu, [mt["entries"], mt["user_keys"], 0]), None)
    rng = np.random.default_rng(64)
    qs = C.queries_over(case.items, [0, 11, 14, M], rng, some=90)
    qs = [q for q in qs if len(q[0]) >= 5][:60] + [("resume", 100, 1, None, M)]
    qkeys, rows = C.pack(qs)
    mid = next(i for i in range(len(qs) // 2, len(qs)) if int(rows[i]["lo_len"]) >= 8)
    qcut = int(rows[mid]["lo_off"]) + 3
    tq, qbase = P.high_window(torch, gpu, qkeys, qcut, P.complement(qkeys))
    d_qk = tq[: qbase + len(qkeys)]
    hrows = P.rebase(rows, qbase)
    assert int(hrows["lo_off"].max()) > HI > int(hrows["lo_off"][0]) and int(hrows["hi_off"].max()) > HI
    above = 0
    for limit, max_scan in ((BIG, BIG), (2, 20)):
        lim = C.clamp(limit)
        r = MT.range_device(table, hrows, d_qk, lim, max_scan, fill=CANARY, guard=GUARD)
        hits, res = r.sync()
        assert tail_is_canary(r.hits_t, len(rows) * lim * 4) and tail_is_canary(r.results_t, len(rows) * 40)
        wants = C.model_all(case.payload, case.ops, order, mt, qkeys, rows, lim, max_scan)
        C.compare(hits, res, wants, lim, (limit, max_scan))
        above += sum(int(hops[h]["key_off"]) > HI for w, _ in wants for h in w)
        assert sum(r_["count"] for _, r_ in wants) > 50
    assert above > 20
    del r, table, pay, d_qk, t, tq
    gc.collect()
    torch.cuda.empty_cache()
