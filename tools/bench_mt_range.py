#!/usr/bin/env python3
"""lv_memtable_range_device against the host route it replaces, beside
lv_memtable_get_device over the same keys.  One JSON line per setting.

    python tools/bench_mt_range.py                       # hidden 0 and 0.5, 2^16 and 2^20 ranges, limit 16 and 256
    python tools/bench_mt_range.py --hidden 0.5 --nq 65536 --limits 16

The table: the op table of tools/bench_memtable.py's workload A with "user:"
keys at --mib 64 (512 K single-Put entries, 16-byte keys), sorted by
lv_memtable_build_device.  Overwrites as in tools/bench_compact.py: a share
--hidden of the ops, chosen at random, have their keys pointed at another op's
key, so that after the sort they are older versions of it and hidden at the
snapshot LV_MT_MAX_SEQUENCE.  A range: a seek to the key of a random entry (its
extent in the payload itself: d_qkeys is d_payload), no hi, max_scan 2^40, so
every walk runs to `limit` hits or the end of the table.

Timed per call, by HIP events on the launch stream after a warm-up (median of
--steps): "range_ms", lv_memtable_range_device; "seek_only_ms",
lv_memtable_get_device over the same lo keys at the same snapshot (the
yardstick for the seek part: one lane per query, a binary search).  From the
results: "examined" = the sum of next_pos - seek_pos, "entries_per_s" =
examined / range_ms, "bytes_per_examined_entry" = what the walk reads for an
entry (its order word, its op, its key and the predecessor's key for the group
test; the hit's 4 B written are "hit_bytes") and "seek_probe_bytes", what one
query's seek probes (ceil(log64 n) steps of 64 order words, ops and keys).
"host_route", in the same run: payload, ops and order copied to page-locked
host memory (wall clock, best of 3), then lv_memtable_range_host on one core
for the first --host-queries queries (wall clock, less the measured cost of as
many calls that return at once), scaled to all queries in "ms_scaled".  Before
anything is reported the device's results and hits of those queries are
compared with the host twin's.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "leveldb-rs_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_memtable import build_log_payload, event_ms  # noqa: E402


def make_table(args, np, torch, MT, WB, dev, hidden):
    """The sorted table of workload A with a share `hidden` of older versions:
    (Table, ops as a structured array)."""
    payload, off, ln, nops = build_log_payload(np, "A", args.mib, "user")
    n_ops = off.size * nops
    d_pay = torch.from_numpy(payload).to(dev)
    wops = WB.decode_device(d_pay, torch.from_numpy(off.view(np.int64)).to(dev), torch.from_numpy(ln.view(np.int64)).to(dev),
                            torch.tensor([off.size], dtype=torch.int64, device=dev), None, rec_cap=off.size, op_cap=n_ops)
    if wops.sync_totals()["ops"] != n_ops:
        raise SystemExit(f"decode: {wops.sync_totals()}")
    ops = wops.ops_t[: 32 * n_ops].cpu().numpy().view(WB.OP_DTYPE).copy()
    rng = np.random.default_rng(21)
    over = rng.permutation(n_ops)[: int(hidden * n_ops)]  # these become older or newer versions of other keys
    live = np.setdiff1d(np.arange(n_ops), over)
    src = live[rng.integers(0, live.size, size=over.size)]
    ops["key_off"][over] = ops["key_off"][src]
    ops["key_len"][over] = ops["key_len"][src]
    d_ops = torch.from_numpy(ops.view(np.uint8)).to(dev)
    table = MT.build_device(d_pay, d_ops, torch.tensor([n_ops], dtype=torch.int64, device=dev), op_cap=n_ops)
    table.sync_totals()
    return table, ops


def host_route(np, torch, lvgpu, MT, table, rows, limit, max_scan, count, dev_hits, dev_res):
    """Copy-back and lv_memtable_range_host for the first `count` queries;
    checks the device's answers to them."""
    L = MT._bind()
    n = table.op_cap
    srcs = (table.payload, table.ops_t[: 32 * n], table.order_t[:n].view(torch.uint8))
    bufs = [lvgpu.host_alloc(max(s.numel(), 1)) for s in srcs]
    views = [torch.from_numpy(b) for b in bufs]
    copies = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for v, s in zip(views, srcs):
            v[: s.numel()].copy_(s)
        torch.cuda.synchronize()
        copies.append((time.perf_counter() - t0) * 1e3)
    tot = MT.Totals(*[int(v) for v in table.totals.cpu().numpy().view(np.uint64)])
    rows = np.ascontiguousarray(rows[:count])
    hits = np.zeros((count, limit), dtype=np.uint32)
    res = np.zeros(count, dtype=MT.RANGE_RESULT_DTYPE)
    idle = rows.copy()  # the same calls, answered at once: the cost of calling
    idle["flags"], idle["pos"] = MT.RANGE_RESUME, tot.entries
    fn, pay, pn = L.lv_memtable_range_host, bufs[0].ctypes.data, srcs[0].numel()
    op, od, tp = bufs[1].ctypes.data, bufs[2].ctypes.data, ctypes.byref(tot)

    def loop(q):
        qp, hp, rp = q.ctypes.data, hits.ctypes.data, res.ctypes.data
        t0 = time.perf_counter()
        for i in range(count):  # d_qkeys is the payload
            if fn(pay, pn, op, od, tp, n, pay, pn, qp + 48 * i, limit, max_scan, hp + 4 * limit * i, rp + 40 * i):
                raise SystemExit("lv_memtable_range_host refused a query")
        return (time.perf_counter() - t0) * 1e3

    call_ms = loop(idle)
    raw_ms = loop(rows)
    if not np.array_equal(res, dev_res[:count]):
        bad = int(np.nonzero(res != dev_res[:count])[0][0])
        raise SystemExit(f"the device result of query {bad} differs from the host twin's: {dev_res[bad]} vs {res[bad]}")
    live = np.arange(limit)[None, :] < res["count"][:, None]
    if not np.array_equal(np.where(live, hits, 0), np.where(live, dev_hits[:count], 0)):
        raise SystemExit("the device hits differ from the host twin's")
    ms = max(raw_ms - call_ms, 0.0)
    return {"copy_ms": round(min(copies), 3), "queries": count, "walk_ms_raw": round(raw_ms, 3),
            "call_overhead_ms": round(call_ms, 3), "walk_ms": round(ms, 3), "us_per_query": round(ms * 1e3 / count, 3),
            "note": "D2H of payload, ops and order into page-locked memory + lv_memtable_range_host on one core"}


def run(args, hidden):
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.memtable as MT
    import lvgpu.write_batch as WB

    dev = torch.device("cuda:0")
    lvgpu.device_init()
    table, ops = make_table(args, np, torch, MT, WB, dev, hidden)
    mt = table.sync_totals()
    n = mt["entries"]
    klen = float(ops["key_len"].astype(np.uint64).sum()) / max(n, 1)
    steps64 = 0
    while 64 ** steps64 < max(n, 1):
        steps64 += 1
    rng = np.random.default_rng(5)
    max_scan = 1 << 40
    for nq in args.nq:
        pick = rng.integers(0, n, size=nq)
        rows = np.zeros(nq, dtype=MT.RANGE_QUERY_DTYPE)
        rows["lo_off"], rows["lo_len"], rows["seq"] = ops["key_off"][pick], ops["key_len"][pick], MT.MAX_SEQUENCE
        d_q = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
        d_off = torch.from_numpy(rows["lo_off"].astype(np.int64)).to(dev)
        d_len = torch.from_numpy(rows["lo_len"].astype(np.int32)).to(dev)
        d_seq = torch.from_numpy(rows["seq"].astype(np.int64)).to(dev)
        keep = {}

        def seek_only():
            keep["g"] = MT.get_device(table, table.payload, d_off, d_len, d_seq, nq=nq)

        seek_ms = event_ms(torch, seek_only, args.steps, args.warmup)
        for limit in args.limits:
            def ranges():
                keep["r"] = MT.range_device(table, d_q, table.payload, limit, max_scan, nq=nq)

            range_ms = event_ms(torch, ranges, args.steps, args.warmup)
            hits, res = keep["r"].sync()
            examined = int((res["next_pos"] - res["seek_pos"]).sum())
            shown = int(res["count"].astype(np.uint64).sum())
            st = {int(k): int(v) for k, v in zip(*np.unique(res["status"], return_counts=True))}
            host = None
            if not args.no_host:
                host = host_route(np, torch, lvgpu, MT, table, rows, limit, max_scan, min(args.host_queries, nq), hits, res)
                host["ms_scaled"] = round(host["copy_ms"] + host["walk_ms"] * nq / host["queries"], 3)
            del hits
            walk_bytes = 4 + 32 + 2 * klen
            out = {"tool": "bench_mt_range", "api": "lv_memtable_range_device", "label": args.label, "workload": "A/user",
                   "mib": args.mib, "hidden_asked": hidden, "memtable_totals": mt,
                   "hidden_share": round(1 - mt["user_keys"] / max(n, 1), 4), "nq": nq, "limit": limit,
                   "steps": args.steps, "warmup": args.warmup, "range_ms": round(range_ms[0], 4),
                   "range_ms_min": round(range_ms[1], 4), "range_ms_max": round(range_ms[2], 4),
                   "seek_only_ms": round(seek_ms[0], 4), "examined": examined, "hits": shown, "statuses": st,
                   "entries_per_s": round(examined / (range_ms[0] / 1e3), 1),
                   "ns_per_query": round(range_ms[0] * 1e6 / nq, 2),
                   "bytes_per_examined_entry": round(walk_bytes, 1), "hit_bytes": 4,
                   "seek_probe_bytes": round(steps64 * 64 * (4 + 32 + klen), 1),
                   "walk_GB_per_s": round(examined * walk_bytes / 1e9 / (range_ms[0] / 1e3), 1),
                   "host_route": host,
                   "speedup_vs_host_route_scaled": round(host["ms_scaled"] / range_ms[0], 1) if host else None,
                   "checked": None if args.no_host else
                   f"results and hits of the first {host['queries']} queries == lv_memtable_range_host's"}
            print(json.dumps(out), flush=True)
            keep.pop("r", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64, help="payload MiB of workload A (64: 512 K entries)")
    ap.add_argument("--hidden", default="0,0.5", help="shares of the entries hidden at the snapshot")
    ap.add_argument("--nq", default="65536,1048576", help="ranges per call")
    ap.add_argument("--limits", default="16,256", help="hits per range")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-queries", type=int, default=16384, help="queries the host route walks (and the check covers)")
    ap.add_argument("--no-host", action="store_true", help="leave out the host route and the check against it")
    ap.add_argument("--label", default="product", help="free text for the line (a variant library's name)")
    args = ap.parse_args()
    args.nq = [int(x) for x in args.nq.split(",")]
    args.limits = [int(x) for x in args.limits.split(",")]
    for h in args.hidden.split(","):
        run(args, float(h))


if __name__ == "__main__":
    main()
