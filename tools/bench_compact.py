#!/usr/bin/env python3
"""lv_compact_filter_device against the host route it replaces, beside the
memtable build of the same input.  One JSON line per workload.

    python tools/bench_compact.py                          # A-C at 64 MiB and W
    python tools/bench_compact.py --workloads A --mib 256 --hidden 0.75

Workloads, the op tables of tools/bench_sst_scan.py's merge ("user:" keys): (A)
single-Put records; (B) 64-op batches; (C) batches of 16 ops with 4 KiB values;
(W) --worst-ops entries of one identical 4 KiB user key, the serial worst case:
one lane compares 4 KiB with its predecessor per entry.  Overwrites: in A-C a
share --hidden of the ops, chosen at random, have their keys pointed at another
op's key, so that after the sort they are older versions of it and hidden at
S = LV_MT_MAX_SEQUENCE - 1; in W, S is the sequence below which that share of
the versions lies.  "hidden_share" is what the totals then say.

Timed per call, by HIP events on the launch stream after a warm-up (median of
--steps): "memtable_build_ms", lv_memtable_build_device over the op table (the
yardstick: the stage before the filter, over the same input in the same run);
"filter_ms", lv_compact_filter_device alone with LV_COMPACT_BASE_LEVEL;
"filter_build_ms", the filter followed by lv_sst_build_device; "build_all_ms"
and "build_kept_ms", lv_sst_build_device alone over the unfiltered memtable and
over the filter's result (the same op_cap, so the same launches: what shrinks
is the work inside them).  "bytes_per_entry": order, op
and key bytes read plus 4 B written (two order words, two ops and two keys per
entry in the flag kernel, the order word and two scanned words in the scatter,
two order words, ops and keys per kept entry in the user-key count), and
"filter_GB_per_s" those bytes over filter_ms.  "host_route", in the same run:
payload, ops and order copied to page-locked host memory (wall clock, best of
3), then lv_compact_filter_host on one core (wall clock, one run).  Before
anything is reported the device's totals and d_order_out are compared with the
host twin's.
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


def host_route(np, torch, lvgpu, CP, table, filtered, S, flags):
    """Copy-back and lv_compact_filter_host; checks the device result."""
    L = CP._bind()
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
    mt = CP.MtTotals(*[int(v) for v in table.totals.cpu().numpy().view(np.uint64)])
    mto, tot = CP.MtTotals(), CP.CompactTotals()
    out = np.empty(max(n, 1), dtype=np.uint32)
    t0 = time.perf_counter()
    rc = L.lv_compact_filter_host(bufs[0].ctypes.data, srcs[0].numel(), bufs[1].ctypes.data, bufs[2].ctypes.data,
                                  ctypes.byref(mt), n, S, None, 0, None, 0, out.ctypes.data, ctypes.byref(mto),
                                  ctypes.byref(tot), flags)
    ms = (time.perf_counter() - t0) * 1e3
    got = {k: int(getattr(tot, k)) for k in CP.TOTALS}
    if rc or got != filtered.sync():
        raise SystemExit(f"the device totals differ from the host twin's: {filtered.sync()} vs {got} (rc {rc})")
    if not np.array_equal(filtered.order_t[: got["kept"]].cpu().numpy().view(np.uint32), out[: got["kept"]]):
        raise SystemExit("the device d_order_out differs from the host twin's")
    return {"copy_ms": round(min(copies), 3), "filter_ms": round(ms, 3), "ms": round(min(copies) + ms, 3),
            "note": "D2H of payload, ops and order into page-locked memory + lv_compact_filter_host on one core"}


def run(args, name):
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.compact as CP
    import lvgpu.memtable as MT
    import lvgpu.table as T
    import lvgpu.write_batch as WB

    dev = torch.device("cuda:0")
    lvgpu.device_init()
    rng = np.random.default_rng(21)
    S = MT.MAX_SEQUENCE - 1
    if name == "W":
        n_ops, klen = args.worst_ops, 4096
        key = np.random.default_rng(9).integers(0, 256, size=klen, dtype=np.uint8)
        payload = np.tile(key, n_ops)
        ops = np.zeros(n_ops, dtype=WB.OP_DTYPE)
        ops["tag"] = (np.random.default_rng(10).permutation(n_ops).astype(np.uint64) << np.uint64(8)) | np.uint64(1)
        ops["key_off"] = np.arange(n_ops, dtype=np.uint64) * np.uint64(klen)
        ops["val_off"] = ops["key_off"] + np.uint64(klen)
        ops["key_len"] = klen
        S = int(args.hidden * n_ops)  # the versions below S are hidden
        d_pay = torch.from_numpy(payload).to(dev)
    else:
        payload, off, ln, nops = build_log_payload(np, name, args.mib, "user")
        n_ops = off.size * nops
        d_pay = torch.from_numpy(payload).to(dev)
        wops = WB.decode_device(d_pay, torch.from_numpy(off.view(np.int64)).to(dev),
                                torch.from_numpy(ln.view(np.int64)).to(dev),
                                torch.tensor([off.size], dtype=torch.int64, device=dev), None, rec_cap=off.size,
                                op_cap=n_ops)
        if wops.sync_totals()["ops"] != n_ops:
            raise SystemExit(f"{name}: {wops.sync_totals()}")
        ops = wops.ops_t[: 32 * n_ops].cpu().numpy().view(WB.OP_DTYPE).copy()
        over = rng.permutation(n_ops)[: int(args.hidden * n_ops)]  # these become older versions of other keys
        live = np.setdiff1d(np.arange(n_ops), over)
        src = live[rng.integers(0, live.size, size=over.size)]
        ops["key_off"][over] = ops["key_off"][src]
        ops["key_len"][over] = ops["key_len"][src]
    d_ops = torch.from_numpy(ops.view(np.uint8)).to(dev)
    d_n = torch.tensor([n_ops], dtype=torch.int64, device=dev)
    mws = torch.empty(MT.build_workspace_bytes(n_ops), dtype=torch.uint8, device=dev)
    keep = {}

    def sort():
        keep["t"] = MT.build_device(d_pay, d_ops, d_n, op_cap=n_ops, workspace=mws)

    steps = max(args.steps // 5, 1) if name == "W" else args.steps
    sort_ms = event_ms(torch, sort, steps, args.warmup)
    table = keep["t"]
    mt = table.sync_totals()
    flags = CP.BASE_LEVEL
    cws = torch.empty(max(CP.filter_workspace_bytes(n_ops), 16), dtype=torch.uint8, device=dev)
    order_out = torch.empty(max(n_ops, 4), dtype=torch.int32, device=dev)
    mt_out = torch.empty(3, dtype=torch.int64, device=dev)
    ctot = torch.empty(8, dtype=torch.int64, device=dev)

    def filt():
        keep["f"] = CP.filter_device(table, S, None, flags, order_t=order_out, mt_totals=mt_out, totals=ctot, workspace=cws)

    filter_ms = event_ms(torch, filt, steps, args.warmup)
    tot = keep["f"].sync()
    size_all = T.build_device(table, file_cap=0, block_cap=0).sync_totals(check=False)  # sizing calls
    size_kept = T.build_device(keep["f"], file_cap=0, block_cap=0).sync_totals(check=False)
    fcap, bcap = size_all["file_bytes"], size_all["data_blocks"]
    bws = torch.empty(T.build_workspace_bytes(n_ops, bcap), dtype=torch.uint8, device=dev)

    def build_all():
        keep["a"] = T.build_device(table, file_cap=fcap, block_cap=bcap, workspace=bws)

    def filter_build():
        filt()
        keep["b"] = T.build_device(keep["f"], file_cap=fcap, block_cap=bcap, workspace=bws)

    def build_kept():
        keep["k"] = T.build_device(keep["f"], file_cap=fcap, block_cap=bcap, workspace=bws)

    build_all_ms = event_ms(torch, build_all, steps, args.warmup)
    build_kept_ms = event_ms(torch, build_kept, steps, args.warmup)
    filter_build_ms = event_ms(torch, filter_build, steps, args.warmup)
    kept_tot = keep["b"].sync_totals()
    if kept_tot["entries"] != tot["kept"] or kept_tot["file_bytes"] != size_kept["file_bytes"]:
        raise SystemExit(f"{name}: the compacted table holds {kept_tot}, the filter kept {tot}")
    host = None if args.no_host else host_route(np, torch, lvgpu, CP, table, keep["f"], S, flags)
    klen = int(ops["key_len"].astype(np.uint64).sum()) / max(n_ops, 1)
    n, k = tot["entries_in"], tot["kept"]
    moved = n * (2 * 4 + 2 * 32 + 2 * klen) + n * (4 + 4 + 4) + k * 4 + k * (2 * 4 + 2 * 32 + 2 * klen)
    out = {"tool": "bench_compact", "api": "lv_compact_filter_device", "workload": name, "label": args.label,
           "cf_tile": CP.CF_TILE, "steps": steps, "warmup": args.warmup, "hidden_asked": args.hidden,
           "smallest_snapshot": S, "flags": flags, "memtable_totals": mt, "totals": tot,
           "hidden_share": round(tot["dropped_hidden"] / max(n, 1), 4),
           "memtable_build_ms": round(sort_ms[0], 4), "filter_ms": round(filter_ms[0], 4),
           "filter_ms_min": round(filter_ms[1], 4), "filter_ms_max": round(filter_ms[2], 4),
           "filter_over_memtable_build": round(filter_ms[0] / sort_ms[0], 4),
           "bytes_per_entry": round(moved / max(n, 1), 1),
           "filter_GB_per_s": round(moved / 1e9 / (filter_ms[0] / 1e3), 1),
           "build_all_ms": round(build_all_ms[0], 4), "build_kept_ms": round(build_kept_ms[0], 4),
           "filter_build_ms": round(filter_build_ms[0], 4),
           "build_speedup_kept_vs_all": round(build_all_ms[0] / build_kept_ms[0], 3),
           "build_all_over_filter_build": round(build_all_ms[0] / filter_build_ms[0], 3),
           "file_bytes_all": size_all["file_bytes"], "file_bytes_kept": size_kept["file_bytes"],
           "file_shrink": round(1 - size_kept["file_bytes"] / max(size_all["file_bytes"], 1), 4),
           "host_route": host, "filter_speedup_vs_host_route": round(host["ms"] / filter_ms[0], 2) if host else None,
           "filter_speedup_vs_host_filter_alone": round(host["filter_ms"] / filter_ms[0], 2) if host else None,
           "checked": "the compacted table's entries == kept" + ("" if args.no_host else
                                                               "; totals and d_order_out == lv_compact_filter_host's")}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="A,B,C,W")
    ap.add_argument("--mib", type=int, default=64, help="payload MiB of A-C")
    ap.add_argument("--worst-ops", type=int, default=1 << 14, help="entries of W")
    ap.add_argument("--hidden", type=float, default=0.5, help="share of the entries hidden at the snapshot")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="leave out the host route and the check against it")
    ap.add_argument("--label", default="product", help="free text for the line (a variant library's name)")
    args = ap.parse_args()
    for name in args.workloads.split(","):
        run(args, name.strip().upper())


if __name__ == "__main__":
    main()
