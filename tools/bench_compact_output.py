#!/usr/bin/env python3
"""lv_compact_output_device against the routes it replaces, beside the one-file
build of the same input.  One JSON line per workload.

    python tools/bench_compact_output.py                    # A-C at 64 MiB
    python tools/bench_compact_output.py --workloads A --mib 256 --max-file-mib 2

Workloads, the op tables of tools/bench_compact.py ("user:" keys): (A)
single-Put records; (B) 64-op batches; (C) batches of 16 ops with 4 KiB values.
The sorted memtable is written with a Bloom filter (--bits-per-key, 0: none) and
upstream's max_file_size of --max-file-mib (2 MiB).

Timed per call, by HIP events on the launch stream after a warm-up (median of
--steps): "build_one_ms", lv_sst_build_bloom_device over the same memtable (one
image: the yardstick, the same block chain in the same run); "output_ms",
lv_compact_output_device with every record; "per_file_ms", the route a caller
had before, with the cuts known on the host: per output file one
lv_sst_build_bloom_device over its order slice, lv_sst_open_device,
lv_sst_bloom_open_device and lv_version_file_device, the slice copied on the
device to the head of an order array of op_cap entries first (no copy-back is
timed: the cuts are the output call's own, which flatters this route).  "host_route":
payload, ops and order copied to page-locked memory (wall clock, best of 3) and
lv_compact_output_host on one core (wall clock, one run).  Before anything is
reported the device's totals, arena, handles, records and bound keys are
compared with the host twin's.
"""
import argparse
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


def run(args, name):
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.compact as CP
    import lvgpu.memtable as MT
    import lvgpu.table as T
    import lvgpu.version as LV
    import lvgpu.write_batch as WB

    dev = torch.device("cuda:0")
    lvgpu.device_init()
    bpk = args.bits_per_key or None
    mf = args.max_file_mib << 20
    payload, off, ln, nops = build_log_payload(np, name, args.mib, "user")
    n_ops = off.size * nops
    d_pay = torch.from_numpy(payload).to(dev)
    wops = WB.decode_device(d_pay, torch.from_numpy(off.view(np.int64)).to(dev),
                            torch.from_numpy(ln.view(np.int64)).to(dev),
                            torch.tensor([off.size], dtype=torch.int64, device=dev), None, rec_cap=off.size, op_cap=n_ops)
    if wops.sync_totals()["ops"] != n_ops:
        raise SystemExit(f"{name}: {wops.sync_totals()}")
    d_n = torch.tensor([n_ops], dtype=torch.int64, device=dev)
    table = MT.build_device(d_pay, wops.ops_t, d_n, op_cap=n_ops)
    mt = table.sync_totals()
    keep = {}
    # the sizes, from the host twin (also the reference of the check below)
    ops = wops.ops_t[: 32 * n_ops].cpu().numpy().view(WB.OP_DTYPE).copy()
    order = table.order_t[:n_ops].cpu().numpy().view(np.uint32).copy()
    t0 = time.perf_counter()
    want = CP.output_host(payload.tobytes(), ops, order, mt, mf, bits_per_key=bpk, guard=0)
    host_ms = (time.perf_counter() - t0) * 1e3 / 2  # (a sizing pass and the call)
    t = want.totals
    acap, bcap, fcap, kcap = t["arena_bytes"], t["data_blocks"], t["files"], t["bound_bytes"]
    ws = torch.empty(CP.output_workspace_bytes(n_ops, bcap, fcap), dtype=torch.uint8, device=dev)
    # (the bytes between two files are never written: the twin's buffer was filled with 0xA5 first, so is this one)
    arena = torch.full((acap + 16,), 0xA5, dtype=torch.uint8, device=dev)
    bounds = torch.empty(kcap + 16, dtype=torch.uint8, device=dev)
    used = torch.zeros(1, dtype=torch.int64, device=dev)

    def output():
        used.zero_()
        keep["o"] = CP.output_device(table, mf, bits_per_key=bpk, arena_t=arena, arena_cap=acap, block_cap=bcap,
                                     files_cap=fcap, bounds_t=bounds, bound_cap=kcap, used_t=used, workspace=ws)

    output_ms = event_ms(torch, output, args.steps, args.warmup)
    out = keep["o"]
    if out.sync() != t:
        raise SystemExit(f"{name}: the device totals {out.sync()} differ from the host twin's {t}")
    for what, got, ref, nbytes in (("arena", arena, want.arena, acap), ("handles", out.handles_t, want.handles, 16 * t["handle_pairs"]),
                                   ("files", out.files_t, want.files, 64 * fcap), ("tables", out.tables_t, want.tables, 64 * fcap),
                                   ("blooms", out.blooms_t, want.blooms, 64 * fcap),
                                   ("version files", out.version_files_t, want.version_files, 64 * fcap),
                                   ("bound keys", bounds, want.bounds, kcap)):
        if not np.array_equal(got.view(torch.uint8)[:nbytes].cpu().numpy(), np.frombuffer(ref.tobytes(), dtype=np.uint8)[:nbytes]):
            raise SystemExit(f"{name}: the device {what} differ from the host twin's")
    one_cap = T.bloom_file_bound(d_pay.numel(), n_ops, bpk) if bpk else T.file_bound(d_pay.numel(), n_ops)
    bws = torch.empty((T.build_bloom_workspace_bytes if bpk else T.build_workspace_bytes)(n_ops, bcap), dtype=torch.uint8,
                      device=dev)

    def build_one():
        keep["b"] = T.build_device(table, file_cap=one_cap, block_cap=bcap, workspace=bws, bits_per_key=bpk)

    build_one_ms = event_ms(torch, build_one, args.steps, args.warmup)
    # the route before: a build, two opens and a version file per output file, the cuts known on the host
    files = want.files[:fcap]
    # (a build reads d_order[0, op_cap) and the order indexes the whole op table, so a file's slice is copied to
    # the head of an order array of op_cap entries: part of this route's cost)
    oslice = torch.zeros(max(n_ops, 4), dtype=torch.int32, device=dev)
    slices = [MT.Table(table.payload, table.ops_t, n_ops, oslice,
                       torch.tensor([int(f["entries"]), 0, 0], dtype=torch.int64, device=dev), None) for f in files]
    vout = torch.empty(64 * max(fcap, 1), dtype=torch.uint8, device=dev)

    def per_file():
        used.zero_()
        for k, (f, sl) in enumerate(zip(files, slices)):
            fe, fb = int(f["first_entry"]), int(f["file_bytes"])
            oslice[: int(f["entries"])].copy_(table.order_t[fe: fe + int(f["entries"])])
            b = T.build_device(sl, file_cap=fb, block_cap=int(f["data_blocks"]), workspace=bws, bits_per_key=bpk)
            op = T.open_device(b.file_t, b.totals[2:3], b.totals[7:8], handles=False)
            if bpk:
                T.bloom_open_device(op)
            LV.file_device(b.file_t, fb, 0, fb, op.table, 1 + k, 1, bounds, kcap, used, vout[64 * k: 64 * k + 64])

    per_file_ms = None
    if not args.no_per_file:
        per_file_ms = event_ms(torch, per_file, max(args.steps // 3, 1), 1)
    srcs = (table.payload, table.ops_t[: 32 * n_ops], table.order_t[:n_ops].view(torch.uint8))
    bufs = [torch.from_numpy(lvgpu.host_alloc(max(s.numel(), 1))) for s in srcs]
    copies = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for v, s in zip(bufs, srcs):
            v[: s.numel()].copy_(s)
        torch.cuda.synchronize()
        copies.append((time.perf_counter() - t0) * 1e3)
    line = {"tool": "bench_compact_output", "api": "lv_compact_output_device", "workload": name, "label": args.label,
            "steps": args.steps, "warmup": args.warmup, "bits_per_key": args.bits_per_key, "max_file_bytes": mf,
            "memtable_totals": mt, "totals": t, "output_ms": round(output_ms[0], 4),
            "output_ms_min": round(output_ms[1], 4), "output_ms_max": round(output_ms[2], 4),
            "build_one_ms": round(build_one_ms[0], 4), "output_over_build_one": round(output_ms[0] / build_one_ms[0], 3),
            "arena_GB_per_s": round(acap / 1e9 / (output_ms[0] / 1e3), 2),
            "per_file_ms": round(per_file_ms[0], 3) if per_file_ms else None,
            "speedup_vs_per_file": round(per_file_ms[0] / output_ms[0], 2) if per_file_ms else None,
            "host_route": {"copy_ms": round(min(copies), 3), "host_ms": round(host_ms, 3),
                           "ms": round(min(copies) + host_ms, 3),
                           "note": "D2H of payload, ops and order into page-locked memory + lv_compact_output_host on one core"},
            "speedup_vs_host_route": round((min(copies) + host_ms) / output_ms[0], 2),
            "checked": "totals, arena, handles, files, tables, blooms, version files and bound keys == lv_compact_output_host's"}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="A,B,C")
    ap.add_argument("--mib", type=int, default=64, help="payload MiB")
    ap.add_argument("--max-file-mib", type=int, default=2, help="max_file_bytes in MiB (upstream: 2)")
    ap.add_argument("--bits-per-key", type=int, default=10, help="0: no filter policy")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-per-file", action="store_true", help="leave out the per-file route")
    ap.add_argument("--label", default="product", help="free text for the line (a variant library's name)")
    args = ap.parse_args()
    for name in args.workloads.split(","):
        run(args, name.strip().upper())


if __name__ == "__main__":
    main()
