#!/usr/bin/env python3
"""lv_sst_scan_device against the host route it replaces.  One JSON line per
workload.

    python tools/bench_sst_scan.py                          # A-C at 64 MiB and W
    python tools/bench_sst_scan.py --workloads A --mib 256

Workloads, those of tools/bench_sst_build.py ("user:" keys): (A) single-Put
records; (B) 64-op batches; (C) batches of 16 ops with 4 KiB values; (W)
--worst-ops entries of one identical 4 KiB user key, so every key is rebuilt
from the lane's own previous arena write.  The log is decoded, sorted and
flushed on the device (default options); the image stays where
lv_sst_build_device wrote it and is opened there.

Timed per call, by HIP events on the launch stream after a warm-up (median of
--steps): "scan_ms", lv_sst_scan_device alone with d_order (capacities from a
first, sizing call); "rebuild_ms", the scan and lv_sst_build_device over its
quadruple; "merge4_ms", the K = 4 merge: four scans of the image into one
arena, lv_memtable_build_device over the union and lv_sst_build_device over
that.  "kernel_us": every kernel's microseconds per scan from a child run of
this tool under `rocprofv3 --kernel-trace --stats` (nothing else traced; the
child is given the capacities, so every call it makes is a whole scan), and
"emit_frac": the emit kernel's bytes read (the image) plus bytes written (the
arena and 32 B of op per entry) over its time, as a fraction of 8 TB/s.
"host_route", in the same run: the image copied to page-locked host memory
(wall clock, best of 3), then lv_sst_scan_host on one core (wall clock, one
run).  Before anything is reported the totals and the first --check entries of
the device result (ops, keys and values) are compared with the host twin's.
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

KERNELS = ("ss_header", "ss_blocks", "ss_carry", "ss_count", "ss_plan", "ss_emit", "ss_order", "ss_finish")


def kernel_split(argv):
    """({kernel: us per scan call}, note) from a child run under rocprofv3
    --kernel-trace --stats, or (None, reason)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not found"
    if any(k.startswith("ROCPROF") for k in os.environ):  # already under a profiler: never nest one
        return None, "skipped (running under rocprofv3)"
    out = tempfile.mkdtemp(prefix="lvgpu_ss_", dir="/tmp")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "kt", "--", sys.executable,
           os.path.abspath(__file__)] + argv + ["--steps", "5", "--warmup", "2", "--scan-only"]
    try:
        subprocess.run(cmd, env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                       timeout=300, check=True)
    except Exception as e:  # noqa: BLE001 - report, never fail the bench on the profiler
        shutil.rmtree(out, ignore_errors=True)
        return None, f"rocprofv3 pass failed: {e}"
    tot, calls = {}, {}
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                k = row["Name"].split("(")[0].split("<")[0].replace("void ", "").replace("lvk::", "")
                if k in KERNELS:
                    tot[k] = tot.get(k, 0.0) + float(row["TotalDurationNs"])
                    calls[k] = calls.get(k, 0) + int(row["Calls"])
    shutil.rmtree(out, ignore_errors=True)
    if "ss_header" not in calls or "ss_emit" not in tot:
        return None, "kernels missing from the trace"
    n = calls["ss_header"]  # one per scan call
    if any(calls.get(k) != n for k in ("ss_emit", "ss_plan", "ss_count", "ss_order")):
        return None, f"the trace holds calls that are not whole scans: {calls}"
    return ({k: round(tot[k] / 1e3 / n, 2) for k in tot},
            "rocprofv3 --kernel-trace --stats, all launches of a kernel per scan call")


def host_route(np, torch, lvgpu, T, file_t, tab, dev, check):
    """Copy-back and lv_sst_scan_host; checks the device result."""
    L = T._bind_scan()
    nbytes = file_t.numel()
    h_file = lvgpu.host_alloc(max(nbytes, 1))
    t_file = torch.from_numpy(h_file)
    copies = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t_file[:nbytes].copy_(file_t)
        torch.cuda.synchronize()
        copies.append((time.perf_counter() - t0) * 1e3)
    tot_d = dev.sync()
    ne, nb = tot_d["table_entries"], tot_d["table_bytes"]
    htab = T.SstTable(*[tab[f] for f in T.TABLE_FIELDS])
    arena = np.empty(max(nb, 1), dtype=np.uint8)
    ops = np.empty(max(ne, 1) * 32, dtype=np.uint8)
    order = np.empty(max(ne, 1), dtype=np.uint32)
    tot, mt = T.ScanTotals(), T.MtTotals()
    t0 = time.perf_counter()
    rc = L.lv_sst_scan_host(h_file.ctypes.data, ctypes.byref(htab), None, arena.ctypes.data, nb, ops.ctypes.data, ne,
                            order.ctypes.data, ctypes.byref(mt), ctypes.byref(tot))
    scan_ms = (time.perf_counter() - t0) * 1e3
    if rc or tot.status:
        raise SystemExit(f"host scan failed: rc {rc}, status {tot.status}")
    got = {k: int(getattr(tot, k)) for k in T.SCAN_TOTALS}
    if got != tot_d:
        raise SystemExit(f"the device totals differ from the host twin's: {tot_d} vs {got}")
    hmt = dict(entries=int(mt.entries), user_keys=int(mt.user_keys), status=int(mt.status))
    if hmt != dev.mt():
        raise SystemExit(f"the device memtable totals differ from the host twin's: {dev.mt()} vs {hmt}")
    k = min(check, ne)
    d_ops = dev.ops_t[: 32 * k].cpu().numpy()
    if not np.array_equal(d_ops, ops[: 32 * k]):
        raise SystemExit("the device ops differ from the host twin's")
    from lvgpu.write_batch import OP_DTYPE
    end = int(ops[: 32 * k].view(OP_DTYPE)["val_off"][-1] + ops[: 32 * k].view(OP_DTYPE)["val_len"][-1]) if k else 0
    if not np.array_equal(dev.arena_t[:end].cpu().numpy(), arena[:end]):
        raise SystemExit("the device arena differs from the host twin's")
    return {"copy_ms": round(min(copies), 3), "scan_ms": round(scan_ms, 3), "ms": round(min(copies) + scan_ms, 3),
            "note": "D2H of the image into page-locked memory + lv_sst_scan_host on one core"}, k


def run(args, name, argv):
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.memtable as MT
    import lvgpu.table as T
    import lvgpu.write_batch as WB

    dev = torch.device("cuda:0")
    lvgpu.device_init()
    if name == "W":
        n_ops, klen = args.worst_ops, 4096
        key = np.random.default_rng(9).integers(0, 256, size=klen, dtype=np.uint8)
        payload = np.tile(key, n_ops)
        ops = np.zeros(n_ops, dtype=WB.OP_DTYPE)
        ops["tag"] = (np.random.default_rng(10).permutation(n_ops).astype(np.uint64) << np.uint64(8)) | np.uint64(1)
        ops["key_off"] = np.arange(n_ops, dtype=np.uint64) * np.uint64(klen)
        ops["val_off"] = ops["key_off"] + np.uint64(klen)
        ops["key_len"] = klen
        d_pay = torch.from_numpy(payload).to(dev)
        d_ops = torch.from_numpy(ops.view(np.uint8)).to(dev)
        d_n = torch.tensor([n_ops], dtype=torch.int64, device=dev)
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
        d_ops, d_n = wops.ops_t, wops.totals[1:2].clone()
    table = MT.build_device(d_pay, d_ops, d_n, op_cap=n_ops)
    table.sync_totals()
    size = T.build_device(table, file_cap=0, block_cap=0).sync_totals(check=False)  # a sizing call
    built = T.build_device(table, file_cap=size["file_bytes"], block_cap=size["data_blocks"])
    tot = built.sync_totals()
    fcap, bcap = tot["file_bytes"], tot["data_blocks"]
    file_t = built.file_t[:fcap]
    opened = T.open_device(file_t, built.totals[2:3], built.totals[7:8], block_cap=bcap)
    tab = opened.sync()
    del table, d_pay, d_ops
    if args.caps:  # the profiled child: the parent's capacities, so that every call it traces is a whole scan
        acap, ocap = (int(v) for v in args.caps.split(","))
    else:
        first = T.scan_device(opened, arena_cap=0, op_cap=0, block_cap=bcap).sync(check=False)  # a sizing call
        acap, ocap = first["arena_bytes"], first["entries"]
    ws = torch.empty(T.scan_workspace_bytes(4 * ocap, bcap), dtype=torch.uint8, device=dev)
    arena = torch.empty(max(4 * acap, 16), dtype=torch.uint8, device=dev)
    ops_t = torch.empty(max(4 * ocap * 32, 16), dtype=torch.uint8, device=dev)
    order_t = torch.empty(max(ocap, 4), dtype=torch.int32, device=dev)
    mt_t = torch.empty(3, dtype=torch.int64, device=dev)
    tots = [torch.empty(8, dtype=torch.int64, device=dev) for _ in range(4)]
    keep = {}

    def scan():
        keep["s"] = T.scan_device(opened, arena_t=arena, arena_cap=acap, ops_t=ops_t, op_cap=ocap, block_cap=bcap,
                                  order=True, order_t=order_t, mt_totals=mt_t, totals=tots[0], workspace=ws)

    steps = max(args.steps // 5, 1) if name == "W" else args.steps
    scan_ms = event_ms(torch, scan, steps, args.warmup)
    if args.scan_only:
        return
    sc = keep["s"]
    t = sc.sync()
    bws = torch.empty(T.build_workspace_bytes(4 * ocap, 4 * bcap + 4), dtype=torch.uint8, device=dev)

    def rebuild():
        scan()
        keep["b"] = T.build_device(keep["s"].memtable(), file_cap=fcap, block_cap=bcap, workspace=bws)

    rebuild_ms = event_ms(torch, rebuild, steps, args.warmup)
    if not torch.equal(keep["b"].file_t[:fcap], file_t):
        raise SystemExit(f"{name}: scan + rebuild does not reproduce the image")
    mws = torch.empty(MT.build_workspace_bytes(4 * ocap), dtype=torch.uint8, device=dev)
    f4 = T.file_bound(4 * acap, 4 * ocap)

    def merge4():
        prev = None
        for k in range(4):
            if prev is None:
                prev = T.scan_device(opened, arena_t=arena, arena_cap=4 * acap, ops_t=ops_t, op_cap=4 * ocap,
                                     block_cap=bcap, totals=tots[0], workspace=ws)
            else:
                prev = T.scan_device(opened, prev, block_cap=bcap, totals=tots[k], workspace=ws)
        m = MT.build_device(arena[: 4 * acap], ops_t, prev.totals[0:1], prev.totals[7:8], op_cap=4 * ocap, workspace=mws)
        keep["m"] = T.build_device(m, file_cap=f4, block_cap=4 * bcap + 4, workspace=bws)

    merge_ms = event_ms(torch, merge4, max(steps // 2, 1), 1)
    mt4 = keep["m"].sync_totals()
    if mt4["entries"] != 4 * t["table_entries"]:
        raise SystemExit(f"{name}: the merge holds {mt4['entries']} entries, not {4 * t['table_entries']}")
    scan()  # (the merge reused the arena)
    host, checked = (None, 0) if args.no_host else host_route(np, torch, lvgpu, T, file_t, tab, keep["s"], args.check)
    split, note = (None, "not asked for") if args.no_split else kernel_split(argv + ["--caps", f"{acap},{ocap}"])
    emit_bytes = fcap + t["table_bytes"] + 32 * t["table_entries"]
    out = {"tool": "bench_sst_scan", "api": "lv_sst_scan_device", "workload": name, "label": args.label,
           "ss_tile": T.SS_TILE, "ss_wave_copy": T.SS_WAVE_COPY, "steps": steps, "warmup": args.warmup, "table": tab,
           "totals": t, "scan_ms": round(scan_ms[0], 4), "scan_ms_min": round(scan_ms[1], 4),
           "scan_ms_max": round(scan_ms[2], 4), "arena_GiB_per_s": round(t["table_bytes"] / 2**30 / (scan_ms[0] / 1e3), 1),
           "rebuild_ms": round(rebuild_ms[0], 4), "merge4_ms": round(merge_ms[0], 4), "merge4_totals": mt4,
           "kernel_us": split, "kernel_us_note": note, "emit_bytes": emit_bytes,
           "emit_frac": round(emit_bytes / (split["ss_emit"] * 1e-6) / 8e12, 4) if split else None,
           "host_route": host, "scan_speedup_vs_host_route": round(host["ms"] / scan_ms[0], 2) if host else None,
           "scan_speedup_vs_host_scan_alone": round(host["scan_ms"] / scan_ms[0], 2) if host else None,
           "checked": "scan + rebuild == the image" + ("" if args.no_host else
                                                      f"; totals and the first {checked} entries == lv_sst_scan_host's")}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="A,B,C,W")
    ap.add_argument("--mib", type=int, default=64, help="payload MiB of A-C")
    ap.add_argument("--worst-ops", type=int, default=1 << 14, help="entries of W")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=20000, help="entries compared with the host twin's")
    ap.add_argument("--no-host", action="store_true", help="leave out the host route and the check against it")
    ap.add_argument("--no-split", action="store_true", help="leave out the rocprofv3 child run")
    ap.add_argument("--scan-only", action="store_true", help="only the timed scan calls (the profiled child run)")
    ap.add_argument("--caps", default="", help="arena_cap,op_cap instead of a sizing call (the profiled child run)")
    ap.add_argument("--label", default="product", help="free text for the line (a variant library's name)")
    args = ap.parse_args()
    for name in args.workloads.split(","):
        name = name.strip().upper()
        argv = ["--workloads", name, "--mib", str(args.mib), "--worst-ops", str(args.worst_ops)]
        run(args, name, argv)


if __name__ == "__main__":
    main()
