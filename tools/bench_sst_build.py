#!/usr/bin/env python3
"""lv_sst_build_device against the host route it replaces.  One JSON line per
workload.

    python tools/bench_sst_build.py                          # A-C at ~256 MiB and W
    python tools/bench_sst_build.py --workloads A --mib 1024
    python tools/bench_sst_build.py --workloads W --worst-ops 262144

Workloads, those of tools/bench_memtable.py ("user:" keys): (A) single-Put
records; (B) 64-op batches; (C) batches of 16 ops with 4 KiB values.  (W) the
worst case of the size kernel: --worst-ops entries of one identical 4 KiB user
key, so every lane compares 4 KiB with its neighbour's key.

Timed per call, by HIP events on the launch stream after a warm-up (median of
--steps): "build_ms", lv_sst_build_device alone over the sorted memtable in
HBM (default options; file_cap and block_cap from a first, sizing call's
file_bytes and data_blocks); "flush_ms", lv_memtable_build_device and
lv_sst_build_device together.  "kernel_us": every kernel's microseconds per
call from a child run of this tool under `rocprofv3 --kernel-trace --stats`
(nothing else traced; the child is given the capacities, so every call it
makes is a whole build and a kernel's total divides by the number of calls), and "emit_frac": the emit kernel's bytes read (keys,
values, 36 B of op and order per entry) plus bytes written (the image) over
its time, as a fraction of 8 TB/s.  "host_route", in the same run: payload, op
table and order copied to page-locked host memory (wall clock, best of 3),
then lv_sst_build_host on one core (wall clock, one run).  The device image is
compared with the host twin's, byte for byte, before anything is reported,
and verified by lv_sst_verify_blocks_device.
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

KERNELS = ("sb_init", "sb_sizes", "sb_carry", "sb_next", "sb_reach", "sb_layout", "sb_index", "sb_plan", "sb_emit",
           "sb_tail", "sst_blocks_kernel", "crc32c_fused_small_kernel", "sb_index_trailer")


def kernel_split(argv):
    """({kernel: us per build call}, note) from a child run under rocprofv3
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
    out = tempfile.mkdtemp(prefix="lvgpu_sb_", dir="/tmp")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "kt", "--", sys.executable,
           os.path.abspath(__file__)] + argv + ["--steps", "5", "--warmup", "2", "--no-host", "--no-split",
                                                "--build-only"]
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
    if "sb_init" not in calls or "sb_emit" not in tot:
        return None, "kernels missing from the trace"
    n = calls["sb_init"]  # one per build call; every traced call is a whole build (--caps: no sizing call)
    if any(calls.get(k) != n for k in ("sb_emit", "sb_tail", "sst_blocks_kernel", "sb_index_trailer")):
        return None, f"the trace holds calls that are not whole builds: {calls}"
    return ({k: round(tot[k] / 1e3 / n, 2) for k in tot},
            "rocprofv3 --kernel-trace --stats, all launches of a kernel per build call (the seal's includes none other)")


def host_route(np, torch, lvgpu, T, table, n_ops, dev_file, dev_tot):
    """Copy-back and lv_sst_build_host; checks the device image."""
    L = T._bind_build()
    d_pay, d_ops, d_order = table.payload, table.ops_t, table.order_t
    nbytes = d_pay.numel()
    h_pay, h_ops = lvgpu.host_alloc(max(nbytes, 1)), lvgpu.host_alloc(max(n_ops * 32, 1))
    h_ord = lvgpu.host_alloc(max(n_ops * 4, 1))
    t_pay, t_ops, t_ord = torch.from_numpy(h_pay), torch.from_numpy(h_ops), torch.from_numpy(h_ord)
    copies = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t_pay[:nbytes].copy_(d_pay)
        t_ops[: n_ops * 32].copy_(d_ops[: n_ops * 32])
        t_ord[: n_ops * 4].copy_(d_order.view(torch.uint8)[: n_ops * 4])
        torch.cuda.synchronize()
        copies.append((time.perf_counter() - t0) * 1e3)
    mt = T.MtTotals(n_ops, 0, 0)
    tot = T.BuildTotals()
    file = np.empty(max(dev_tot["file_bytes"], 1), dtype=np.uint8)
    handles = np.empty(2 * (dev_tot["data_blocks"] + 2), dtype=np.uint64)
    t0 = time.perf_counter()
    rc = L.lv_sst_build_host(h_pay.ctypes.data, nbytes, h_ops.ctypes.data, h_ord.ctypes.data, ctypes.byref(mt), None,
                             file.ctypes.data, dev_tot["file_bytes"], handles.ctypes.data, dev_tot["data_blocks"],
                             ctypes.byref(tot))
    build_ms = (time.perf_counter() - t0) * 1e3
    if rc or tot.status:
        raise SystemExit(f"host build failed: rc {rc}, status {tot.status}")
    got = {k: int(getattr(tot, k)) for k in T.BUILD_TOTALS}
    if got != dev_tot:
        raise SystemExit(f"the device totals differ from the host twin's: {dev_tot} vs {got}")
    if not np.array_equal(file[: got["file_bytes"]], dev_file):
        bad = int(np.nonzero(file[: got["file_bytes"]] != dev_file)[0][0])
        raise SystemExit(f"the device image differs from the host twin's at byte {bad}")
    return {"copy_ms": round(min(copies), 3), "build_ms": round(build_ms, 3), "ms": round(min(copies) + build_ms, 3),
            "note": "D2H of payload, op table and order into page-locked memory + lv_sst_build_host on one core"}


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
        moved = int(ops["key_len"].sum())
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
        moved = None
    mws = torch.empty(MT.build_workspace_bytes(n_ops), dtype=torch.uint8, device=dev)
    table = MT.build_device(d_pay, d_ops, d_n, op_cap=n_ops, workspace=mws)
    table.sync_totals()
    if args.caps:  # the profiled child: the parent's capacities, so that every call it traces is a whole build
        fcap, bcap = (int(v) for v in args.caps.split(","))
    else:
        first = T.build_device(table, file_cap=0, block_cap=0)  # a sizing call: FILE_OVER | HANDLE_OVER, the true counts
        size = first.sync_totals(check=False)
        fcap, bcap = size["file_bytes"], size["data_blocks"]
    if fcap > T.file_bound(d_pay.numel(), n_ops):
        raise SystemExit("the image is larger than lv_sst_build_file_bound")
    sws = torch.empty(T.build_workspace_bytes(n_ops, bcap), dtype=torch.uint8, device=dev)
    keep = {}

    def build():
        keep["b"] = T.build_device(table, file_cap=fcap, block_cap=bcap, workspace=sws)

    def flush():
        keep["t"] = MT.build_device(d_pay, d_ops, d_n, op_cap=n_ops, workspace=mws)
        keep["b"] = T.build_device(keep["t"], file_cap=fcap, block_cap=bcap, workspace=sws)

    steps = max(args.steps // 5, 1) if name == "W" else args.steps
    build_ms = event_ms(torch, build, steps, args.warmup)
    if args.build_only:
        return
    tot = keep["b"].sync_totals()
    st = T.verify_blocks(keep["b"].file_t[: tot["file_bytes"]], keep["b"].handles_view())
    if int((st != T.BLOCK_OK).sum()):
        raise SystemExit(f"{name}: lv_sst_verify_blocks_device rejects a block")
    dev_file = keep["b"].file_t[: tot["file_bytes"]].cpu().numpy()
    flush_ms = event_ms(torch, flush, steps, args.warmup)
    if moved is None:
        o = d_ops[: n_ops * 32].view(torch.int64).view(-1, 4)[:, 3]
        moved = int((o & 0xFFFFFFFF).sum()) + int((o >> 32).sum())
    host = None if args.no_host else host_route(np, torch, lvgpu, T, table, n_ops, dev_file, tot)
    split, note = (None, "not asked for") if args.no_split else kernel_split(argv + ["--caps", f"{fcap},{bcap}"])
    emit_bytes = moved + 36 * n_ops + tot["file_bytes"]
    out = {"tool": "bench_sst_build", "api": "lv_sst_build_device", "workload": name, "label": args.label,
           "sb_tile": T.SB_TILE, "sb_wave_copy": T.SB_WAVE_COPY, "steps": steps, "warmup": args.warmup,
           "ops": int(n_ops), "payload_bytes": int(d_pay.numel()), "totals": tot,
           "build_ms": round(build_ms[0], 4), "build_ms_min": round(build_ms[1], 4), "build_ms_max": round(build_ms[2], 4),
           "flush_ms": round(flush_ms[0], 4), "file_GiB_per_s": round(tot["file_bytes"] / 2**30 / (build_ms[0] / 1e3), 1),
           "kernel_us": split, "kernel_us_note": note, "emit_bytes": emit_bytes,
           "emit_frac": round(emit_bytes / (split["sb_emit"] * 1e-6) / 8e12, 4) if split else None,
           "host_route": host, "build_speedup_vs_host_route": round(host["ms"] / build_ms[0], 2) if host else None,
           "build_speedup_vs_host_build_alone": round(host["build_ms"] / build_ms[0], 2) if host else None,
           "checked": "verify_blocks OK" + ("" if args.no_host else "; image == lv_sst_build_host's, every byte")}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="A,B,C,W")
    ap.add_argument("--mib", type=int, default=256, help="payload MiB of A-C")
    ap.add_argument("--worst-ops", type=int, default=1 << 16, help="entries of W")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="leave out the host route and the check against it")
    ap.add_argument("--no-split", action="store_true", help="leave out the rocprofv3 child run")
    ap.add_argument("--build-only", action="store_true", help="only the timed build calls (the profiled child run)")
    ap.add_argument("--caps", default="", help="file_cap,block_cap instead of a sizing call (the profiled child run)")
    ap.add_argument("--label", default="product", help="free text for the line (a variant library's name)")
    args = ap.parse_args()
    for name in args.workloads.split(","):
        name = name.strip().upper()
        argv = ["--workloads", name, "--mib", str(args.mib), "--worst-ops", str(args.worst_ops)]
        run(args, name, argv)


if __name__ == "__main__":
    main()
