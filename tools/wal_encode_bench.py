#!/usr/bin/env python3
"""lv_wal_encode_device against lv_wal_encode_host on the records of
`bench.py --wal`: logical sizes Random(301).skewed(17) (oracle/wal_oracle.py,
the generator bench.py's wal_bench draws from) until --mib of payload, the
payload generated in HBM by lv_fill_splitmix.  Prints one JSON line.

    python tools/wal_encode_bench.py                 # ~1 GiB
    python tools/wal_encode_bench.py --mib 64        # one Infinity-Cache-sized batch
    # counters: one per pass (FETCH_SIZE and WRITE_SIZE together exceed one pass), nothing else traced
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d OUT -- \
        python tools/wal_encode_bench.py --steps 3 --warmup 1 --no-host --no-split

The device call is timed by HIP events around lv_wal_encode_device: the host's
layout and table fill, the table upload, the CRC step and wal_frame_kernel.
The split between the CRC step and wal_frame_kernel is the kernels' own time:
a child run of this tool under `rocprofv3 --kernel-trace --stats` (nothing
else traced), mean microseconds per launch of each kernel the call makes
("kernel_us").  "crc_step_ms" is the same lv_crc32c_batch_device_hint call over
the same fragments timed by events on its own (their lengths read back from a
scan of the encoded log; the records lie end to end, so fragment k starts
where fragment k - 1 ended), and "rest_ms" what remains of the call: host
layout, upload and wal_frame_kernel.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "leveldb-rs_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12  # bytes / s


def event_ms(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2], ts[0], ts[-1]


CALL_KERNELS = ("lvk::sort_hist", "lvk::sort_scan", "lvk::sort_scatter", "lvk::crc32c_classes_kernel<true>",
                "lvk::crc32c_fused_small_kernel", "lvk::combine_long_kernel", "lvk::wal_frame_kernel")


def kernel_split(mib):
    """{kernel: mean us per launch} of the kernels lv_wal_encode_device
    launches, from a child run under rocprofv3 --kernel-trace --stats; or
    (None, reason)."""
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
    out = tempfile.mkdtemp(prefix="lvgpu_kt_", dir="/tmp")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "kt", "--", sys.executable,
           os.path.abspath(__file__), "--mib", str(mib), "--steps", "10", "--warmup", "3", "--no-host", "--no-split"]
    try:
        subprocess.run(cmd, env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                       timeout=300, check=True)
    except Exception as e:  # noqa: BLE001 - report, never fail the bench on the profiler
        shutil.rmtree(out, ignore_errors=True)
        return None, f"rocprofv3 pass failed: {e}"
    per = {}
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                k = row["Name"].split("(")[0].replace("void ", "")
                if k in CALL_KERNELS:
                    per[k] = round(float(row["AverageNs"]) / 1e3, 2)
    shutil.rmtree(out, ignore_errors=True)
    if "lvk::wal_frame_kernel" not in per:
        return None, "no wal_frame_kernel in the trace"
    return per, "rocprofv3 --kernel-trace --stats, mean per launch"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024, help="payload MiB")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="leave out the lv_wal_encode_host baseline (counter runs)")
    ap.add_argument("--no-split", action="store_true", help="leave out the kernel-trace child run")
    args = ap.parse_args()

    import numpy as np
    import torch

    import lvgpu
    import lvgpu.wal as LW
    import wal_oracle as W

    dev = torch.device("cuda:0")
    lvgpu.device_init()
    target = args.mib << 20
    r = W.Random(301)
    sizes, tot = [], 0
    while tot < target:
        sizes.append(r.skewed(17))
        tot += sizes[-1]
    ln = np.array(sizes, dtype=np.uint64)
    off = np.zeros(ln.size, dtype=np.uint64)
    off[1:] = np.cumsum(ln[:-1])
    payload = torch.empty(tot, dtype=torch.uint8, device=dev)
    lvgpu.fill_splitmix(payload, 0, 0x5EED)
    need, frags = LW.encode_size(ln)
    out = torch.empty(need, dtype=torch.uint8, device=dev)
    ws = torch.empty(LW.encode_workspace_bytes(frags), dtype=torch.uint8, device=dev)

    def encode():
        LW.encode_device(payload, off, ln, 0, out=out, workspace=ws)

    ms, ms_min, ms_max = event_ms(torch, encode, args.steps, args.warmup)

    # the CRC step alone: the same hinted offsets-API call over the same fragments
    hdr, crc, info, count = LW.scan_device(out, frags)
    torch.cuda.synchronize()
    assert int(count.item()) == frags
    flen = (info.view(torch.int32).to(torch.int64) >> 16) & 0xFFFF
    foff = torch.cumsum(flen, 0) - flen
    flen32 = flen.to(torch.int32)
    seed = torch.zeros(frags, dtype=torch.int32, device=dev)
    hint = lvgpu.hint_for(flen.cpu().numpy())
    hint.uniform = 0
    crc_out = torch.empty(frags, dtype=torch.int32, device=dev)
    crc_ws = torch.empty(lvgpu.workspace_bytes(frags), dtype=torch.uint8, device=dev)

    def crc_step():
        lvgpu.batch_hint(payload, foff, flen32, hint, seed=seed, out=crc_out, masked=True, workspace=crc_ws)

    crc_ms, _, _ = event_ms(torch, crc_step, args.steps, args.warmup)
    del hdr, crc, info, crc_out, crc_ws

    host = None
    if not args.no_host:
        L = LW._bind()
        h_pay = payload.cpu().numpy()
        h_out = np.empty(need, dtype=np.uint8)
        got = ctypes.c_size_t()

        def host_encode():
            rc = L.lv_wal_encode_host(h_pay.ctypes.data, off.ctypes.data, ln.ctypes.data, ln.size, 0, h_out.ctypes.data,
                                      h_out.size, ctypes.byref(got), 0)
            if rc:
                raise SystemExit("lv_wal_encode_host: " + lvgpu.lib().lv_last_error().decode())

        host_encode()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            host_encode()
            ts.append((time.perf_counter() - t0) * 1e3)
        host_ms = sorted(ts)[len(ts) // 2]
        same = bool(np.array_equal(out.cpu().numpy(), h_out))
        host = {"ms": round(host_ms, 3), "gib_s": round(need / 2**30 / (host_ms / 1e3), 2),
                "device_log_equals_host_log": same}
        if not same:
            raise SystemExit("device log differs from lv_wal_encode_host's")

    kernel_us, kernel_note = (None, "off") if args.no_split else kernel_split(args.mib)
    moved = 2 * tot + need  # the payload read by the CRC step and by the frame kernel, the log written once
    res = {"tool": "wal_encode_bench", "api": "lv_wal_encode_device", "records": int(ln.size), "fragments": frags,
           "payload_bytes": int(tot), "log_bytes": int(need), "steps": args.steps, "warmup": args.warmup,
           "ms": round(ms, 4), "ms_min": round(ms_min, 4), "ms_max": round(ms_max, 4),
           "gib_s": round(need / 2**30 / (ms / 1e3), 1),
           "kernel_us": kernel_us, "kernel_us_note": kernel_note,
           "crc_kernels_us": round(sum(v for k, v in kernel_us.items() if k != "lvk::wal_frame_kernel"), 2)
           if kernel_us else None,
           "frame_kernel_us": kernel_us["lvk::wal_frame_kernel"] if kernel_us else None,
           "crc_step_ms": round(crc_ms, 4), "rest_ms": round(ms - crc_ms, 4),
           "rest_note": "call - CRC step by events: host layout and table fill, upload, wal_frame_kernel",
           "bytes_moved": int(moved), "frac_of_8TBs": round(moved / (ms / 1e3) / HBM_PEAK, 4),
           "host": host, "speedup_vs_host": round(host["ms"] / ms, 1) if host else None}
    print(json.dumps(res))
    if host and not ms < host["ms"]:
        raise SystemExit("lv_wal_encode_device is not faster than lv_wal_encode_host")


if __name__ == "__main__":
    main()
