#!/usr/bin/env python3
"""lv_wal_decode_device on the log of `tools/wal_encode_bench.py`: logical sizes
Random(301).skewed(17) (oracle/wal_oracle.py) until --mib of payload, the
payload generated in HBM by lv_fill_splitmix and the log written there by
lv_wal_encode_device.  Prints one JSON line.

    python tools/wal_decode_bench.py                 # ~1 GiB
    python tools/wal_decode_bench.py --mib 64
    # counters: one per pass, nothing else traced
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d OUT -- \
        python tools/wal_decode_bench.py --steps 3 --warmup 1 --no-host --no-split

Timed per call, by HIP events after a warm-up:
  (a) "scan_decode_ms": lv_wal_scan_device + lv_wal_decode_device, and
      "decode_ms": lv_wal_decode_device alone over the scan's arrays;
  (b) "host_route": in the same run, the only route to the records without
      lv_wal_decode_device -- the log and the scan arrays copied to page-locked
      host memory (wall clock, best of 5), then lv_wal_reader drained by the
      native loop of tools/host_replay.c (best of 5) -- to which the scan itself
      ("scan_ms", events) is added for the comparison with (a).
The kernels' own times are a child run of this tool under `rocprofv3
--kernel-trace --stats` (nothing else traced), mean microseconds per launch
("kernel_us").  The records the device decode returns are checked against the
input (lengths and payload bytes) before anything is reported.
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


CALL_KERNELS = ("lvk::wal_dec_classify", "lvk::wal_dec_reduce", "lvk::wal_dec_tiles", "lvk::wal_dec_apply",
                "lvk::wal_unframe_kernel")


def kernel_split(mib, keep=None):
    """{kernel: mean us per launch} of the kernels lv_wal_decode_device
    launches, from a child run under rocprofv3 --kernel-trace --stats; or
    (None, reason).  keep: a path the whole kernel statistics table is copied to."""
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
        if keep:
            shutil.copyfile(f, keep)
        with open(f) as fh:
            for row in csv.DictReader(fh):
                k = row["Name"].split("(")[0].replace("void ", "")
                if k in CALL_KERNELS:
                    per[k] = round(float(row["AverageNs"]) / 1e3, 2)
    shutil.rmtree(out, ignore_errors=True)
    if "lvk::wal_unframe_kernel" not in per:
        return None, "no wal_unframe_kernel in the trace"
    return per, "rocprofv3 --kernel-trace --stats, mean per launch"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024, help="payload MiB")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="leave out the host route (counter runs)")
    ap.add_argument("--no-split", action="store_true", help="leave out the kernel-trace child run")
    ap.add_argument("--keep-stats", default=None, help="copy the child run's kernel statistics table here")
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
    log = LW.encode_device(payload, off, ln, 0)
    torch.cuda.synchronize()
    assert log.numel() == need

    cap = frags
    scan_ws = torch.empty(LW.scan_workspace_bytes(need, cap), dtype=torch.uint8, device=dev)
    dec_ws = torch.empty(LW.decode_workspace_bytes(cap), dtype=torch.uint8, device=dev)
    out_pay = torch.empty(need, dtype=torch.uint8, device=dev)
    state = {}

    def scan():
        state["scan"] = LW.scan_device(log, cap, workspace=scan_ws)

    def decode():
        state["dec"] = LW.decode_device(log, *state["scan"], scan_cap=cap, payload=out_pay, workspace=dec_ws)

    def both():
        scan()
        decode()

    both()
    dec = state["dec"]
    t = dec.sync_totals()
    if t != {"records": int(ln.size), "payload_bytes": int(tot), "reports": 0, "dropped_bytes": 0, "status": 0}:
        raise SystemExit(f"decode totals differ from the input: {t}")
    if not (torch.equal(out_pay[:tot], payload) and
            torch.equal(dec.rec_len[: ln.size].cpu(), torch.from_numpy(ln.astype(np.int64))) and
            torch.equal(dec.rec_off[: ln.size].cpu(), torch.from_numpy(off.astype(np.int64)))):
        raise SystemExit("decoded records differ from the input")

    both_ms, both_min, both_max = event_ms(torch, both, args.steps, args.warmup)
    scan()
    dec_ms, dec_min, dec_max = event_ms(torch, decode, args.steps, args.warmup)
    scan_ms, _, _ = event_ms(torch, scan, args.steps, args.warmup)

    host = None
    if not args.no_host:
        hdr, crc, info, count = state["scan"]
        h_log = lvgpu.host_alloc(need)
        h_hdr = np.empty(frags, dtype=np.int64)
        h_crc = np.empty(frags, dtype=np.int32)
        h_info = np.empty(frags, dtype=np.int32)
        t_log = torch.from_numpy(h_log)
        t_hdr, t_crc, t_info = torch.from_numpy(h_hdr), torch.from_numpy(h_crc), torch.from_numpy(h_info)
        copies = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t_log.copy_(log)
            t_hdr.copy_(hdr[:frags])
            t_crc.copy_(crc[:frags])
            t_info.copy_(info[:frags])
            torch.cuda.synchronize()
            copies.append((time.perf_counter() - t0) * 1e3)
        copy_ms = min(copies)
        sc = LW.Scan.from_arrays(h_hdr.view(np.uint64), h_crc.view(np.uint32), h_info.view(np.uint32))
        R = ctypes.CDLL(os.path.join(ROOT, "leveldb-rs_amd", "lib", "libhostreplay.so"))
        R.lv_replay_reader.restype = ctypes.c_double
        R.lv_replay_reader.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        nr, nb = ctypes.c_uint64(), ctypes.c_uint64()
        drain_s = R.lv_replay_reader(h_log.ctypes.data, need, sc._h, 5, ctypes.byref(nr), ctypes.byref(nb))
        if drain_s < 0 or nr.value != ln.size or nb.value != tot:
            raise SystemExit(f"host reader replay failed: {drain_s} s, {nr.value} records, {nb.value} bytes")
        host = {"copy_ms": round(copy_ms, 3), "reader_drain_ms": round(drain_s * 1e3, 3),
                "ms": round(copy_ms + drain_s * 1e3, 3), "ms_with_scan": round(scan_ms + copy_ms + drain_s * 1e3, 3),
                "note": "D2H of the log and the scan arrays into page-locked memory + lv_wal_reader drained natively"}

    kernel_us, kernel_note = (None, "off") if args.no_split else kernel_split(args.mib, args.keep_stats)
    moved = need + tot
    res = {"tool": "wal_decode_bench", "api": "lv_wal_decode_device", "records": int(ln.size), "fragments": frags,
           "payload_bytes": int(tot), "log_bytes": int(need), "steps": args.steps, "warmup": args.warmup,
           "scan_decode_ms": round(both_ms, 4), "scan_decode_ms_min": round(both_min, 4),
           "scan_decode_ms_max": round(both_max, 4),
           "decode_ms": round(dec_ms, 4), "decode_ms_min": round(dec_min, 4), "decode_ms_max": round(dec_max, 4),
           "scan_ms": round(scan_ms, 4),
           "decode_gib_s": round(need / 2**30 / (dec_ms / 1e3), 1),
           "scan_decode_gib_s": round(need / 2**30 / (both_ms / 1e3), 1),
           "kernel_us": kernel_us, "kernel_us_note": kernel_note,
           "unframe_kernel_us": kernel_us["lvk::wal_unframe_kernel"] if kernel_us else None,
           "unframe_frac_of_8TBs": round((need + tot) / (kernel_us["lvk::wal_unframe_kernel"] * 1e-6) / HBM_PEAK, 4)
           if kernel_us else None,
           "bytes_moved": int(moved), "bytes_moved_note": "the log read once + the records written once",
           "decode_frac_of_8TBs": round(moved / (dec_ms / 1e3) / HBM_PEAK, 4),
           "host_route": host,
           "speedup_vs_host_route": round(host["ms_with_scan"] / both_ms, 1) if host else None}
    print(json.dumps(res))
    if host and not both_ms < host["ms_with_scan"]:
        raise SystemExit("scan_device + decode_device is not faster than the host route")


if __name__ == "__main__":
    main()
