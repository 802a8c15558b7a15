#!/usr/bin/env python3
"""lv_write_batch_decode_device against the host route it replaces, on
db_bench's 16-byte keys and 100-byte values.  One JSON line per workload.

    python tools/bench_write_batch.py                       # A-D at ~1 GiB (D: 64 MiB)
    python tools/bench_write_batch.py --workloads A,B --mib 256
    # counters: one per pass, nothing else traced
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT -- \
        python tools/bench_write_batch.py --workloads C --steps 3 --warmup 1 --no-host --no-split

Workloads: (A) single-Put records; (B) 64-op batches; (C) batches of 16 ops
with 4 KiB values, where the walk skips the values; (D) one 64 MiB batch, the
format's serial worst case.

Timed per call, by HIP events on the launch stream after a warm-up (median of
--steps).  "stage_us": the three kernels' mean microseconds per launch from a
child run of this tool under `rocprofv3 --kernel-trace --stats` (nothing else
traced).  "host_route", in the same run: the payload and the offsets copied to
page-locked host memory (wall clock, best of 3), then lv_write_batch_iterate
over every record on one core, writing the same op table (the native loop of
tools/host_replay.c, best of 3).  The device's ops, bounds and totals are
checked against the Python model on the first and last 1,000 records before
anything is reported.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "leveldb-rs_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12  # bytes / s
KERNELS = ("lvk::wb_count", "lvk::wb_tiles", "lvk::wb_emit")


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


def varint(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def batch_template(nops, vlen):
    """One rep of nops Puts of a 16-byte key and a vlen-byte value, sequence 0."""
    entry = bytes([1, 16]) + b"k" * 16 + varint(vlen) + b"v" * vlen
    return (0).to_bytes(8, "little") + nops.to_bytes(4, "little") + entry * nops


def build(np, name, mib):
    """(payload uint8 array, rec_off, rec_len, ops per record) of a workload."""
    nops, vlen = {"A": (1, 100), "B": (64, 100), "C": (16, 4096)}.get(name, (0, 100))
    if name == "D":
        nops = ((min(mib, 64) << 20) - 12) // 119
        n = 1
    rep = np.frombuffer(batch_template(nops, vlen), dtype=np.uint8)
    if name != "D":
        n = max((mib << 20) // rep.size, 1)
    payload = np.tile(rep, n)
    rows = payload.reshape(n, rep.size)
    rows[:, 0:8] = (np.arange(n, dtype="<u8") * nops).view(np.uint8).reshape(n, 8)  # sequence = ops before the record
    # distinct first key byte per record, so that a mixed-up op shows in the check
    rows[:, 14] = (np.arange(n) % 251).astype(np.uint8)
    off = np.arange(n, dtype=np.uint64) * np.uint64(rep.size)
    ln = np.full(n, rep.size, dtype=np.uint64)
    return payload, off, ln, nops


def kernel_split(name, mib):
    """{kernel: mean us per launch} from a child run under rocprofv3
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
    out = tempfile.mkdtemp(prefix="lvgpu_wb_", dir="/tmp")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "kt", "--", sys.executable,
           os.path.abspath(__file__), "--workloads", name, "--mib", str(mib), "--steps", "5", "--warmup", "2",
           "--no-host", "--no-split"]
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
                if k in KERNELS:
                    per[k.replace("lvk::", "")] = round(float(row["AverageNs"]) / 1e3, 2)
    shutil.rmtree(out, ignore_errors=True)
    if len(per) != len(KERNELS):
        return None, "kernels missing from the trace"
    return per, "rocprofv3 --kernel-trace --stats, mean per launch"


def check_ends(np, WB, C, res, payload, off, ln, nops):
    """The first and last 1,000 records against the Python model."""
    n = off.size
    bounds, st, ops = res.record_bounds(), res.statuses(), res.ops()
    for lo, hi in ((0, min(n, 1000)), (max(n - 1000, 0), n)):
        for r in range(lo, hi):
            o, k = int(off[r]), int(ln[r])
            if nops > 100000 and r == 0:  # D: the model walk of one huge record is slow in Python; sample it
                w_st, w_ops = C.OK, None
            else:
                w_st, w_ops, _, _ = C.iterate_ext(payload[o:o + k].tobytes())
            if int(st[r]) != w_st or int(bounds[r + 1] - bounds[r]) != nops:
                raise SystemExit(f"record {r}: status {st[r]} / {w_st}, ops {bounds[r + 1] - bounds[r]} / {nops}")
            got = ops[int(bounds[r]):int(bounds[r + 1])]
            if w_ops is None:
                idx = [0, 1, nops // 2, nops - 1]
                want = [(((r * nops + i) << 8) | 1, o + 12 + 119 * i + 2, o + 12 + 119 * i + 19, 16, 100) for i in idx]
                have = [(int(g["tag"]), int(g["key_off"]), int(g["val_off"]), int(g["key_len"]), int(g["val_len"]))
                        for g in got[idx]]
            else:
                want = [(t, ko + o, vo + o, kl, vl) for t, ko, kl, vo, vl in w_ops]
                have = [(int(g["tag"]), int(g["key_off"]), int(g["val_off"]), int(g["key_len"]), int(g["val_len"]))
                        for g in got]
            if want != have:
                raise SystemExit(f"record {r}: ops differ from the model")


def run(args, name):
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.write_batch as WB
    import write_batch_cases as C

    dev = torch.device("cuda:0")
    lvgpu.device_init()
    payload, off, ln, nops = build(np, name, args.mib)
    n, nbytes = off.size, payload.size
    d_pay = torch.from_numpy(payload).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_len = torch.from_numpy(ln.view(np.int64)).to(dev)
    d_n = torch.tensor([n], dtype=torch.int64, device=dev)
    ws = torch.empty(WB.decode_workspace_bytes(n), dtype=torch.uint8, device=dev)
    op_cap = n * nops
    state = {}

    def call():
        state["r"] = WB.decode_device(d_pay, d_off, d_len, d_n, rec_cap=n, op_cap=op_cap, workspace=ws)

    # the output arrays are allocated once: every later call reuses the caching allocator's blocks
    call()
    res = state["r"]
    t = res.sync_totals()
    want = dict(records=n, ops=n * nops, key_bytes=16 * n * nops, bad_records=0, last_sequence=n * nops - 1, status=0)
    if {k: t[k] for k in want} != want:
        raise SystemExit(f"{name}: totals differ from the input: {t}")
    check_ends(np, WB, C, res, payload, off, ln, nops)

    ms, ms_min, ms_max = event_ms(torch, call, args.steps, args.warmup)

    host = None
    if not args.no_host:
        h_pay = lvgpu.host_alloc(nbytes)
        h_off, h_len = lvgpu.host_alloc(8 * n).view(np.uint64), lvgpu.host_alloc(8 * n).view(np.uint64)
        t_pay, t_off, t_len = torch.from_numpy(h_pay), torch.from_numpy(h_off.view(np.int64)), torch.from_numpy(h_len.view(np.int64))
        copies = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t_pay.copy_(d_pay)
            t_off.copy_(d_off)
            t_len.copy_(d_len)
            torch.cuda.synchronize()
            copies.append((time.perf_counter() - t0) * 1e3)
        copy_ms = min(copies)
        R = ctypes.CDLL(os.path.join(ROOT, "leveldb-rs_amd", "lib", "libhostreplay.so"))
        R.lv_replay_write_batch.restype = ctypes.c_double
        R.lv_replay_write_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        h_ops = np.empty(max(op_cap, 1), dtype=WB.OP_DTYPE)
        tot, bad = ctypes.c_uint64(), ctypes.c_uint64()
        walk_s = R.lv_replay_write_batch(h_pay.ctypes.data, h_off.ctypes.data, h_len.ctypes.data, n, h_ops.ctypes.data,
                                         op_cap, 3, ctypes.byref(tot), ctypes.byref(bad))
        if walk_s < 0 or tot.value != n * nops or bad.value:
            raise SystemExit(f"{name}: host walk failed: {walk_s} s, {tot.value} ops, {bad.value} bad")
        dev_ops = res.ops()
        if not (np.array_equal(dev_ops[:1000], h_ops[:1000]) and np.array_equal(dev_ops[-1000:], h_ops[op_cap - 1000:op_cap])):
            raise SystemExit(f"{name}: the host route's ops differ from the device's")
        host = {"copy_ms": round(copy_ms, 3), "iterate_ms": round(walk_s * 1e3, 3),
                "ms": round(copy_ms + walk_s * 1e3, 3),
                "note": "D2H of payload and offsets into page-locked memory + lv_write_batch_iterate on one core"}

    stage_us, stage_note = (None, "off") if args.no_split else kernel_split(name, args.mib)
    out = {"tool": "bench_write_batch", "api": "lv_write_batch_decode_device", "workload": name, "records": int(n),
           "ops": int(n * nops), "payload_bytes": int(nbytes), "steps": args.steps, "warmup": args.warmup,
           "ms": round(ms, 4), "ms_min": round(ms_min, 4), "ms_max": round(ms_max, 4),
           "stage_us": stage_us, "stage_us_note": stage_note,
           "ops_per_s": round(n * nops / (ms / 1e3)), "payload_gib_s": round(nbytes / 2**30 / (ms / 1e3), 1),
           "frac_of_8TBs_by_payload": round(nbytes / (ms / 1e3) / HBM_PEAK, 4),
           "wb_small": WB.WB_SMALL, "wb_window": WB.WB_WINDOW,
           "host_route": host, "speedup_vs_host_route": round(host["ms"] / ms, 1) if host else None,
           "checked": "ops, bounds, statuses of the first and last 1,000 records == the Python model"}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="A,B,C,D")
    ap.add_argument("--mib", type=int, default=1024, help="payload MiB of A-C (D: at most 64)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="leave out the host route (counter runs)")
    ap.add_argument("--no-split", action="store_true", help="leave out the kernel-trace child run")
    args = ap.parse_args()
    for name in args.workloads.split(","):
        run(args, name.strip().upper())


if __name__ == "__main__":
    main()
