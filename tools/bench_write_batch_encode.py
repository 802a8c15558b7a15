#!/usr/bin/env python3
"""lv_write_batch_encode_device against the host route it replaces and the
copy it cannot beat, on db_bench's 16-byte keys and 100-byte values.  One JSON
line per workload.

    python tools/bench_write_batch_encode.py                     # A-D, ~1 GiB of output (D: 64 MiB)
    python tools/bench_write_batch_encode.py --workloads A,B --mib 256

Workloads, as in tools/bench_write_batch.py: (A) single-Put records; (B) 64-op
batches; (C) batches of 16 ops with 4 KiB values; (D) one record holding a
single 64 MiB value, the stage's serial worst case (one group of lanes copies
it).

Timed per call, by HIP events on the launch stream after a warm-up (median of
--steps).  "stage_us": the five kernels' mean microseconds per launch from a
child run of this tool under `rocprofv3 --kernel-trace --stats` (nothing else
traced).  Beside it, in the same run: "host_route", the only route without this
entry point -- the arena, the ops and the bounds copied to page-locked host
memory, lv_write_batch_encode_host on one core, the reps copied back (wall
clock, best of 3 each) --, and "d2d_ms", a device-to-device copy of out_bytes,
the floor.  Before anything is reported the device's bytes, record arrays and
op table are compared whole with the host twin's.
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
KERNELS = ("lvk::we_validate", "lvk::we_size", "lvk::we_carry", "lvk::we_records", "lvk::we_emit")


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


def build(np, OP_DTYPE, name, mib):
    """(arena uint8 array, ops, rec_op) of a workload: every op a Put whose key
    and value lie one after the other in the arena."""
    per, klen, vlen = {"A": (1, 16, 100), "B": (64, 16, 100), "C": (16, 16, 4096), "D": (1, 16, min(mib, 64) << 20)}[name]
    vi = 1 if vlen < 128 else 2 if vlen < 16384 else 3 if vlen < (1 << 21) else 4
    entry = 1 + 1 + klen + vi + vlen
    n = 1 if name == "D" else max((mib << 20) // (12 + per * entry), 1)
    nops = n * per
    rng = np.random.default_rng(12)
    arena = rng.integers(0, 256, size=nops * (klen + vlen), dtype=np.uint8)
    at = np.arange(nops, dtype=np.uint64) * np.uint64(klen + vlen)
    ops = np.zeros(nops, dtype=OP_DTYPE)
    ops["tag"], ops["key_off"], ops["key_len"], ops["val_off"], ops["val_len"] = 1, at, klen, at + np.uint64(klen), vlen
    rec_op = np.arange(n + 1, dtype=np.uint64) * np.uint64(per)
    return arena, ops, rec_op


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
    out = tempfile.mkdtemp(prefix="lvgpu_we_", dir="/tmp")
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


def run(args, name):
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.write_batch as WB

    dev = torch.device("cuda:0")
    lvgpu.device_init()
    arena, ops, rec_op = build(np, WB.OP_DTYPE, name, args.mib)
    n, nops = rec_op.size - 1, ops.size
    first = 1000
    d_src = torch.from_numpy(arena).to(dev)
    d_ops = torch.from_numpy(ops.view(np.uint8)).to(dev)
    d_rec_op = torch.from_numpy(rec_op.view(np.int64)).to(dev)
    d_n = torch.tensor([n], dtype=torch.int64, device=dev)
    ws = torch.empty(max(WB.encode_workspace_bytes(n, nops), 16), dtype=torch.uint8, device=dev)
    out_cap = WB.encode_bound(n, nops, int(ops["key_len"].sum(dtype=np.uint64)), int(ops["val_len"].sum(dtype=np.uint64)))
    d_out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    state = {}

    def call():
        state["r"] = WB.encode_device(d_src, d_ops, d_rec_op, d_n, first_sequence=first, rec_cap=n, op_cap=nops,
                                      out=d_out, workspace=ws)

    call()  # the record and op arrays are allocated once: every later call reuses the caching allocator's blocks
    res = state["r"]
    t = res.sync_totals()
    out_bytes = t["out_bytes"]
    if (t["records"], t["ops"], t["last_sequence"]) != (n, nops, first - 1 + nops) or out_bytes > out_cap:
        raise SystemExit(f"{name}: totals differ from the input: {t}")

    ms, ms_min, ms_max = event_ms(torch, call, args.steps, args.warmup)
    d_copy = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    d2d_ms, _, _ = event_ms(torch, lambda: d_copy.copy_(d_out[:out_bytes]), args.steps, args.warmup)

    # the host twin over the same table: the reference for the whole output, and the host route's middle step
    L = WB._bind()
    h_src, h_ops = lvgpu.host_alloc(arena.size), lvgpu.host_alloc(ops.size * 32)
    h_rec_op = lvgpu.host_alloc(rec_op.size * 8)
    h_out = lvgpu.host_alloc(out_bytes)
    t_src, t_ops, t_rec_op, t_out = (torch.from_numpy(a) for a in (h_src, h_ops, h_rec_op, h_out))
    copies = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t_src.copy_(d_src)
        t_ops.copy_(d_ops)
        t_rec_op.copy_(d_rec_op.view(torch.uint8))
        torch.cuda.synchronize()
        copies.append((time.perf_counter() - t0) * 1e3)
    h_off, h_len = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    h_ops_out = np.zeros(nops, dtype=WB.OP_DTYPE)
    tot = WB.EncodeTotals()
    encodes = []
    for _ in range(1 if args.no_host else 3):
        t0 = time.perf_counter()
        rc = L.lv_write_batch_encode_host(h_src.ctypes.data, h_src.size, h_ops.ctypes.data, nops, h_rec_op.ctypes.data, n,
                                          first, h_out.ctypes.data, out_bytes, h_off.ctypes.data, h_len.ctypes.data,
                                          h_ops_out.ctypes.data, ctypes.byref(tot))
        encodes.append((time.perf_counter() - t0) * 1e3)
        if rc != 0 or tot.status != 0 or tot.out_bytes != out_bytes:
            raise SystemExit(f"{name}: host twin failed: rc {rc}, status {tot.status}, {tot.out_bytes} bytes")
    backs = []
    d_back = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d_back.copy_(t_out)
        torch.cuda.synchronize()
        backs.append((time.perf_counter() - t0) * 1e3)
    if not torch.equal(d_back, d_out[:out_bytes]):
        raise SystemExit(f"{name}: the device's bytes differ from the host twin's")
    if not (np.array_equal(res.rec_off(), h_off) and np.array_equal(res.rec_len(), h_len)
            and np.array_equal(res.ops(), h_ops_out)):
        raise SystemExit(f"{name}: the device's record arrays or op table differ from the host twin's")
    host = None
    if not args.no_host:
        host = {"d2h_ms": round(min(copies), 3), "encode_ms": round(min(encodes), 3), "h2d_ms": round(min(backs), 3),
                "ms": round(min(copies) + min(encodes) + min(backs), 3),
                "note": "D2H of arena, ops and bounds into page-locked memory + lv_write_batch_encode_host on one core "
                        "+ H2D of the reps"}

    stage_us, stage_note = (None, "off") if args.no_split else kernel_split(name, args.mib)
    moved = out_bytes + int(t["key_bytes"]) + int(t["value_bytes"])  # written, and the strings read
    out = {"tool": "bench_write_batch_encode", "api": "lv_write_batch_encode_device", "workload": name,
           "records": int(n), "ops": int(nops), "out_bytes": int(out_bytes), "steps": args.steps, "warmup": args.warmup,
           "ms": round(ms, 4), "ms_min": round(ms_min, 4), "ms_max": round(ms_max, 4),
           "stage_us": stage_us, "stage_us_note": stage_note,
           "ops_per_s": round(nops / (ms / 1e3)), "out_gib_s": round(out_bytes / 2**30 / (ms / 1e3), 1),
           "frac_of_8TBs_by_bytes_moved": round(moved / (ms / 1e3) / HBM_PEAK, 4),
           "d2d_ms": round(d2d_ms, 4), "times_the_d2d_copy": round(ms / d2d_ms, 2),
           "we_tile": WB.WE_TILE, "we_wave_copy": WB.WE_WAVE_COPY, "we_copy_lanes": WB.WE_COPY_LANES,
           "host_route": host, "speedup_vs_host_route": round(host["ms"] / ms, 1) if host else None,
           "checked": "d_out, rec_off, rec_len and d_ops_out whole == lv_write_batch_encode_host"}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="A,B,C,D")
    ap.add_argument("--mib", type=int, default=1024, help="output MiB of A-C (D: one value of at most 64 MiB)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="leave out the host route's timing (profiler runs)")
    ap.add_argument("--no-split", action="store_true", help="leave out the kernel-trace child run")
    args = ap.parse_args()
    for name in args.workloads.split(","):
        run(args, name.strip().upper())


if __name__ == "__main__":
    main()
