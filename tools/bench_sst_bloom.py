#!/usr/bin/env python3
"""Bloom filter blocks: lv_sst_build_bloom_device beside lv_sst_build_device,
and lv_sst_get_bloom_device beside lv_sst_get_device.  One JSON line per
workload for the build and one per workload and key set for the gets.

    python tools/bench_sst_bloom.py                       # A, B and C at 64 MiB, 2^20 queries
    python tools/bench_sst_bloom.py --workloads A --mib 256 --bits-per-key 10

Workloads, those of tools/bench_memtable.py ("user:" keys, 16 bytes): (A)
single-Put records; (B) 64-op batches; (C) batches of 16 ops with 4 KiB values.
The log is decoded and sorted on the device; the same memtable is flushed by
both builds (default options) in the same run.

Build line: "plain_ms" and "bloom_ms", one whole call each by HIP events on the
launch stream after a warm-up (median of --steps; exact capacities from a
sizing call); "kernel_us", every kernel's microseconds per bloom build from a
child run of this tool under `rocprofv3 --kernel-trace --stats` ("sb_emit" is
the entry emit, "sb_bloom_emit" the filter emit).  Before anything is reported
the bloom image's data blocks are compared with the plain image's, all
data_blocks + 3 checksums are verified and the filter block is compared with
lv_sst_build_bloom_host's unless --no-host.

Get lines, key sets of --nq keys at the newest snapshot: "present" (drawn
uniformly from the stored keys), "absent" (the same with the last two bytes
replaced by two no stored key ends in; two, because upstream's hash keeps a
change of a key's last byte alone out of the low bits of h and of its delta,
so such a key probes the same bits of a 64-bit filter, which is what a block
of one entry gets), "half" (alternating), each in "random" order and
"sorted" bytewise.  "plain_get_ms": lv_sst_get_device over the bloom image;
"bloom_get_ms": lv_sst_get_bloom_device.  Every filtered result must be ABSENT
in the plain get and every other result equal to it, field for field, and the
first --host-nq results equal to lv_sst_get_bloom_host's over the image copied
to host memory.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "leveldb-rs_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_memtable import build_log_payload, event_ms  # noqa: E402

KERNELS = ("sb_init", "sb_sizes", "sb_carry", "sb_next", "sb_reach", "sb_layout", "sb_index", "sb_bloom_sizes", "sb_plan",
           "sb_emit", "sb_bloom_emit", "sb_bloom_big", "sb_bloom_offsets", "sb_tail", "sst_blocks_kernel",
           "crc32c_fused_small_kernel", "sb_index_trailer")


def kernel_split(argv):
    """({kernel: us per bloom build call}, note) from a child run under
    rocprofv3 --kernel-trace --stats, or (None, reason)."""
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
    out = tempfile.mkdtemp(prefix="lvgpu_bloom_", dir="/tmp")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "kt", "--", sys.executable,
           os.path.abspath(__file__)] + argv + ["--steps", "5", "--warmup", "2", "--build-only"]
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
    n = calls.get("sb_bloom_emit")
    if not n or calls.get("sb_emit") != n:
        return None, f"the trace does not hold whole bloom builds only: {calls}"
    return ({k: round(tot[k] / 1e3 / n, 2) for k in tot},
            "rocprofv3 --kernel-trace --stats of a --build-only child run: bloom builds only, per call")


def run(args, name, argv):
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.memtable as MT
    import lvgpu.table as T
    import lvgpu.write_batch as WB

    dev = torch.device("cuda:0")
    lvgpu.device_init()
    bpk = args.bits_per_key
    payload, off, ln, nops = build_log_payload(np, name, args.mib, "user")
    n_ops = off.size * nops
    d_pay = torch.from_numpy(payload).to(dev)
    wops = WB.decode_device(d_pay, torch.from_numpy(off.view(np.int64)).to(dev),
                            torch.from_numpy(ln.view(np.int64)).to(dev),
                            torch.tensor([off.size], dtype=torch.int64, device=dev), None, rec_cap=off.size, op_cap=n_ops)
    if wops.sync_totals()["ops"] != n_ops:
        raise SystemExit(f"{name}: {wops.sync_totals()}")
    table = MT.build_device(d_pay, wops.ops_t, wops.totals[1:2].clone(), op_cap=n_ops)
    table.sync_totals()
    bsize = T.build_bloom_device(table, bpk, file_cap=0, block_cap=0).sync_totals(check=False)  # a sizing call
    fcap, bcap = bsize["file_bytes"], bsize["data_blocks"]
    bws = torch.empty(T.build_bloom_workspace_bytes(n_ops, bcap), dtype=torch.uint8, device=dev)
    keep = {}

    def bloom():
        keep["b"] = T.build_bloom_device(table, bpk, file_cap=fcap, block_cap=bcap, workspace=bws)

    if args.build_only:  # the profiled child: bloom builds and nothing else
        event_ms(torch, bloom, args.steps, args.warmup)
        return
    psize = T.build_device(table, file_cap=0, block_cap=0).sync_totals(check=False)
    pws = torch.empty(T.build_workspace_bytes(n_ops, bcap), dtype=torch.uint8, device=dev)

    def plain():
        keep["p"] = T.build_device(table, file_cap=psize["file_bytes"], block_cap=bcap, workspace=pws)

    plain_ms = event_ms(torch, plain, args.steps, args.warmup)
    bloom_ms = event_ms(torch, bloom, args.steps, args.warmup)
    plain_ms2 = event_ms(torch, plain, args.steps, args.warmup)  # again, behind the other: drift shows here
    built, pbuilt = keep["b"], keep["p"]
    tot, btot, ptot = built.sync_totals(), built.sync_bloom_totals(), pbuilt.sync_totals()
    file_t = built.file_t[: tot["file_bytes"]]
    if not torch.equal(file_t[: btot["filter_offset"]], pbuilt.file_t[: ptot["metaindex_offset"]]):
        raise SystemExit(f"{name}: the bloom image's data blocks differ from the plain image's")
    st = T.verify_blocks(file_t, built.handles_view())
    if int((st != T.BLOCK_OK).sum()):
        raise SystemExit(f"{name}: lv_sst_verify_blocks_device rejects a block of the bloom image")
    checked = "data blocks == the plain image's; all data_blocks + 3 checksums OK"
    if not args.no_host:
        order = table.order_t[:n_ops].cpu().numpy().view(np.uint32)
        ops = wops.ops_t[: n_ops * 32].cpu().numpy().view(WB.OP_DTYPE)
        hfile, _, htot, hbtot = T.build_bloom_host(payload.tobytes(), ops, order, table.sync_totals(), bpk)
        if (htot, hbtot) != (tot, btot) or hfile != file_t.cpu().numpy().tobytes():
            raise SystemExit(f"{name}: the device image differs from lv_sst_build_bloom_host's")
        checked += "; the whole image == lv_sst_build_bloom_host's"
    split, note = (None, "not asked for") if args.no_split else kernel_split(argv + ["--workloads", name])
    out = {"tool": "bench_sst_bloom", "api": "lv_sst_build_bloom_device", "workload": name, "label": args.label,
           "steps": args.steps, "warmup": args.warmup, "ops": int(n_ops), "bits_per_key": bpk, "totals": tot,
           "bloom_totals": btot, "plain_file_bytes": ptot["file_bytes"],
           "plain_ms": round(plain_ms[0], 4), "plain_ms_min": round(plain_ms[1], 4), "plain_ms_again": round(plain_ms2[0], 4),
           "bloom_ms": round(bloom_ms[0], 4), "bloom_ms_min": round(bloom_ms[1], 4), "bloom_ms_max": round(bloom_ms[2], 4),
           "bloom_over_plain": round(bloom_ms[0] / plain_ms[0], 4), "kernel_us": split, "kernel_us_note": note,
           "checked": checked}
    print(json.dumps(out), flush=True)

    # ---- the gets ----
    opened = T.open_device(file_t, built.totals[2:3], built.totals[7:8], handles=False)
    bloom_t = T.bloom_open_device(opened)
    bd = T.bloom_dict(bloom_t)
    if opened.sync()["status"] or bd["present"] != 1:
        raise SystemExit(f"{name}: no filter found: {bd}")
    ops = wops.ops_t[: n_ops * 32].cpu().numpy().view(WB.OP_DTYPE)
    rng = np.random.default_rng(5)
    pick = rng.integers(0, n_ops, size=args.nq)
    present = payload[(ops["key_off"][pick].astype(np.int64)[:, None] + np.arange(16)[None, :])]
    absent = present.copy()
    absent[:, 14] = ord("y")
    absent[:, 15] = ord("x")
    half = present.copy()
    half[1::2] = absent[1::2]
    q_off = torch.arange(args.nq, dtype=torch.int64, device=dev) * 16
    q_len = torch.full((args.nq,), 16, dtype=torch.int32, device=dev)
    q_seq = torch.full((args.nq,), MT.MAX_SEQUENCE, dtype=torch.int64, device=dev)
    image = file_t.cpu().numpy().tobytes()
    L = T._bind_bloom()
    htab = T.SstTable(*[opened.sync()[f] for f in T.TABLE_FIELDS])
    hbloom = T.SstBloom(*[bd[f] for f in T.BLOOM_FIELDS])
    hn = min(args.host_nq, args.nq)
    for kind, keys in (("absent", absent), ("present", present), ("half", half)):
        for order_name in ("random", "sorted"):
            kb = np.ascontiguousarray(keys if order_name == "random" else keys[np.lexsort(keys.T[::-1])])
            d_qk = torch.from_numpy(kb.reshape(-1)).to(dev)

            def pget():
                keep["pg"] = T.get_device(opened, d_qk, q_off, q_len, q_seq, nq=args.nq)

            def bget():
                keep["bg"] = T.get_bloom_device(opened, bloom_t, d_qk, q_off, q_len, q_seq, nq=args.nq)

            p_ms = event_ms(torch, pget, args.steps, args.warmup)
            b_ms = event_ms(torch, bget, args.steps, args.warmup)
            p_ms2 = event_ms(torch, pget, args.steps, args.warmup)
            got, base = keep["bg"].sync(), keep["pg"].sync()
            filt = got["reserved"] == T.GET_FILTERED
            if (base["status"][filt] != T.GET_ABSENT).any() or not np.array_equal(got[~filt], base[~filt]):
                raise SystemExit(f"{name}/{kind}/{order_name}: the filtered get disagrees with lv_sst_get_device")
            r = T.SstGetResult()
            host = np.zeros(hn, dtype=T.GET_DTYPE)
            for i in range(hn):
                L.lv_sst_get_bloom_host(image, ctypes.byref(htab), ctypes.byref(hbloom), kb[i].tobytes(), 16,
                                        MT.MAX_SEQUENCE, ctypes.byref(r))
                host[i] = (r.val_off, r.tag, r.val_len, r.block, r.status, r.reserved)
            if not np.array_equal(host, got[:hn]):
                bad = int(np.nonzero(host != got[:hn])[0][0])
                raise SystemExit(f"{name}/{kind}/{order_name}: query {bad}: device {got[bad]} vs lv_sst_get_bloom_host {host[bad]}")
            statuses = {int(s): int(c) for s, c in zip(*np.unique(base["status"], return_counts=True))}
            out = {"tool": "bench_sst_bloom", "api": "lv_sst_get_bloom_device", "workload": name, "keys": kind,
                   "order": order_name, "label": args.label, "steps": args.steps, "warmup": args.warmup, "ops": int(n_ops),
                   "nq": args.nq, "bits_per_key": bpk, "plain_statuses": statuses, "filtered": int(filt.sum()),
                   "plain_get_ms": round(p_ms[0], 4), "plain_get_ms_min": round(p_ms[1], 4),
                   "plain_get_ms_again": round(p_ms2[0], 4),
                   "bloom_get_ms": round(b_ms[0], 4), "bloom_get_ms_min": round(b_ms[1], 4), "bloom_get_ms_max": round(b_ms[2], 4),
                   "bloom_over_plain": round(b_ms[0] / p_ms[0], 4), "Mget_per_s": round(args.nq / b_ms[0] / 1e3, 1),
                   "checked": "every filtered result is ABSENT in lv_sst_get_device; every other result == its, every field; "
                              f"first {hn} results == lv_sst_get_bloom_host's"}
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="A,B,C")
    ap.add_argument("--mib", type=int, default=64, help="payload MiB")
    ap.add_argument("--nq", type=int, default=1 << 20, help="queries per call")
    ap.add_argument("--bits-per-key", type=int, default=10)
    ap.add_argument("--host-nq", type=int, default=20000, help="queries of the field-for-field check against the host twin")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="leave out the comparison with lv_sst_build_bloom_host")
    ap.add_argument("--no-split", action="store_true", help="leave out the rocprofv3 child run")
    ap.add_argument("--build-only", action="store_true", help="bloom builds only (the profiled child run)")
    ap.add_argument("--label", default="product", help="free text for the line (a variant library's name)")
    args = ap.parse_args()
    argv = ["--mib", str(args.mib), "--bits-per-key", str(args.bits_per_key)]
    for name in args.workloads.split(","):
        run(args, name.strip().upper(), argv)


if __name__ == "__main__":
    main()
