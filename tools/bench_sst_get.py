#!/usr/bin/env python3
"""lv_sst_open_device / lv_sst_get_device: point lookups over a table image in
HBM.  One JSON line per workload and key set.

    python tools/bench_sst_get.py                       # A and B at 64 MiB, 2^20 queries
    python tools/bench_sst_get.py --workloads A --mib 256 --nq 4194304

Workloads, those of tools/bench_memtable.py ("user:" keys, 16 bytes): (A)
single-Put records; (B) 64-op batches; (C) batches of 16 ops with 4 KiB values.
The log is decoded, sorted and flushed on the device (default options); the
image stays where lv_sst_build_device wrote it.

Key sets: "random", --nq keys drawn uniformly from the stored ones; "sorted",
the same keys in bytewise order (neighbouring lanes probe neighbouring blocks);
"absent", the same keys with their last byte replaced by one no stored key
ends in.  All at the newest snapshot.

Timed per call, by HIP events on the launch stream after a warm-up (median of
--steps): "open_ms", lv_sst_open_device with handles; "get_ms",
lv_sst_get_device; "memtable_get_ms", lv_memtable_get_device on the same
query arrays over the op table the image was flushed from (the in-project
comparison: a binary search over fixed-size entries against footer, index
block, data block, entry).  "host_us_per_get": lv_sst_get_host on one core
over --host-nq of the queries, the image copied to host memory once (wall
clock per call, the ctypes call included).  Before anything is reported every
device result of those --host-nq queries is compared with the host twin's,
field for field, and every status with the memtable get's.
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


def run(args, name):
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.memtable as MT
    import lvgpu.table as T
    import lvgpu.write_batch as WB

    dev = torch.device("cuda:0")
    lvgpu.device_init()
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
    size = T.build_device(table, file_cap=0, block_cap=0).sync_totals(check=False)  # a sizing call
    built = T.build_device(table, file_cap=size["file_bytes"], block_cap=size["data_blocks"])
    tot = built.sync_totals()
    file_t = built.file_t[: tot["file_bytes"]]
    keep = {}

    def do_open():
        keep["o"] = T.open_device(file_t, built.totals[2:3], built.totals[7:8], block_cap=tot["data_blocks"])

    open_ms = event_ms(torch, do_open, args.steps, args.warmup)
    opened = keep["o"]
    tab = opened.sync()
    if opened.handles() != built.handles():
        raise SystemExit(f"{name}: the open's handles differ from the build's")
    st = T.verify_blocks(file_t, opened.handles_view())
    if int((st != T.BLOCK_OK).sum()):
        raise SystemExit(f"{name}: lv_sst_verify_blocks_device rejects a block of the open's handles")

    # the key sets: 16-byte keys gathered from the payload
    ops = wops.ops_t[: n_ops * 32].cpu().numpy().view(WB.OP_DTYPE)
    rng = np.random.default_rng(5)
    pick = rng.integers(0, n_ops, size=args.nq)
    keys = payload[(ops["key_off"][pick].astype(np.int64)[:, None] + np.arange(16)[None, :])]
    sets = {"random": keys, "sorted": keys[np.lexsort(keys.T[::-1])], "absent": keys.copy()}
    sets["absent"][:, 15] = ord("x")
    image = file_t.cpu().numpy().tobytes()
    L = T._bind_get()
    htab = T.SstTable(*[tab[f] for f in T.TABLE_FIELDS])
    q_off = torch.arange(args.nq, dtype=torch.int64, device=dev) * 16
    q_len = torch.full((args.nq,), 16, dtype=torch.int32, device=dev)
    q_seq = torch.full((args.nq,), MT.MAX_SEQUENCE, dtype=torch.int64, device=dev)
    for kind in args.keys.split(","):
        kb = np.ascontiguousarray(sets[kind])
        d_qk = torch.from_numpy(kb.reshape(-1)).to(dev)

        def get():
            keep["g"] = T.get_device(opened, d_qk, q_off, q_len, q_seq, nq=args.nq)

        def mget():
            keep["m"] = MT.get_device(table, d_qk, q_off, q_len, q_seq, nq=args.nq)

        get_ms = event_ms(torch, get, args.steps, args.warmup)
        mget_ms = event_ms(torch, mget, args.steps, args.warmup)
        got = keep["g"].sync()
        mgot = MT.results(keep["m"], args.nq)
        if not np.array_equal(got["status"], mgot["status"]):
            bad = int(np.nonzero(got["status"] != mgot["status"])[0][0])
            raise SystemExit(f"{name}/{kind}: query {bad}: table status {got[bad]} vs memtable {mgot[bad]}")
        hn = min(args.host_nq, args.nq)
        r = T.SstGetResult()
        host = np.zeros(hn, dtype=T.GET_DTYPE)
        rows = [kb[i].tobytes() for i in range(hn)]
        t0 = time.perf_counter()
        for i in range(hn):
            L.lv_sst_get_host(image, ctypes.byref(htab), rows[i], 16, MT.MAX_SEQUENCE, ctypes.byref(r))
            host[i] = (r.val_off, r.tag, r.val_len, r.block, r.status, r.reserved)
        host_us = (time.perf_counter() - t0) * 1e6 / max(hn, 1)
        if not np.array_equal(host, got[:hn]):
            bad = int(np.nonzero(host != got[:hn])[0][0])
            raise SystemExit(f"{name}/{kind}: query {bad}: device {got[bad]} vs lv_sst_get_host {host[bad]}")
        statuses = {int(s): int(c) for s, c in zip(*np.unique(got["status"], return_counts=True))}
        out = {"tool": "bench_sst_get", "api": "lv_sst_get_device", "workload": name, "keys": kind, "label": args.label,
               "steps": args.steps, "warmup": args.warmup, "ops": int(n_ops), "nq": args.nq, "table": tab,
               "statuses": statuses, "open_ms": round(open_ms[0], 4), "open_ms_min": round(open_ms[1], 4),
               "get_ms": round(get_ms[0], 4), "get_ms_min": round(get_ms[1], 4), "get_ms_max": round(get_ms[2], 4),
               "Mget_per_s": round(args.nq / get_ms[0] / 1e3, 1),
               "memtable_get_ms": round(mget_ms[0], 4), "memtable_Mget_per_s": round(args.nq / mget_ms[0] / 1e3, 1),
               "host_us_per_get": round(host_us, 3), "host_nq": hn,
               "speedup_vs_one_core": round(host_us * args.nq / 1e3 / get_ms[0], 1),
               "checked": f"first {hn} results == lv_sst_get_host's, every field; every status == lv_memtable_get_device's; "
                          "the open's handles == the build's, verify_blocks OK"}
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="A,B")
    ap.add_argument("--keys", default="random,sorted,absent")
    ap.add_argument("--mib", type=int, default=64, help="payload MiB")
    ap.add_argument("--nq", type=int, default=1 << 20, help="queries per call")
    ap.add_argument("--host-nq", type=int, default=20000, help="queries of the one-core run and the field-for-field check")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="product", help="free text for the line (a variant library's name)")
    args = ap.parse_args()
    for name in args.workloads.split(","):
        run(args, name.strip().upper())


if __name__ == "__main__":
    main()
