#!/usr/bin/env python3
"""lv_memtable_build_device against the host route it replaces.  One JSON line
per workload and key style.

    python tools/bench_memtable.py                          # A-C at ~1 GiB, both key styles, and W
    python tools/bench_memtable.py --workloads A --keys user --mib 256
    python tools/bench_memtable.py --workloads W --worst-ops 1048576

Workloads, those of tools/bench_write_batch.py: (A) single-Put records; (B)
64-op batches; (C) batches of 16 ops with 4 KiB values; 16-byte keys, either
random bytes ("random") or "user:" and eleven random digits ("user"), where the
8-byte prefix of a sort entry ties on every comparison.  (W) the serial worst
case: --worst-ops ops of one identical 4 KiB key, every comparison decided by
the tag after 4 KiB of equal bytes on both sides.

Timed per call, by HIP events on the launch stream after a warm-up (median of
--steps): "build_ms", lv_memtable_build_device alone over the op table in HBM;
"chain_ms", lv_wal_scan_device -> lv_wal_decode_device ->
lv_write_batch_decode_device -> lv_memtable_build_device over the log in HBM;
"get_ms", lv_memtable_get_device for --queries stored keys.  "host_route", in
the same run: the op table and the payload copied to page-locked host memory
(wall clock, best of 3), then lv_memtable_build_host on one core (wall clock,
one run).  The device order is checked against the host twin's, entry by entry,
before anything is reported.
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


def make_keys(np, rng, count, style):
    """count 16-byte keys as a (count, 16) uint8 array."""
    if style == "random":
        return rng.integers(0, 256, size=(count, 16), dtype=np.uint8)
    keys = np.empty((count, 16), dtype=np.uint8)
    keys[:, :5] = np.frombuffer(b"user:", dtype=np.uint8)
    v = rng.integers(0, 10**11, size=count, dtype=np.int64)
    for d in range(11):
        keys[:, 15 - d] = (v % 10 + 48).astype(np.uint8)
        v //= 10
    return keys


def build_log_payload(np, name, mib, style, seed=1):
    """(payload, rec_off, rec_len, ops per record) of workload A, B or C with
    the keys filled in."""
    nops, vlen = {"A": (1, 100), "B": (64, 100), "C": (16, 4096)}[name]
    entry = bytes([1, 16]) + b"k" * 16 + varint(vlen) + b"v" * vlen
    rep = np.frombuffer((0).to_bytes(8, "little") + nops.to_bytes(4, "little") + entry * nops, dtype=np.uint8)
    n = max((mib << 20) // rep.size, 1)
    payload = np.tile(rep, n)
    rows = payload.reshape(n, rep.size)
    rows[:, 0:8] = (np.arange(n, dtype="<u8") * nops).view(np.uint8).reshape(n, 8)
    keys = make_keys(np, np.random.default_rng(seed), n * nops, style).reshape(n, nops, 16)
    for i in range(nops):
        at = 12 + i * len(entry) + 2
        rows[:, at:at + 16] = keys[:, i, :]
    off = np.arange(n, dtype=np.uint64) * np.uint64(rep.size)
    ln = np.full(n, rep.size, dtype=np.uint64)
    return payload, off, ln, nops


def host_route(np, torch, lvgpu, MT, d_pay, d_ops_t, n_ops, dev_order):
    """Copy-back and lv_memtable_build_host; checks the device order."""
    L = MT._bind()
    nbytes = d_pay.numel()
    h_pay, h_ops = lvgpu.host_alloc(max(nbytes, 1)), lvgpu.host_alloc(max(n_ops * 32, 1))
    t_pay, t_ops = torch.from_numpy(h_pay), torch.from_numpy(h_ops)
    copies = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t_pay[:nbytes].copy_(d_pay)
        t_ops[: n_ops * 32].copy_(d_ops_t[: n_ops * 32])
        torch.cuda.synchronize()
        copies.append((time.perf_counter() - t0) * 1e3)
    order = np.empty(max(n_ops, 1), dtype=np.uint32)
    tot = MT.Totals()
    t0 = time.perf_counter()
    rc = L.lv_memtable_build_host(h_pay.ctypes.data, nbytes, h_ops.ctypes.data, n_ops, order.ctypes.data,
                                  ctypes.byref(tot))
    sort_ms = (time.perf_counter() - t0) * 1e3
    if rc or tot.status:
        raise SystemExit(f"host build failed: rc {rc}, status {tot.status}")
    if not np.array_equal(order[:n_ops], dev_order):
        bad = int(np.nonzero(order[:n_ops] != dev_order)[0][0])
        raise SystemExit(f"the device order differs from the host twin's at entry {bad}")
    return {"copy_ms": round(min(copies), 3), "sort_ms": round(sort_ms, 3), "ms": round(min(copies) + sort_ms, 3),
            "user_keys": int(tot.user_keys),
            "note": "D2H of payload and op table into page-locked memory + lv_memtable_build_host on one core"}


def report(args, name, style, extra):
    import lvgpu.memtable as MT
    out = {"tool": "bench_memtable", "api": "lv_memtable_build_device", "workload": name, "keys": style,
           "label": args.label, "mt_tile": args.tile or MT.MT_TILE, "mt_prefix": args.prefix or MT.MT_PREFIX,
           "steps": args.steps, "warmup": args.warmup}
    out.update(extra)
    print(json.dumps(out), flush=True)


def run_log(args, name, style):
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.memtable as MT
    import lvgpu.wal as LW
    import lvgpu.write_batch as WB

    dev = torch.device("cuda:0")
    lvgpu.device_init()
    payload, off, ln, nops = build_log_payload(np, name, args.mib, style)
    n, n_ops = off.size, off.size * nops
    d_src = torch.from_numpy(payload).to(dev)
    need, frags = LW.encode_size(ln)
    log_t = LW.encode_device(d_src, off, ln)
    torch.cuda.synchronize()
    del d_src
    cap = frags + 8
    keep = {}

    def chain():
        scan = LW.scan_device(log_t, cap)
        dec = LW.decode_device(log_t, *scan, scan_cap=cap, reports=False)
        wops = WB.decode_device(dec.payload, dec.rec_off, dec.rec_len, dec.totals[0:1], dec.totals[4:5], rec_cap=cap,
                                op_cap=n_ops)
        keep["t"] = MT.build_device(dec.payload, wops.ops_t, wops.totals[1:2], wops.totals[6:7], op_cap=n_ops,
                                    workspace=ws)
        keep["dec"], keep["wops"] = dec, wops

    ws = torch.empty(MT.build_workspace_bytes(n_ops), dtype=torch.uint8, device=dev)
    chain()
    table, dec, wops = keep["t"], keep["dec"], keep["wops"]
    tot = table.sync_totals()
    if tot["entries"] != n_ops:
        raise SystemExit(f"{name}: {tot}")
    d_pay, d_ops_t, d_n = dec.payload, wops.ops_t, wops.totals[1:2].clone()

    def build():
        keep["b"] = MT.build_device(d_pay, d_ops_t, d_n, op_cap=n_ops, workspace=ws)

    build_ms = event_ms(torch, build, args.steps, args.warmup)
    dev_order = keep["b"].order()
    chain_ms = event_ms(torch, chain, args.steps, args.warmup)
    # lookups of stored keys at the newest snapshot
    nq = min(args.queries, n_ops)
    rng = np.random.default_rng(5)
    pick = torch.from_numpy(rng.integers(0, n_ops, size=nq).astype(np.int64)).to(dev)
    ops64 = d_ops_t[: n_ops * 32].view(torch.int64).view(-1, 4)
    q_off = ops64[pick, 1].contiguous()
    q_len = torch.full((nq,), 16, dtype=torch.int32, device=dev)
    q_seq = torch.full((nq,), MT.MAX_SEQUENCE, dtype=torch.int64, device=dev)
    res = {}

    def get():
        res["r"] = MT.get_device(keep["b"], d_pay, q_off, q_len, q_seq, nq=nq)

    get_ms = event_ms(torch, get, args.steps, args.warmup)
    found = MT.results(res["r"], nq)["status"]
    if not (found == MT.GET_FOUND).all():
        raise SystemExit(f"{name}: a stored key was not found")
    host = None if args.no_host else host_route(np, torch, lvgpu, MT, d_pay, d_ops_t, n_ops, dev_order)
    report(args, name, style, {
        "records": int(n), "ops": int(n_ops), "payload_bytes": int(payload.size), "user_keys": tot["user_keys"],
        "build_ms": round(build_ms[0], 4), "build_ms_min": round(build_ms[1], 4), "build_ms_max": round(build_ms[2], 4),
        "chain_ms": round(chain_ms[0], 4), "chain_ms_min": round(chain_ms[1], 4), "chain_ms_max": round(chain_ms[2], 4),
        "get_queries": nq, "get_ms": round(get_ms[0], 4),
        "ops_per_s": round(n_ops / (build_ms[0] / 1e3)), "host_route": host,
        "build_speedup_vs_host_route": round(host["ms"] / build_ms[0], 2) if host else None,
        "build_speedup_vs_host_sort_alone": round(host["sort_ms"] / build_ms[0], 2) if host else None,
        "checked": None if args.no_host else "d_order == lv_memtable_build_host's, every entry"})


def run_worst(args):
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.memtable as MT
    import lvgpu.write_batch as WB

    dev = torch.device("cuda:0")
    lvgpu.device_init()
    n_ops, klen = args.worst_ops, 4096
    key = np.random.default_rng(9).integers(0, 256, size=klen, dtype=np.uint8)
    payload = np.tile(key, n_ops)
    ops = np.zeros(n_ops, dtype=WB.OP_DTYPE)
    ops["tag"] = (np.random.default_rng(10).permutation(n_ops).astype(np.uint64) << np.uint64(8)) | np.uint64(1)
    ops["key_off"] = np.arange(n_ops, dtype=np.uint64) * np.uint64(klen)
    ops["val_off"] = ops["key_off"] + np.uint64(klen)
    ops["key_len"] = klen
    d_pay = torch.from_numpy(payload).to(dev)
    d_ops_t = torch.from_numpy(ops.view(np.uint8)).to(dev)
    d_n = torch.tensor([n_ops], dtype=torch.int64, device=dev)
    ws = torch.empty(MT.build_workspace_bytes(n_ops), dtype=torch.uint8, device=dev)
    keep = {}

    def build():
        keep["b"] = MT.build_device(d_pay, d_ops_t, d_n, op_cap=n_ops, workspace=ws)

    build_ms = event_ms(torch, build, max(args.steps // 5, 1), 1)
    tot = keep["b"].sync_totals()
    if tot != dict(entries=n_ops, user_keys=1, status=0):
        raise SystemExit(f"W: {tot}")
    host = None if args.no_host else host_route(np, torch, lvgpu, MT, d_pay, d_ops_t, n_ops, keep["b"].order())
    report(args, "W", "one 4 KiB key", {
        "ops": int(n_ops), "payload_bytes": int(payload.size), "build_ms": round(build_ms[0], 3),
        "build_ms_min": round(build_ms[1], 3), "build_ms_max": round(build_ms[2], 3), "host_route": host,
        "build_speedup_vs_host_route": round(host["ms"] / build_ms[0], 3) if host else None,
        "build_speedup_vs_host_sort_alone": round(host["sort_ms"] / build_ms[0], 3) if host else None,
        "checked": None if args.no_host else "d_order == lv_memtable_build_host's, every entry"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="A,B,C,W")
    ap.add_argument("--keys", default="random,user")
    ap.add_argument("--mib", type=int, default=1024, help="payload MiB of A-C")
    ap.add_argument("--worst-ops", type=int, default=1 << 20, help="ops of W")
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="leave out the host route and the check against it")
    ap.add_argument("--label", default="product", help="free text for the line (a variant library's name)")
    ap.add_argument("--tile", type=int, default=0, help="LVK_MT_TILE of the loaded library, if it is a variant")
    ap.add_argument("--prefix", type=int, default=0, help="LVK_MT_PREFIX of the loaded library, if it is a variant")
    args = ap.parse_args()
    for name in args.workloads.split(","):
        name = name.strip().upper()
        if name == "W":
            run_worst(args)
        else:
            for style in args.keys.split(","):
                run_log(args, name, style.strip())


if __name__ == "__main__":
    main()
