#!/usr/bin/env python3
"""lv_version_get_device: point lookups over the tables of a version in HBM.
One JSON line per key set and filter setting.

    python tools/bench_version_get.py                  # about 64 MiB, 2^20 queries
    python tools/bench_version_get.py --l2-entries 1000 --nq 65536   # a quick look

The version: --l0 overlapping level-0 tables, --l1 tables on level 1 and --l2
on level 2 (defaults 4 / 10 / 100), 16-byte "user" keys and 100-byte values,
built on the device by lv_memtable_build_device and lv_sst_build_bloom_device
(bits_per_key 10, default options) and copied into one arena.  Level 2 holds
every key of the key space, range-partitioned; level 1 a random fifth of them
at newer sequences, range-partitioned; each level-0 table random keys of the
whole range at the newest sequences.  The descriptors are made on the device
(lv_sst_open_device, lv_sst_bloom_open_device, lv_version_file_device,
lv_version_open_device).

Key sets: "present", --nq keys drawn uniformly from the key space; "absent",
the same keys with their last two bytes replaced by two no stored key ends in
(inside the files' ranges, in no table); each "random" and "sorted" (bytewise order:
neighbouring lanes take neighbouring paths).  All at the newest snapshot, with
and without the filters.

Timed per call, by HIP events on the launch stream after a warm-up (median of
--steps): "version_get_ms", the one lv_version_get_device launch; "per_file_ms",
the only route without it: one lv_sst_get_bloom_device (lv_sst_get_device
without filters) launch per file over all queries, each into a result array of
its own; the pick among those arrays, for which the C ABI has no kernel, is not
timed, so this is a lower bound of that route; "single_table_ms", the floor:
one lv_sst_get_bloom_device over a single table that holds all entries.  Before
anything is reported every status and tag of the version get is compared with
the single table's (the union rule) and with the first answer in d_files order
among the per-file results."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "leveldb-rs_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_memtable import event_ms  # noqa: E402

KEY, VAL = 16, 100


def key_rows(np, ids):
    """ids -> uint8 [n, 16]: b"user" and twelve decimal digits."""
    rows = np.empty((ids.size, KEY), dtype=np.uint8)
    rows[:, :4] = np.frombuffer(b"user", dtype=np.uint8)
    rows[:, 4:] = (ids[:, None] // 10 ** np.arange(11, -1, -1, dtype=np.int64)[None, :]) % 10 + 48
    return rows


def build_table(np, torch, dev, ids, seq0, bloom=10):
    """The image of one table over keys `ids` at sequences seq0 + j, built on
    the device: (BuiltBloom, totals dict)."""
    import lvgpu.memtable as MT
    import lvgpu.table as T
    import lvgpu.write_batch as WB
    n = ids.size
    rows = np.empty((n, KEY + VAL), dtype=np.uint8)
    rows[:, :KEY] = key_rows(np, ids)
    rows[:, KEY:] = (ids[:, None] + np.arange(VAL)[None, :]) % 251
    ops = np.zeros(n, dtype=WB.OP_DTYPE)
    ops["tag"] = ((seq0 + np.arange(n, dtype=np.uint64)) << np.uint64(8)) | np.uint64(1)
    ops["key_off"] = np.arange(n, dtype=np.uint64) * (KEY + VAL)
    ops["val_off"] = ops["key_off"] + KEY
    ops["key_len"], ops["val_len"] = KEY, VAL
    d_pay = torch.from_numpy(rows.reshape(-1)).to(dev)
    d_ops = torch.from_numpy(ops.view(np.uint8)).to(dev)
    table = MT.build_device(d_pay, d_ops, torch.tensor([n], dtype=torch.int64, device=dev), op_cap=n)
    built = T.build_bloom_device(table, bloom, block_cap=n // 8 + 8)
    return built, built.sync_totals()


def run(args):
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.memtable as MT
    import lvgpu.table as T
    import lvgpu.version as V

    dev = torch.device("cuda:0")
    lvgpu.device_init()
    rng = np.random.default_rng(15)
    space = args.l2 * args.l2_entries
    specs, seq = [], 1  # (level, number, ids, seq0), oldest first
    for i in range(args.l2):
        ids = np.arange(i * args.l2_entries, (i + 1) * args.l2_entries, dtype=np.int64)
        specs.append((2, len(specs) + 1, ids, seq))
        seq += ids.size
    l1 = np.sort(rng.choice(space, size=max(space // 5 // 10 * 10, args.l1), replace=False))
    for part in np.array_split(l1, args.l1):
        specs.append((1, len(specs) + 1, part, seq))
        seq += part.size
    for i in range(args.l0):
        ids = rng.choice(space, size=max(space // 40, 1), replace=False)
        specs.append((0, len(specs) + 1, ids, seq))
        seq += ids.size
    # d_files order: level ascending, level 0 newest first, the others in key order
    order = sorted(range(len(specs)), key=lambda j: (specs[j][0], -specs[j][1] if specs[j][0] == 0 else int(specs[j][2][0])))
    images, placed, entries = [], [], 0
    at = 0
    for j in order:
        level, number, ids, seq0 = specs[j]
        built, tot = build_table(np, torch, dev, ids, seq0)
        fb = tot["file_bytes"]
        images.append(built.file_t[:fb].clone())
        placed.append((at, fb, level, number))
        at += (fb + 15) & ~15
        entries += ids.size
    arena = torch.zeros(at, dtype=torch.uint8, device=dev)
    for (off, fb, _, _), img in zip(placed, images):
        arena[off:off + fb].copy_(img)
    del images
    n = len(placed)
    tables_t = torch.zeros(8 * n, dtype=torch.int64, device=dev)
    blooms_t = torch.zeros(8 * n, dtype=torch.int64, device=dev)
    files_t = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
    bounds_t = torch.zeros(2 * (KEY + 8) * n, dtype=torch.uint8, device=dev)
    used_t = torch.zeros(1, dtype=torch.int64, device=dev)
    opened_files = []
    for f, (off, fb, level, number) in enumerate(placed):
        op = T.open_device(arena[off:off + fb], torch.tensor([fb], dtype=torch.int64, device=dev), None, handles=False,
                           table=tables_t[8 * f:8 * f + 8])
        T.bloom_open_device(op, bloom=blooms_t[8 * f:8 * f + 8])
        V.file_device(arena, at, off, fb, tables_t[8 * f:8 * f + 8], number, level, bounds_t, bounds_t.numel(), used_t,
                      files_t[64 * f:64 * f + 64])
        opened_files.append(op)
    opened = V.open_device(arena, files_t, tables_t, n, bounds_t, blooms_t=blooms_t)
    version = opened.sync()
    if any(int(s) for s in opened.files()["status"]):
        raise SystemExit("lv_version_file_device reported a status")
    # the floor: one table with every entry
    all_ids = np.concatenate([s[2] for s in specs])
    single, single_tot = build_table(np, torch, dev, all_ids, 1)
    sfb = single_tot["file_bytes"]
    single_op = T.open_device(single.file_t[:sfb], single.totals[2:3], single.totals[7:8], handles=False)
    single_bloom = T.bloom_open_device(single_op)
    single_op.sync()

    pick = rng.integers(0, space, size=args.nq)
    keys = key_rows(np, pick)
    absent = keys.copy()
    absent[:, KEY - 2:] = np.frombuffer(b"xy", dtype=np.uint8)  # two bytes: see DESIGN §8, "Bloom filter blocks", finding (2)
    sets = {}
    for name, k in (("present", keys), ("absent", absent)):
        sets[name + "/random"] = k
        sets[name + "/sorted"] = k[np.lexsort(k.T[::-1])]
    q_off = torch.arange(args.nq, dtype=torch.int64, device=dev) * KEY
    q_len = torch.full((args.nq,), KEY, dtype=torch.int32, device=dev)
    q_seq = torch.full((args.nq,), MT.MAX_SEQUENCE, dtype=torch.int64, device=dev)
    per_file_res = [torch.empty(args.nq * 32, dtype=torch.uint8, device=dev) for _ in range(n)]
    res = torch.empty(args.nq * 48, dtype=torch.uint8, device=dev)
    sres = torch.empty(args.nq * 32, dtype=torch.uint8, device=dev)
    keep = {}
    for kind in args.keys.split(","):
        d_qk = torch.from_numpy(np.ascontiguousarray(sets[kind]).reshape(-1)).to(dev)
        for bloom in (True, False):
            def version_get():
                keep["v"] = V.get_device(opened, d_qk, q_off, q_len, q_seq, nq=args.nq, res=res, bloom=bloom)

            def per_file():
                for f, op in enumerate(opened_files):
                    if bloom:
                        T.get_bloom_device(op, blooms_t[8 * f:8 * f + 8], d_qk, q_off, q_len, q_seq, nq=args.nq,
                                           res=per_file_res[f])
                    else:
                        T.get_device(op, d_qk, q_off, q_len, q_seq, nq=args.nq, res=per_file_res[f])

            def single_get():
                if bloom:
                    keep["s"] = T.get_bloom_device(single_op, single_bloom, d_qk, q_off, q_len, q_seq, nq=args.nq, res=sres)
                else:
                    keep["s"] = T.get_device(single_op, d_qk, q_off, q_len, q_seq, nq=args.nq, res=sres)

            v_ms = event_ms(torch, version_get, args.steps, args.warmup)
            p_ms = event_ms(torch, per_file, args.steps, args.warmup)
            s_ms = event_ms(torch, single_get, args.steps, args.warmup)
            got = keep["v"].sync()
            sgot = keep["s"].sync()
            for field in ("status", "tag"):
                if not np.array_equal(got[field], sgot[field]):
                    bad = int(np.nonzero(got[field] != sgot[field])[0][0])
                    raise SystemExit(f"{kind}: query {bad}: version {got[bad]} vs the single table {sgot[bad]}")
            # the pick the per-file route would need: the first answer in d_files order
            first = np.zeros(args.nq, dtype=T.GET_DTYPE)
            open_q = np.ones(args.nq, dtype=bool)
            for f in range(n):
                r = per_file_res[f].cpu().numpy().view(T.GET_DTYPE)
                take = open_q & (r["status"] != T.GET_ABSENT)
                first[take] = r[take]
                open_q &= ~take
            if not (np.array_equal(first["status"], got["status"]) and np.array_equal(first["tag"], got["tag"])):
                raise SystemExit(f"{kind}: the per-file route's first answers differ from the version get's")
            reads = int(got["files_read"].sum())
            out = {"tool": "bench_version_get", "api": "lv_version_get_device", "keys": kind, "filters": bloom,
                   "steps": args.steps, "warmup": args.warmup, "files": n, "levels": [args.l0, args.l1, args.l2],
                   "entries": int(entries), "images_MiB": round(at / 2**20, 1), "nq": args.nq,
                   "level_start": version["level_start"],
                   "statuses": {int(s): int(c) for s, c in zip(*np.unique(got["status"], return_counts=True))},
                   "version_get_ms": round(v_ms[0], 4), "version_get_ms_min": round(v_ms[1], 4),
                   "version_get_ms_max": round(v_ms[2], 4), "Mget_per_s": round(args.nq / v_ms[0] / 1e3, 1),
                   "per_file_ms": round(p_ms[0], 4), "per_file_ms_min": round(p_ms[1], 4),
                   "single_table_ms": round(s_ms[0], 4), "single_table_ms_min": round(s_ms[1], 4),
                   "per_file_over_version": round(p_ms[0] / v_ms[0], 2),
                   "version_over_single_table": round(v_ms[0] / s_ms[0], 2),
                   "mean_files_read": round(reads / args.nq, 3),
                   "filtered_share": round(int(got["filtered"].sum()) / max(reads, 1), 4),
                   "checked": "every status and tag == the single table's and == the first answer among the per-file results"}
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--l0", type=int, default=4)
    ap.add_argument("--l1", type=int, default=10)
    ap.add_argument("--l2", type=int, default=100)
    ap.add_argument("--l2-entries", type=int, default=4000, help="entries of one level-2 table")
    ap.add_argument("--keys", default="present/random,present/sorted,absent/random,absent/sorted")
    ap.add_argument("--nq", type=int, default=1 << 20, help="queries per call")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
