#!/usr/bin/env python3
"""lv_version_apply_device against the route a caller has without it: copy the
decoded tables back and run lv_version_apply_host.  One JSON line per shape.

    python tools/bench_version_apply.py                      # both shapes
    python tools/bench_version_apply.py --shapes manifest --log2-edits 10   # a small rehearsal

Shapes: "manifest", 2^16 edits of 30 new files and 30 deleted files each (the
manifest tools/bench_version_edit.py decodes: about 3.9 M rows): every edit
deletes the files of the edit before it, except that every 64th edit's files
stay, so about 30,000 files are live at the end; "snapshot", one record of
2^20 new files on levels 1-6 in the order upstream's WriteSnapshot writes them
(all live: the sort's largest input, ten merge passes).  Keys are 24-byte
internal keys (16-byte user keys), sizes around 2 MiB, and every live file has
a directory entry.

Timed per call by HIP events on the launch stream after a warm-up (median of
--steps, with the minimum and maximum).  Beside it, in the same run, wall
clock, best of 3: the edits, the three row tables, their bounds and the key
bytes copied to page-locked host memory, lv_version_apply_host on one core,
the rows copied back.  Before anything is reported the device's rows,
directory indices and totals are compared whole with the host twin's.
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


def keys_of(np, ordinals, seq):
    """24-byte internal keys: the ordinal as 16 decimal digits, then (seq << 8 | 1)."""
    n = len(ordinals)
    out = np.zeros((n, 24), dtype=np.uint8)
    out[:, :16] = (ordinals[:, None] // (10 ** np.arange(15, -1, -1, dtype=np.uint64))[None, :]) % 10 + 48
    out[:, 16:] = ((seq.astype(np.uint64) << np.uint64(8)) | np.uint64(1)).astype("<u8").view(np.uint8).reshape(n, 8)
    return out


def make(np, VE, VS, shape, log2_edits, log2_files):
    """(src, E, F, bf, D, bd, P, bp, directory) as arrays."""
    if shape == "manifest":
        n, per = 1 << log2_edits, 30
        rec = np.repeat(np.arange(n, dtype=np.uint64), per)
        number = np.arange(n * per, dtype=np.uint64) + 2
        level = (rec % 6 + 1).astype(np.uint32)
        bf = np.arange(n + 1, dtype=np.uint64) * per
        keep = np.arange(n) % 64 == 0                                   # edits whose files nobody deletes
        dmask = np.repeat(~keep[:-1], per)                              # edit r + 1 deletes edit r's files
        D = np.zeros(int(dmask.sum()), dtype=VE.DELETED_DTYPE)
        D["number"], D["level"] = number[: (n - 1) * per][dmask], level[: (n - 1) * per][dmask]
        bd = np.concatenate([[0, 0], np.cumsum(np.where(keep[:-1], 0, per))]).astype(np.uint64)
        live = np.concatenate([np.repeat(keep[:-1], per), np.ones(per, dtype=bool)])
    else:
        n, files = 1, 1 << log2_files
        number = np.arange(files, dtype=np.uint64) + 2
        level = (np.arange(files, dtype=np.uint64) * 6 // files + 1).astype(np.uint32)   # WriteSnapshot: level by level
        bf = np.array([0, files], dtype=np.uint64)
        D, bd = np.zeros(0, dtype=VE.DELETED_DTYPE), np.zeros(2, dtype=np.uint64)
        live = np.ones(files, dtype=bool)
    nf = len(number)
    src = np.zeros((nf, 2, 24), dtype=np.uint8)
    src[:, 0] = keys_of(np, number * 2, number)
    src[:, 1] = keys_of(np, number * 2 + 1, number)
    F = np.zeros(nf, dtype=VE.FILE_DTYPE)
    F["number"], F["level"] = number, level
    F["file_size"] = (2 << 20) + (number % 4096)
    F["smallest_off"], F["largest_off"] = np.arange(nf, dtype=np.uint64) * 48, np.arange(nf, dtype=np.uint64) * 48 + 24
    F["smallest_len"] = F["largest_len"] = 24
    E = np.zeros(n, dtype=VE.EDIT_DTYPE)
    E["log_number"], E["next_file_number"], E["last_sequence"] = 1, bf[1:] + 2, bf[1:] + 2
    E["has"] = VE.HAS_LOG_NUMBER | VE.HAS_NEXT_FILE | VE.HAS_LAST_SEQUENCE
    P, bp = np.zeros(0, dtype=VE.POINTER_DTYPE), np.zeros(n + 1, dtype=np.uint64)
    dr = np.zeros(int(live.sum()), dtype=VS.PLACEMENT_DTYPE)
    dr["number"] = number[live]
    dr["file_cap"] = F["file_size"][live]
    dr["file_off"] = np.concatenate([[0], np.cumsum(dr["file_cap"][:-1] + 15 & ~np.uint64(15))])
    return src.reshape(-1), E, F, bf, D, bd, P, bp, dr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="manifest,snapshot")
    ap.add_argument("--log2-edits", type=int, default=16)
    ap.add_argument("--log2-files", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.version_edit as VE
    import lvgpu.version_set as VS
    lvgpu.device_init()
    dev = torch.device("cuda:0")
    L = VS._bind()
    for shape in a.shapes.split(","):
        src, E, F, bf, D, bd, P, bp, dr = make(np, VE, VS, shape, a.log2_edits, a.log2_files)
        host_arrays = (src, E.view(np.uint8), F.view(np.uint8), bf.view(np.int64), D.view(np.uint8), bd.view(np.int64),
                       P.view(np.uint8), bp.view(np.int64), dr.view(np.uint8))
        d = [torch.from_numpy(np.ascontiguousarray(x) if x.size else np.zeros(16, dtype=x.dtype)).to(dev) for x in host_arrays]
        d_n = torch.tensor([len(E)], dtype=torch.int64, device=dev)
        caps = (len(F), len(D), len(P))
        files_cap = 1 << 16 if shape == "manifest" else 1 << a.log2_files
        ws = torch.empty(VS.workspace_bytes(caps[0], caps[1], files_cap), dtype=torch.uint8, device=dev)

        def run():
            return VS.apply_device(d[0][: src.size], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d_n, directory=d[8],
                                   dir_n=len(dr), rec_cap=len(E), caps=caps, files_cap=files_cap, workspace=ws)

        # the route without the entry point: tables to pinned host memory, the twin, the rows back
        pinned = [torch.empty(x.shape, dtype=x.dtype).pin_memory() for x in d]
        rows_h = torch.empty(files_cap * 64, dtype=torch.uint8).pin_memory()
        index_h = torch.empty(files_cap, dtype=torch.int32).pin_memory()
        tot_h = np.zeros(VS.TOTALS_WORDS, dtype=np.uint64)
        rows_d = torch.empty(files_cap * 64, dtype=torch.uint8, device=dev)
        index_d = torch.empty(files_cap, dtype=torch.int32, device=dev)

        def host_route():
            for h, t in zip(pinned, d):
                h.copy_(t, non_blocking=True)
            torch.cuda.synchronize()
            i = VE.EncodeIn()
            i.d_edits = pinned[1].data_ptr()
            i.d_files, i.file_cap, i.d_rec_file = pinned[2].data_ptr(), caps[0], pinned[3].data_ptr()
            i.d_deleted, i.deleted_cap, i.d_rec_deleted = (pinned[4].data_ptr() if caps[1] else None), caps[1], pinned[5].data_ptr()
            i.d_pointers, i.pointer_cap, i.d_rec_pointer = (pinned[6].data_ptr() if caps[2] else None), caps[2], pinned[7].data_ptr()
            o = VS.ApplyOut()
            o.d_files_out, o.files_cap, o.d_dir_index, o.d_totals = rows_h.data_ptr(), files_cap, index_h.data_ptr(), tot_h.ctypes.data
            rc = L.lv_version_apply_host(pinned[0].data_ptr(), src.size, ctypes.byref(i), len(E), pinned[8].data_ptr(), len(dr),
                                         ctypes.byref(o))
            assert rc == 0, rc
            live = int(tot_h[4])
            rows_d[: live * 64].copy_(rows_h[: live * 64], non_blocking=True)
            index_d[:live].copy_(index_h[:live], non_blocking=True)
            torch.cuda.synchronize()
            return live

        got = run()
        t = got.sync_totals()
        live = host_route()
        want = VS.totals_dict(tot_h)
        assert t == want and t["live"] == live and t["unplaced"] == 0, (t, want)
        assert torch.equal(got.files_t[: live * 64].cpu(), rows_h[: live * 64]), "rows differ from the host twin's"
        assert torch.equal(got.dir_index_t[:live].cpu(), index_h[:live]), "dir_index differs from the host twin's"
        med, lo, hi = event_ms(torch, run, a.steps, a.warmup)
        host = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_route()
            host.append((time.perf_counter() - t0) * 1e3)
        line = dict(bench="version_apply", shape=shape, records=len(E), new_files=len(F), deleted=len(D), live=live,
                    files_cap=files_cap, workspace_bytes=int(ws.numel()), device_ms=round(med, 4), device_ms_min=round(lo, 4),
                    device_ms_max=round(hi, 4), host_route_ms=round(min(host), 3), ratio=round(min(host) / med, 2),
                    steps=a.steps, warmup=a.warmup, kernel=lvgpu.last_kernel(), device=torch.cuda.get_device_name(0))
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(s + "\n")
        del d, pinned, ws, rows_d, rows_h
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
