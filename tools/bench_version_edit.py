#!/usr/bin/env python3
"""lv_version_edit_decode_device and lv_version_edit_encode_device against the
copy-back-and-host-twin routes they replace.  One JSON line per shape and
direction.

    python tools/bench_version_edit.py                       # both shapes, both directions
    python tools/bench_version_edit.py --shapes manifest --log2-edits 12   # a small rehearsal

Shapes: "manifest", 2^16 edits of 30 new files and 30 deleted files each (what
a long-lived MANIFEST holds); "snapshot", one edit of 2^20 new files
(upstream's WriteSnapshot: the stage's serial worst case, one wave walks it).
Keys are 24-byte internal keys (16-byte user keys), numbers six-digit file
numbers, sizes around 2 MiB.

Timed per call by HIP events on the launch stream after a warm-up (median of
--steps, with the minimum and maximum).  Beside it, in the same run, the only
route without these entry points (wall clock, best of 3 each step):
  decode: the payload and the record arrays copied to page-locked host memory,
          lv_version_edit_decode_host over every record on one core in a native
          loop (tools/host_replay.c), the edits and the three row tables copied
          back;
  encode: the tables, the bounds and the key arena copied to page-locked host
          memory, lv_version_edit_encode_host on one core, the records copied
          back.
Before anything is reported the device's outputs are compared whole with the
host twin's.
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


def best_ms(torch, fn, reps=3):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out)


def build(np, VE, shape, log2_edits, log2_files):
    """The encode's inputs of a shape: (src, edits, files, rec_file, deleted,
    rec_deleted, pointers, rec_pointer), numpy arrays."""
    rng = np.random.default_rng(19)
    if shape == "manifest":
        n, per_f, per_d = 1 << log2_edits, 30, 30
    else:
        n, per_f, per_d = 1, 1 << log2_files, 0
    nf, nd = n * per_f, n * per_d
    src = rng.integers(0, 256, size=nf * 48 + 32, dtype=np.uint8)
    E = np.zeros(n, dtype=VE.EDIT_DTYPE)
    E["log_number"] = np.arange(n, dtype=np.uint64) + np.uint64(100000)
    E["next_file_number"] = np.arange(n, dtype=np.uint64) * np.uint64(per_f) + np.uint64(200000)
    E["last_sequence"] = np.arange(n, dtype=np.uint64) * np.uint64(4096) + np.uint64(1 << 32)
    E["has"] = VE.HAS_LOG_NUMBER | VE.HAS_NEXT_FILE | VE.HAS_LAST_SEQUENCE
    if shape == "snapshot":
        E["has"] |= VE.HAS_COMPARATOR
        E["comparator_off"], E["comparator_len"] = 0, 27  # about the length of "leveldb.BytewiseComparator"
    F = np.zeros(nf, dtype=VE.FILE_DTYPE)
    i = np.arange(nf, dtype=np.uint64)
    F["number"] = i + np.uint64(200000)
    F["file_size"] = np.uint64(2 << 20) + (i * np.uint64(7919)) % np.uint64(1 << 18)
    F["smallest_off"], F["largest_off"] = i * np.uint64(48) + np.uint64(32), i * np.uint64(48) + np.uint64(56)
    F["smallest_len"] = F["largest_len"] = 24
    F["level"] = (i % np.uint64(6) + np.uint64(1)).astype(np.uint32)
    D = np.zeros(nd, dtype=VE.DELETED_DTYPE)
    if nd:
        j = np.arange(nd, dtype=np.uint64)
        D["level"] = ((j % np.uint64(per_d)) // np.uint64(5)).astype(np.uint32)  # ascending inside an edit
        D["number"] = j + np.uint64(100000)
    P = np.zeros(0, dtype=VE.POINTER_DTYPE)
    u = lambda per: np.arange(n + 1, dtype=np.uint64) * np.uint64(per)
    return src, E, F, u(per_f), D, u(per_d), P, u(0)


def run(args, shape):
    import numpy as np
    import torch

    import lvgpu
    import lvgpu.version_edit as VE

    dev = torch.device("cuda:0")
    lvgpu.device_init()
    L = VE._bind()
    R = ctypes.CDLL(os.path.join(ROOT, "leveldb-rs_amd", "lib", "libhostreplay.so"))
    R.lv_replay_version_edit.restype = ctypes.c_double
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    R.lv_replay_version_edit.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp, sz, vp, sz, ctypes.c_int, vp, vp]

    src, E, F, bf, D, bd, P, bp = build(np, VE, shape, args.log2_edits, args.log2_files)
    n, nf, nd = E.size, F.size, D.size
    caps = (nf, nd, 0)

    def pinned(a):
        h = lvgpu.host_alloc(max(a.nbytes, 16))
        h[: a.nbytes] = np.frombuffer(a.tobytes(), dtype=np.uint8) if a.nbytes else 0
        return h

    def h_in(h_src, hE, hF, hD, hbf, hbd, hbp):
        i = VE.EncodeIn()
        i.d_edits = hE.ctypes.data
        i.d_files, i.file_cap, i.d_rec_file = hF.ctypes.data, nf, hbf.ctypes.data
        i.d_deleted, i.deleted_cap, i.d_rec_deleted = (hD.ctypes.data if nd else None), nd, hbd.ctypes.data
        i.d_pointers, i.pointer_cap, i.d_rec_pointer = None, 0, hbp.ctypes.data
        return i

    # ---- the host twin's encode: the reference for the bytes, and the decode's input ----
    h_src, hE, hF, hD = pinned(src), pinned(E), pinned(F), pinned(D)
    hbf, hbd, hbp = pinned(bf), pinned(bd), pinned(bp)
    h_off, h_len = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    tot = VE.EncodeTotals()
    i = h_in(h_src, hE, hF, hD, hbf, hbd, hbp)
    o = VE.EncodeOut()
    o.d_rec_off, o.d_rec_len, o.d_totals = h_off.ctypes.data, h_len.ctypes.data, ctypes.addressof(tot)
    if L.lv_version_edit_encode_host(None, src.size, ctypes.byref(i), n, ctypes.byref(o)) or tot.status:
        raise SystemExit(f"{shape}: host sizing failed, status {tot.status}")
    out_bytes = int(tot.out_bytes)
    h_out = lvgpu.host_alloc(out_bytes)
    o.d_out, o.out_cap = h_out.ctypes.data, out_bytes
    enc_host = []
    for _ in range(3):
        t0 = time.perf_counter()
        rc = L.lv_version_edit_encode_host(h_src.ctypes.data, src.size, ctypes.byref(i), n, ctypes.byref(o))
        enc_host.append((time.perf_counter() - t0) * 1e3)
        if rc or tot.status or tot.out_bytes != out_bytes:
            raise SystemExit(f"{shape}: host encode failed")

    up = lambda a: torch.from_numpy(np.frombuffer(a.tobytes() + bytes(16), dtype=np.uint8).copy()).to(dev)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to(dev)
    d_src, dE, dF, dD, dP = torch.from_numpy(src).to(dev), up(E), up(F), up(D), up(P)
    dbf, dbd, dbp, d_n = i64(bf), i64(bd), i64(bp), torch.tensor([n], dtype=torch.int64, device=dev)
    base = {"tool": "bench_version_edit", "shape": shape, "records": int(n), "files": int(nf), "deleted": int(nd),
            "record_bytes": out_bytes, "steps": args.steps, "warmup": args.warmup}

    # ---- encode ----
    if "encode" in args.directions:
        ews = torch.empty(max(VE.encode_workspace_bytes(n, *caps), 16), dtype=torch.uint8, device=dev)
        d_out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
        st = {}

        def enc():
            st["r"] = VE.encode_device(d_src, dE, dF, dbf, dD, dbd, dP, dbp, d_n, rec_cap=n, caps=caps, out=d_out,
                                       workspace=ews)
        enc()
        t = st["r"].sync_totals()
        if t["out_bytes"] != out_bytes or not torch.equal(d_out.cpu(), torch.from_numpy(h_out[:out_bytes])):
            raise SystemExit(f"{shape}: the device's bytes differ from the host twin's")
        if not (np.array_equal(st["r"].rec_off(), h_off) and np.array_equal(st["r"].rec_len(), h_len)):
            raise SystemExit(f"{shape}: the device's record arrays differ from the host twin's")
        ms, lo, hi = event_ms(torch, enc, args.steps, args.warmup)
        tens = [(torch.from_numpy(h), d) for h, d in ((h_src, d_src), (hE, dE), (hF, dF), (hD, dD))]
        d2h = best_ms(torch, lambda: [h[: d.numel()].copy_(d[: h.numel()]) for h, d in tens])
        t_out = torch.from_numpy(h_out)
        h2d = best_ms(torch, lambda: d_out.copy_(t_out[:out_bytes]))
        host = {"d2h_ms": round(d2h, 3), "encode_ms": round(min(enc_host), 3), "h2d_ms": round(h2d, 3),
                "ms": round(d2h + min(enc_host) + h2d, 3),
                "note": "D2H of the tables and the key arena into page-locked memory + lv_version_edit_encode_host on one "
                        "core + H2D of the records"}
        print(json.dumps(dict(base, api="lv_version_edit_encode_device", ms=round(ms, 4), ms_min=round(lo, 4),
                              ms_max=round(hi, 4), out_gib_s=round(out_bytes / 2**30 / (ms / 1e3), 2), host_route=host,
                              speedup_vs_host_route=round(host["ms"] / ms, 2),
                              checked="d_out, rec_off and rec_len whole == lv_version_edit_encode_host")), flush=True)

    # ---- decode ----
    if "decode" in args.directions:
        d_pay = torch.from_numpy(h_out[:out_bytes].copy()).to(dev)
        d_off, d_len = i64(h_off), i64(h_len)
        dws = torch.empty(max(VE.decode_workspace_bytes(n), 16), dtype=torch.uint8, device=dev)
        st = {}

        def dec():
            st["r"] = VE.decode_device(d_pay, d_off, d_len, d_n, rec_cap=n, caps=caps, workspace=dws)
        dec()
        r = st["r"]
        t = r.sync_totals()
        if (t["files"], t["deleted"], t["bad_records"]) != (nf, nd, 0):
            raise SystemExit(f"{shape}: decode totals differ from the input: {t}")
        # the native loop over the host twin
        gE, gF = np.zeros(n, dtype=VE.EDIT_DTYPE), np.zeros(max(nf, 1), dtype=VE.FILE_DTYPE)
        gD, gP = np.zeros(max(nd, 1), dtype=VE.DELETED_DTYPE), np.zeros(1, dtype=VE.POINTER_DTYPE)
        counts, bad = (ctypes.c_uint64 * 3)(), ctypes.c_uint64()
        sec = R.lv_replay_version_edit(h_out.ctypes.data, h_off.ctypes.data, h_len.ctypes.data, n, gE.ctypes.data,
                                       gF.ctypes.data, nf, gD.ctypes.data, nd, gP.ctypes.data, 0, 3, counts,
                                       ctypes.byref(bad))
        if sec < 0 or tuple(counts) != (nf, nd, 0) or bad.value:
            raise SystemExit(f"{shape}: the host route failed")
        if not (r.edits().tobytes() == gE.tobytes() and r.files().tobytes() == gF[:nf].tobytes()
                and r.deleted().tobytes() == gD[:nd].tobytes()):
            raise SystemExit(f"{shape}: the device's tables differ from the host twin's")
        ms, lo, hi = event_ms(torch, dec, args.steps, args.warmup)
        hp, ho, hl = (torch.from_numpy(lvgpu.host_alloc(max(x.numel() * x.element_size(), 16))) for x in (d_pay, d_off, d_len))
        d2h = best_ms(torch, lambda: (hp[: d_pay.numel()].copy_(d_pay), ho[: n * 8].copy_(d_off.view(torch.uint8)),
                                      hl[: n * 8].copy_(d_len.view(torch.uint8))))
        back = [(torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).pin_memory(), d) for a, d in
                ((gE, r.edits_t), (gF[:nf], r.files_t), (gD[:nd], r.deleted_t)) if a.nbytes]
        h2d = best_ms(torch, lambda: [d[: h.numel()].copy_(h) for h, d in back])
        host = {"d2h_ms": round(d2h, 3), "decode_ms": round(sec * 1e3, 3), "h2d_ms": round(h2d, 3),
                "ms": round(d2h + sec * 1e3 + h2d, 3),
                "note": "D2H of the payload and record arrays into page-locked memory + lv_version_edit_decode_host per "
                        "record on one core in a native loop + H2D of the edits and row tables"}
        print(json.dumps(dict(base, api="lv_version_edit_decode_device", ms=round(ms, 4), ms_min=round(lo, 4),
                              ms_max=round(hi, 4), payload_gib_s=round(out_bytes / 2**30 / (ms / 1e3), 2),
                              rows_per_s=round((nf + nd) / (ms / 1e3)), host_route=host,
                              speedup_vs_host_route=round(host["ms"] / ms, 2), vd_small=VE.VD_SMALL, vd_tile=VE.VD_TILE,
                              checked="d_edits, d_files and d_deleted whole == lv_version_edit_decode_host")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="manifest,snapshot")
    ap.add_argument("--directions", default="encode,decode")
    ap.add_argument("--log2-edits", type=int, default=16, help="manifest: 2^this edits of 30 + 30 rows")
    ap.add_argument("--log2-files", type=int, default=20, help="snapshot: one edit of 2^this files")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    args.directions = args.directions.split(",")
    for shape in args.shapes.split(","):
        run(args, shape.strip())


if __name__ == "__main__":
    main()
