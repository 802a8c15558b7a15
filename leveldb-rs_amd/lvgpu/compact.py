"""Python mirror of include/lvgpu/compact.h: the entries of a sorted memtable
quadruple that a compaction keeps (upstream's DoCompactionWork loop), on the
host and in HBM.

    pack_ranges(ranges)               [(lo, hi)] -> (RANGE_DTYPE array, key bytes)
    filter_host(payload, ops, order, mt_totals, snapshot, ranges, flags)
                                      lv_compact_filter_host: a HostFiltered
    filter_workspace_bytes(op_cap)    device workspace of filter_device
    filter_device(table, snapshot, ranges, flags)
                                      lv_compact_filter_device over a
                                      lvgpu.memtable.Table: a Filtered, which
                                      lvgpu.table.build_device and
                                      lvgpu.memtable.get_device take as a table;
                                      no host sync until .sync() / .order()
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import LvError, lib
from .memtable import Table
from .memtable import Totals as MtTotals  # lv_mt_totals
from .write_batch import OP_DTYPE

BASE_LEVEL = 1                                                 # LV_COMPACT_BASE_LEVEL
MAX_RANGES = 4096                                              # LV_COMPACT_MAX_RANGES
STATUS = {1: "UPSTREAM", 2: "BAD_INPUT", 4: "BAD_RANGE"}       # LV_COMPACT_*
UPSTREAM, BAD_INPUT, BAD_RANGE = STATUS
TOTALS = ("entries_in", "kept", "dropped_hidden", "dropped_deletions", "unparsed", "user_keys", "reserved", "status")
MT_TOTALS = ("entries", "user_keys", "status")
# csrc/lvk/knobs.h: LVK_CF_TILE (entries per scan tile of the flag kernel).
# The GPU tests stand on its boundaries.
CF_TILE = 1024

RANGE_DTYPE = np.dtype([("lo_off", "<u8"), ("hi_off", "<u8"), ("lo_len", "<u4"), ("hi_len", "<u4")])
assert RANGE_DTYPE.itemsize == 24


class CompactTotals(ctypes.Structure):
    """lv_compact_totals."""
    _fields_ = [(n, ctypes.c_uint64) for n in TOTALS]


_bound = False


def _bind():
    global _bound
    L = lib()
    if not _bound:
        vp, sz, u64, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32
        L.lv_compact_filter_workspace_bytes.restype = sz
        L.lv_compact_filter_workspace_bytes.argtypes = [sz]
        L.lv_compact_filter_host.restype = ctypes.c_int
        L.lv_compact_filter_host.argtypes = [vp, sz, vp, vp, vp, sz, u64, vp, sz, vp, sz, vp, vp, vp, u32]
        L.lv_compact_filter_device.restype = ctypes.c_int
        L.lv_compact_filter_device.argtypes = [vp, sz, vp, vp, vp, sz, u64, vp, sz, vp, sz, vp, vp, vp, u32, vp, sz, vp]
        _bound = True
    return L


def pack_ranges(ranges):
    """[(lo, hi)] as (a RANGE_DTYPE array, the key bytes it points into)."""
    keys, rows = bytearray(), []
    for lo, hi in ranges:
        lo_off = len(keys)
        keys += lo
        hi_off = len(keys)
        keys += hi
        rows.append((lo_off, hi_off, len(lo), len(hi)))
    return np.array(rows, dtype=RANGE_DTYPE) if rows else np.zeros(0, dtype=RANGE_DTYPE), bytes(keys)


def _ranges(ranges):
    """ranges as (RANGE_DTYPE array, key bytes): a list of (lo, hi), or such a
    pair already (raw rows: a test's out-of-range extents)."""
    if ranges is None:
        return np.zeros(0, dtype=RANGE_DTYPE), b""
    if isinstance(ranges, tuple) and len(ranges) == 2 and isinstance(ranges[0], np.ndarray):
        return np.ascontiguousarray(ranges[0], dtype=RANGE_DTYPE), bytes(ranges[1])
    return pack_ranges(ranges)


class HostFiltered:
    """Outputs of filter_host: totals and mt_totals (dicts) and order_out, the
    whole op_cap-element array the call was given, filled with `fill` first
    (order_out[:kept] are the kept op indices)."""

    def __init__(self, totals, mt_totals, order_out):
        self.totals, self.mt_totals, self.order_out = totals, mt_totals, order_out

    def order(self):
        return self.order_out[: self.totals["kept"]]


def filter_host(payload, ops, order, mt_totals, snapshot, ranges=None, flags=0, *, op_cap=None, payload_bytes=None,
                fill=0xA5A5A5A5):
    """lv_compact_filter_host.  mt_totals is the dict of the build (entries,
    user_keys, status); op_cap defaults to len(ops); payload_bytes overrides
    len(payload).  Raises LvError on LV_ERR_INVALID."""
    L = _bind()
    pb = bytes(payload)
    pbuf = ctypes.create_string_buffer(pb, max(len(pb), 1))
    pn = len(pb) if payload_bytes is None else payload_bytes
    arr = np.ascontiguousarray(ops, dtype=OP_DTYPE)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    op_cap = arr.size if op_cap is None else int(op_cap)
    if order.size < op_cap:  # (the entries decide how much of it is read)
        order = np.concatenate([order, np.zeros(op_cap - order.size, dtype=np.uint32)])
    rr, rk = _ranges(ranges)
    rkbuf = ctypes.create_string_buffer(rk, max(len(rk), 1))
    out = np.full(max(op_cap, 1), fill, dtype=np.uint32)
    mt = MtTotals(mt_totals["entries"], mt_totals["user_keys"], mt_totals["status"])
    mto, tot = MtTotals(), CompactTotals()
    rc = L.lv_compact_filter_host(pbuf if pn or pb else None, pn, arr.ctypes.data if arr.size else None,
                                  order.ctypes.data if order.size else None, ctypes.byref(mt), op_cap, snapshot,
                                  rr.ctypes.data if rr.size else None, rr.size, rkbuf if rk else None, len(rk),
                                  out.ctypes.data if op_cap else None, ctypes.byref(mto), ctypes.byref(tot), flags)
    if rc != 0:
        raise LvError(f"lv_compact_filter_host: {rc}")
    return HostFiltered({n: int(getattr(tot, n)) for n in TOTALS}, {n: int(getattr(mto, n)) for n in MT_TOTALS},
                        out[:op_cap])


def filter_workspace_bytes(op_cap: int) -> int:
    return int(_bind().lv_compact_filter_workspace_bytes(op_cap))


class Filtered(Table):
    """Outputs of filter_device, CUDA tensors written asynchronously: order_t
    (int32, the kept op indices; op_cap entries and the guard), totals (int64[3],
    the kept entries' lv_mt_totals) and compact_totals (int64[8], TOTALS).  With
    the source's payload and ops it is a lvgpu.memtable.Table."""

    def __init__(self, source, order_t, mt_totals, compact_totals, keep):
        super().__init__(source.payload, source.ops_t, source.op_cap, order_t, mt_totals, keep)
        self.source, self.compact_totals = source, compact_totals
        self._ctot = None

    def sync(self, check: bool = True) -> dict:
        """Waits for the call; the lv_compact_totals as a dict.  Raises LvError
        naming the status bits if one is set (d_order_out was not written)
        unless check is False."""
        if self._ctot is None:
            import torch
            torch.cuda.synchronize(self.compact_totals.device)
            self._ctot = dict(zip(TOTALS, (int(v) for v in self.compact_totals.cpu().numpy().view(np.uint64))))
        st = self._ctot["status"]
        if st and check:
            names = "|".join(n for b, n in STATUS.items() if st & b)
            raise LvError(f"lv_compact_filter_device: status {names} (totals {self._ctot})")
        return self._ctot


def filter_device(table, snapshot, ranges=None, flags=0, *, op_cap=None, order_t=None, mt_totals=None, totals=None,
                  workspace=None, stream=None, fill=None, guard: int = 0):
    """lv_compact_filter_device over a lvgpu.memtable.Table (a memtable build's,
    Scanned.memtable() or an earlier Filtered): its payload, ops, order and
    totals, read on the device.  ranges is a list of (lo, hi) byte strings (or
    pack_ranges' pair), copied to the device here.  order_t / mt_totals / totals
    reuse the outputs of an earlier call (graph replays).  ranges may also be
    (RANGE_DTYPE array, uint8 CUDA tensor): range keys that already lie in HBM,
    the rows' offsets pointing into that tensor, which is passed as it is
    (range_key_bytes = its numel(): offsets beyond 4 GiB).  fill, a byte value,
    initialises d_order_out with it first and guard allocates that many more
    bytes behind it (canaries).  Returns a Filtered; asynchronous on `stream`."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind()
    dev = table.payload.device
    op_cap = int(table.op_cap) if op_cap is None else int(op_cap)
    d_rr = d_rk = None
    if isinstance(ranges, tuple) and len(ranges) == 2 and torch.is_tensor(ranges[1]):
        rr, d_rk = np.ascontiguousarray(ranges[0], dtype=RANGE_DTYPE), ranges[1]
        if d_rk.dtype != torch.uint8 or d_rk.device != dev:
            raise LvError("range keys must be a uint8 tensor on the payload's device")
        rk_bytes = d_rk.numel()
    else:
        rr, rk = _ranges(ranges)
        rk_bytes = len(rk)
        if rk:
            d_rk = torch.frombuffer(bytearray(rk), dtype=torch.uint8).to(dev)
    if rr.size:
        d_rr = torch.from_numpy(np.frombuffer(rr.tobytes(), dtype=np.int64).copy()).to(dev)
    if workspace is None:
        workspace = torch.empty(max(L.lv_compact_filter_workspace_bytes(op_cap), 16), dtype=torch.uint8, device=dev)
    if order_t is None:
        nbytes = (max(op_cap * 4, 16) + guard + 7) & ~7
        if fill is None:
            order_t = torch.empty(nbytes, dtype=torch.uint8, device=dev).view(torch.int32)
        else:
            order_t = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev).view(torch.int32)
    if mt_totals is None:
        mt_totals = torch.empty(len(MT_TOTALS), dtype=torch.int64, device=dev)
    if totals is None:
        totals = torch.empty(len(TOTALS), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_compact_filter_device(_dev_ptr(table.payload, "payload") if table.payload.numel() else None,
                                        table.payload.numel(), _dev_ptr(table.ops_t, "ops") if op_cap else None,
                                        _dev_ptr(table.order_t, "order") if op_cap else None,
                                        _dev_ptr(table.totals, "mt_totals"), op_cap, snapshot,
                                        _dev_ptr(d_rr, "ranges"), rr.size, _dev_ptr(d_rk, "range_keys"), rk_bytes,
                                        _dev_ptr(order_t, "order_out") if op_cap else None,
                                        _dev_ptr(mt_totals, "mt_totals_out"), _dev_ptr(totals, "totals"), flags,
                                        _dev_ptr(workspace, "workspace"), workspace.numel(), _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_compact_filter_device: {lib().lv_last_error().decode()}")
    return Filtered(table, order_t, mt_totals, totals, (table, d_rr, d_rk, workspace))
