"""Python mirror of include/lvgpu/write_batch.h: WriteBatch::iterate
(write_batch.rs:92-122) on the host and over records in HBM.

    iterate(rep)                      lv_write_batch_iterate: (status, ops, sequence, count),
                                      ops = [(tag, key_off, key_len, val_off, val_len)]
    decode_workspace_bytes(rec_cap)   device workspace of decode_device
    decode_device(payload, rec_off, rec_len, records, upstream_status)
                                      lv_write_batch_decode_device over what
                                      lvgpu.wal.decode_device wrote: the log-ordered op
                                      table, per-record bounds and statuses, totals; no
                                      host sync until .sync_totals() / .ops() / ...
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import LvError, lib

HEADER_SIZE = 12                      # LV_WB_HEADER_SIZE
TYPE_DELETION, TYPE_VALUE = 0, 1      # LV_WB_TYPE_*
OK, TOO_SMALL, BAD_VARINT, BAD_LENGTH, WRONG_COUNT, BAD_TAG, OUT_OF_RANGE = range(7)  # LV_WB_*
# what WriteBatch::iterate says for each status (the header's comments)
STATUS_TEXT = {
    1: "malformed WriteBatch (too small)",
    2: "Error when decoding varint-32",
    3: "Input slice doesn't contain a length-prefixed encoded value.",
    4: "WriteBatch has wrong count",
}
DECODE_STATUS = {1: "UPSTREAM", 2: "REC_OVER", 4: "OP_OVER"}  # LV_WB_DECODE_*
TOTALS = ("records", "ops", "key_bytes", "value_bytes", "bad_records", "last_sequence", "status")
# csrc/write_batch.hip: kWbSmall (records up to this many bytes take one lane),
# kWbWindow / kWbRound (the wave class's LDS window and its first load), kWbTile
# (records per scan tile).  The GPU tests sweep around them.
WB_SMALL = 16384
WB_WINDOW = 4096
WB_ROUND = 1024
WB_TILE = 256

OP_DTYPE = np.dtype([("tag", "<u8"), ("key_off", "<u8"), ("val_off", "<u8"), ("key_len", "<u4"), ("val_len", "<u4")])
assert OP_DTYPE.itemsize == 32


class DecodeOut(ctypes.Structure):
    """lv_wb_decode_out (include/lvgpu/write_batch.h)."""
    _fields_ = [("d_ops", ctypes.c_void_p), ("op_cap", ctypes.c_size_t), ("d_rec_op", ctypes.c_void_p),
                ("d_rec_status", ctypes.c_void_p), ("d_totals", ctypes.c_void_p)]


_bound = False


def _bind():
    global _bound
    L = lib()
    if _bound:
        return L
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.lv_write_batch_iterate.restype = ctypes.c_uint32
    L.lv_write_batch_iterate.argtypes = [vp, sz, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64),
                                         ctypes.POINTER(ctypes.c_uint32)]
    L.lv_write_batch_decode_workspace_bytes.restype = sz
    L.lv_write_batch_decode_workspace_bytes.argtypes = [sz]
    L.lv_write_batch_decode_device.restype = ctypes.c_int
    L.lv_write_batch_decode_device.argtypes = [vp, sz, vp, vp, vp, vp, sz, ctypes.POINTER(DecodeOut), ctypes.c_uint32,
                                               vp, sz, vp]
    _bound = True
    return L


def iterate(rep, op_cap=None):
    """lv_write_batch_iterate over `rep`: (status, ops, sequence, count).  ops
    is a list of (tag, key_off, key_len, val_off, val_len) with offsets into
    rep -- min(found, op_cap) of them (op_cap None: all of them)."""
    st, ops, seq, cnt, _ = _iterate(rep, op_cap)
    return st, ops, seq, cnt


def iterate_found(rep, op_cap=None):
    """iterate plus the number of ops found: (status, ops, sequence, count, found)."""
    return _iterate(rep, op_cap)


def _iterate(rep, op_cap):
    L = _bind()
    rep = bytes(rep)
    buf = ctypes.create_string_buffer(rep, max(len(rep), 1))
    found, seq, cnt = ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_uint32()
    if op_cap is None:  # count, then fetch all
        L.lv_write_batch_iterate(buf, len(rep), None, 0, ctypes.byref(found), None, None)
        op_cap = found.value
    arr = np.zeros(max(op_cap, 1), dtype=OP_DTYPE)
    st = L.lv_write_batch_iterate(buf, len(rep), arr.ctypes.data if op_cap else None, op_cap, ctypes.byref(found),
                                  ctypes.byref(seq), ctypes.byref(cnt))
    k = min(found.value, op_cap)
    ops = [(int(o["tag"]), int(o["key_off"]), int(o["key_len"]), int(o["val_off"]), int(o["val_len"]))
           for o in arr[:k]]
    return int(st), ops, int(seq.value), int(cnt.value), int(found.value)


def decode_workspace_bytes(rec_cap: int) -> int:
    return int(_bind().lv_write_batch_decode_workspace_bytes(rec_cap))


class Ops:
    """Outputs of decode_device, CUDA tensors written asynchronously: ops_t
    (uint8, 32 bytes per lv_wb_op), rec_op (int64, rec_cap + 1), rec_status
    (int32) and totals (int64[7], TOTALS)."""

    def __init__(self, ops_t, op_cap, rec_op, rec_status, totals, keep):
        self.ops_t, self.op_cap, self.rec_op, self.rec_status, self.totals = ops_t, op_cap, rec_op, rec_status, totals
        self._keep = keep  # the inputs and the workspace, until the work has run
        self._tot = None

    def sync_totals(self, check: bool = True) -> dict:
        """Waits for the call; the totals as a dict.  Raises LvError naming the
        status bits if one is set (nothing else was written) unless check is
        False."""
        if self._tot is None:
            import torch
            torch.cuda.synchronize(self.totals.device)
            t = [int(v) for v in self.totals.cpu().numpy().view(np.uint64)]
            self._tot = dict(zip(TOTALS, t))
            self._keep = None
        st = self._tot["status"]
        if st and check:
            names = "|".join(n for b, n in DECODE_STATUS.items() if st & b)
            raise LvError(f"lv_write_batch_decode_device: status {names} (totals {self._tot})")
        return self._tot

    def ops(self):
        """The op table as a numpy structured array (OP_DTYPE; synchronises)."""
        n = self.sync_totals()["ops"]
        return self.ops_t[: n * 32].cpu().numpy().view(OP_DTYPE).copy()

    def record_bounds(self):
        """d_rec_op: records + 1 bounds into the op table (synchronises)."""
        n = self.sync_totals()["records"]
        return self.rec_op[: n + 1].cpu().numpy().view(np.uint64).copy()

    def statuses(self):
        """LV_WB_* of each record (synchronises)."""
        n = self.sync_totals()["records"]
        return self.rec_status[:n].cpu().numpy().view(np.uint32).copy()


def decode_device(payload, rec_off, rec_len, records, upstream_status=None, *, rec_cap=None, op_cap=None,
                  workspace=None, stream=None, fill=None, guard: int = 0, flags: int = 0):
    """lv_write_batch_decode_device.  `payload` is a uint8 CUDA tensor;
    rec_off / rec_len int64 CUDA tensors; `records` and `upstream_status`
    int64 CUDA tensors whose first element is read on the device (e.g.
    Decoded.totals[0:1] and Decoded.totals[4:5] of lvgpu.wal.decode_device).
    rec_cap defaults to rec_off.numel(), op_cap to payload.numel() // 2, which
    always suffices.  fill, a byte value, initialises the output arrays with it
    first and guard allocates that many more bytes behind each (canaries).
    Returns an Ops; asynchronous on `stream`."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind()
    if payload.dtype != torch.uint8:
        raise LvError(f"payload must be a uint8 tensor (got {payload.dtype}: numel() would not count bytes)")
    dev = payload.device
    for name, t in (("rec_off", rec_off), ("rec_len", rec_len), ("records", records),
                    ("upstream_status", upstream_status)):
        if t is None and name == "upstream_status":
            continue
        if t is None or t.dtype != torch.int64 or t.device != dev:
            raise LvError(f"{name} must be an int64 tensor on the payload's device")
    if workspace is not None and (workspace.dtype != torch.uint8 or workspace.device != dev):
        raise LvError("workspace must be a uint8 tensor on the payload's device")
    rec_cap = int(min(rec_off.numel(), rec_len.numel())) if rec_cap is None else int(rec_cap)
    if rec_off.numel() < rec_cap or rec_len.numel() < rec_cap or records.numel() < 1:
        raise LvError("rec_off / rec_len must hold rec_cap entries and records one")
    op_cap = payload.numel() // 2 if op_cap is None else int(op_cap)
    if workspace is None:
        workspace = torch.empty(L.lv_write_batch_decode_workspace_bytes(rec_cap), dtype=torch.uint8, device=dev)

    def alloc(nbytes):
        nbytes = (max(nbytes, 16) + guard + 7) & ~7
        if fill is None:
            return torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
    ops_t = alloc(op_cap * 32)
    rec_op = alloc((rec_cap + 1) * 8).view(torch.int64)
    rec_status = alloc(rec_cap * 4).view(torch.int32)
    totals = torch.empty(len(TOTALS), dtype=torch.int64, device=dev)
    o = DecodeOut()
    o.d_ops, o.op_cap = _dev_ptr(ops_t, "ops"), op_cap
    o.d_rec_op, o.d_rec_status = _dev_ptr(rec_op, "rec_op"), _dev_ptr(rec_status, "rec_status")
    o.d_totals = _dev_ptr(totals, "totals")
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_write_batch_decode_device(_dev_ptr(payload, "payload"), payload.numel(),
                                            _dev_ptr(rec_off, "rec_off"), _dev_ptr(rec_len, "rec_len"),
                                            _dev_ptr(records, "records"), _dev_ptr(upstream_status, "upstream_status"),
                                            rec_cap, ctypes.byref(o), flags, _dev_ptr(workspace, "workspace"),
                                            workspace.numel(), _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_write_batch_decode_device: {lib().lv_last_error().decode()}")
    return Ops(ops_t, op_cap, rec_op, rec_status, totals, (payload, rec_off, rec_len, records, upstream_status, workspace))
