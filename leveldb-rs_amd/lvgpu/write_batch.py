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
    encode_host(src, ops, rec_op, first_sequence)
                                      lv_write_batch_encode_host: the reps of the records
                                      rec_op bounds over an op table into the arena src
    encode_workspace_bytes(rec_cap, op_cap)
    encode_device(src, ops, rec_op, records, upstream_status, first_sequence=...)
                                      lv_write_batch_encode_device: the same in HBM, an
                                      Encoded with lazy .sync_totals() / .out() / ...
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

# the inverse (lv_write_batch_encode_*)
ENCODE_STATUS = {1: "UPSTREAM", 2: "REC_OVER", 4: "BAD_BOUNDS", 8: "BAD_OP", 16: "OUT_OVER"}  # LV_WB_ENCODE_*
ENCODE_TOTALS = ("records", "ops", "key_bytes", "value_bytes", "out_bytes", "last_sequence", "status", "bad_record",
                 "bad_op")
ENCODE_MAX_REC_CAP = (1 << 32) - 2
ENCODE_MAX_OP_CAP = 1 << 30
# csrc/write_batch_encode.hip: kWeTile (ops per scan tile), kWeWaveCopy (a key or
# value of at least this many bytes is copied by a group of kWeCopyLanes lanes
# of its wave).  The GPU tests sweep around them.
WE_TILE = 1024
WE_WAVE_COPY = 64
WE_COPY_LANES = 16

OP_DTYPE = np.dtype([("tag", "<u8"), ("key_off", "<u8"), ("val_off", "<u8"), ("key_len", "<u4"), ("val_len", "<u4")])
assert OP_DTYPE.itemsize == 32


class DecodeOut(ctypes.Structure):
    """lv_wb_decode_out (include/lvgpu/write_batch.h)."""
    _fields_ = [("d_ops", ctypes.c_void_p), ("op_cap", ctypes.c_size_t), ("d_rec_op", ctypes.c_void_p),
                ("d_rec_status", ctypes.c_void_p), ("d_totals", ctypes.c_void_p)]


class EncodeTotals(ctypes.Structure):
    """lv_wb_encode_totals."""
    _fields_ = [(n, ctypes.c_uint64) for n in ENCODE_TOTALS]


class EncodeOut(ctypes.Structure):
    """lv_wb_encode_out."""
    _fields_ = [("d_out", ctypes.c_void_p), ("out_cap", ctypes.c_size_t), ("d_rec_off", ctypes.c_void_p),
                ("d_rec_len", ctypes.c_void_p), ("d_ops_out", ctypes.c_void_p), ("d_totals", ctypes.c_void_p)]


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
    L.lv_write_batch_encode_workspace_bytes.restype = sz
    L.lv_write_batch_encode_workspace_bytes.argtypes = [sz, sz]
    L.lv_write_batch_encode_device.restype = ctypes.c_int
    L.lv_write_batch_encode_device.argtypes = [vp, sz, vp, sz, vp, vp, vp, sz, ctypes.c_uint64,
                                               ctypes.POINTER(EncodeOut), ctypes.c_uint32, vp, sz, vp]
    L.lv_write_batch_encode_host.restype = ctypes.c_int
    L.lv_write_batch_encode_host.argtypes = [vp, sz, vp, sz, vp, sz, ctypes.c_uint64, vp, sz, vp, vp, vp,
                                             ctypes.POINTER(EncodeTotals)]
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


# ---- the inverse: ops over an arena to WriteBatch records ----
def encode_bound(records, ops, key_bytes, value_bytes) -> int:
    """An out_cap that always suffices (write_batch.h, OUT_OVER)."""
    return 12 * records + 11 * ops + key_bytes + value_bytes


def encode_host(src, ops, rec_op, first_sequence, *, records=None, op_cap=None, out_cap=None, sizing=False,
                src_bytes=None, want_ops=True):
    """lv_write_batch_encode_host: (out bytes, rec_off, rec_len, ops_out,
    totals dict).  `ops` is an OP_DTYPE array, rec_op the records + 1 bounds
    into it.  out_cap defaults to the size the call itself reports (a sizing
    call first); sizing=True is the sizing mode alone (out is None, and src may
    be None with src_bytes: it is only bounds-checked).  With a status only the
    totals are meaningful: out is empty and the arrays are as allocated
    (zeros)."""
    L = _bind()
    arr = np.ascontiguousarray(ops, dtype=OP_DTYPE)
    bounds = np.ascontiguousarray(rec_op, dtype=np.uint64)
    records = bounds.size - 1 if records is None else int(records)
    op_cap = arr.size if op_cap is None else int(op_cap)
    if src is None:
        sbuf, sn = None, int(src_bytes or 0)
    else:
        src = bytes(src)
        sbuf, sn = ctypes.create_string_buffer(src, max(len(src), 1)), (len(src) if src_bytes is None else int(src_bytes))
    rec_off = np.zeros(max(records, 1), dtype=np.uint64)
    rec_len = np.zeros(max(records, 1), dtype=np.uint64)
    ops_out = np.zeros(max(op_cap, 1), dtype=OP_DTYPE) if want_ops else None
    tot = EncodeTotals()

    def call(out, cap):
        rc = L.lv_write_batch_encode_host(sbuf, sn, arr.ctypes.data if arr.size else None, op_cap, bounds.ctypes.data,
                                          records, first_sequence & 0xFFFFFFFFFFFFFFFF, out, cap, rec_off.ctypes.data,
                                          rec_len.ctypes.data, ops_out.ctypes.data if want_ops else None,
                                          ctypes.byref(tot))
        if rc != 0:
            raise LvError(f"lv_write_batch_encode_host: {rc}")
        return {n: int(getattr(tot, n)) for n in ENCODE_TOTALS}

    t = call(None, 0)
    out = None
    if not sizing and not t["status"]:
        cap = t["out_bytes"] if out_cap is None else int(out_cap)
        buf = np.zeros(max(cap, 1), dtype=np.uint8)
        t = call(buf.ctypes.data, cap)
        out = b"" if t["status"] else buf[: t["out_bytes"]].tobytes()
    n = 0 if t["status"] else t["records"]
    k = 0 if t["status"] else t["ops"]
    return out, rec_off[:n].copy(), rec_len[:n].copy(), (ops_out[:k].copy() if want_ops else None), t


def encode_workspace_bytes(rec_cap: int, op_cap: int) -> int:
    return int(_bind().lv_write_batch_encode_workspace_bytes(rec_cap, op_cap))


class Encoded:
    """Outputs of encode_device, CUDA tensors written asynchronously: out_t
    (uint8, out_cap bytes), rec_off / rec_len (int64, rec_cap), ops_t (uint8,
    32 bytes per lv_wb_op; None without want_ops) and totals (int64[9],
    ENCODE_TOTALS).  (out_t, rec_off, rec_len, totals[0:1], totals[6:7]) is
    what decode_device takes; (out_t, ops_t, totals[1:2], totals[6:7]) what
    lvgpu.memtable.build_device takes."""

    def __init__(self, out_t, out_cap, rec_off, rec_len, ops_t, op_cap, totals, keep):
        self.out_t, self.out_cap, self.rec_off_t, self.rec_len_t = out_t, out_cap, rec_off, rec_len
        self.ops_t, self.op_cap, self.totals = ops_t, op_cap, totals
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
            self._tot = dict(zip(ENCODE_TOTALS, t))
            self._keep = None
        st = self._tot["status"]
        if st and check:
            names = "|".join(n for b, n in ENCODE_STATUS.items() if st & b)
            raise LvError(f"lv_write_batch_encode_device: status {names} (totals {self._tot})")
        return self._tot

    def out(self) -> bytes:
        """d_out[0, out_bytes) (synchronises)."""
        n = self.sync_totals()["out_bytes"]
        return self.out_t[:n].cpu().numpy().tobytes()

    def rec_off(self):
        n = self.sync_totals()["records"]
        return self.rec_off_t[:n].cpu().numpy().view(np.uint64).copy()

    def rec_len(self):
        n = self.sync_totals()["records"]
        return self.rec_len_t[:n].cpu().numpy().view(np.uint64).copy()

    def ops(self):
        """d_ops_out as a numpy structured array (OP_DTYPE; synchronises)."""
        n = self.sync_totals()["ops"]
        if self.ops_t is None:
            raise LvError("encode_device ran with want_ops=False")
        return self.ops_t[: n * 32].cpu().numpy().view(OP_DTYPE).copy()


def encode_device(src, ops, rec_op, records, upstream_status=None, *, first_sequence, rec_cap=None, op_cap=None,
                  out_cap=None, workspace=None, stream=None, fill=None, guard: int = 0, want_ops: bool = True,
                  out=None, flags: int = 0):
    """lv_write_batch_encode_device.  `src` and `ops` are uint8 CUDA tensors
    (ops: 32 bytes per lv_wb_op, e.g. Ops.ops_t of decode_device), rec_op an
    int64 CUDA tensor of the records + 1 bounds (e.g. Ops.rec_op); `records`
    and `upstream_status` int64 CUDA tensors whose first element is read on the
    device.  rec_cap defaults to rec_op.numel() - 1, op_cap to ops.numel() //
    32, out_cap to the bound 12 rec_cap + 11 op_cap + src.numel() when no key
    or value repeats -- pass it (encode_bound, or a sizing encode_host) when
    extents overlap.  `out`, a uint8 CUDA tensor, is written instead of a fresh
    allocation (out_cap defaults to its size).  fill, a byte value,
    initialises the output arrays with it first and guard allocates that many
    more bytes behind each (canaries).  Returns an Encoded; asynchronous on
    `stream`."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind()
    if src.dtype != torch.uint8 or ops.dtype != torch.uint8:
        raise LvError("src and ops must be uint8 tensors (numel() counts bytes)")
    dev = src.device
    for name, t in (("rec_op", rec_op), ("records", records), ("upstream_status", upstream_status)):
        if t is None and name == "upstream_status":
            continue
        if t is None or t.dtype != torch.int64 or t.device != dev or t.numel() < 1:
            raise LvError(f"{name} must be an int64 tensor on the source's device")
    if ops.device != dev or (workspace is not None and (workspace.dtype != torch.uint8 or workspace.device != dev)):
        raise LvError("ops and workspace must be uint8 tensors on the source's device")
    rec_cap = rec_op.numel() - 1 if rec_cap is None else int(rec_cap)
    op_cap = ops.numel() // 32 if op_cap is None else int(op_cap)
    if ops.numel() < op_cap * 32:
        raise LvError("ops must hold op_cap entries of 32 bytes")
    if out is not None:
        if out.dtype != torch.uint8 or out.device != dev:
            raise LvError("out must be a uint8 tensor on the source's device")
        out_cap = out.numel() if out_cap is None else int(out_cap)
        if out.numel() < out_cap:
            raise LvError("out must hold out_cap bytes")
    elif out_cap is None:
        out_cap = 12 * rec_cap + 11 * op_cap + src.numel()
    out_cap = int(out_cap)
    if workspace is None:
        workspace = torch.empty(max(L.lv_write_batch_encode_workspace_bytes(rec_cap, op_cap), 16), dtype=torch.uint8,
                                device=dev)

    def alloc(nbytes):
        nbytes = (max(nbytes, 16) + guard + 15) & ~15
        if fill is None:
            return torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
    out_t = alloc(out_cap) if out is None else out
    rec_off = alloc(rec_cap * 8).view(torch.int64)
    rec_len = alloc(rec_cap * 8).view(torch.int64)
    ops_t = alloc(op_cap * 32) if want_ops else None
    totals = torch.empty(len(ENCODE_TOTALS), dtype=torch.int64, device=dev)
    o = EncodeOut()
    o.d_out, o.out_cap = _dev_ptr(out_t, "out"), out_cap
    o.d_rec_off, o.d_rec_len = _dev_ptr(rec_off, "rec_off"), _dev_ptr(rec_len, "rec_len")
    o.d_ops_out = _dev_ptr(ops_t, "ops_out")
    o.d_totals = _dev_ptr(totals, "totals")
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_write_batch_encode_device(_dev_ptr(src, "src"), src.numel(), _dev_ptr(ops, "ops"), op_cap,
                                            _dev_ptr(rec_op, "rec_op"), _dev_ptr(records, "records"),
                                            _dev_ptr(upstream_status, "upstream_status"), rec_cap,
                                            first_sequence & 0xFFFFFFFFFFFFFFFF, ctypes.byref(o), flags,
                                            _dev_ptr(workspace, "workspace"), workspace.numel(), _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_write_batch_encode_device: {lib().lv_last_error().decode()}")
    return Encoded(out_t, out_cap, rec_off, rec_len, ops_t, op_cap, totals,
                   (src, ops, rec_op, records, upstream_status, workspace))
