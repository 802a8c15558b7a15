"""Python mirror of include/lvgpu/memtable.h: the op table of
lvgpu.write_batch in memtable order (internal-key order) and MemTable::get
(memtable.rs:105-143) over it, on the host and in HBM.

    compare(a, a_tag, b, b_tag)       lv_internal_key_compare: -1 / 0 / +1
    build_host(payload, ops)          lv_memtable_build_host: (order, totals)
    get_host(payload, ops, order, totals, key, seq)
                                      lv_memtable_get_host: a result dict
    build_workspace_bytes(op_cap)     device workspace of build_device
    build_device(payload, ops, n_ops, upstream_status)
                                      lv_memtable_build_device over what
                                      lvgpu.write_batch.decode_device wrote; no host
                                      sync until .sync_totals() / .order()
    get_device(table, qkeys, q_off, q_len, q_seq)
                                      lv_memtable_get_device: a uint8 CUDA tensor of
                                      lv_mt_get_result (RESULT_DTYPE), asynchronous
    pack_range_queries(queries)       (qkeys bytes, RANGE_QUERY_DTYPE array) of range queries
    range_host(payload, ops, order, totals, qkeys, query, limit, max_scan)
                                      lv_memtable_range_host: (hits, result dict)
    range_device(table, queries, qkeys, limit, max_scan)
                                      lv_memtable_range_device (DBIter's forward walk for a
                                      batch of ranges): a Ranges of CUDA tensors, asynchronous
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import LvError, lib
from .write_batch import OP_DTYPE

MAX_SEQUENCE = (1 << 56) - 1                                  # LV_MT_MAX_SEQUENCE
BUILD_STATUS = {1: "UPSTREAM", 2: "OP_OVER", 4: "BAD_OP"}     # LV_MT_BUILD_*
GET_ABSENT, GET_FOUND, GET_DELETED, GET_BAD_SEQ, GET_NO_TABLE, GET_BAD_QUERY = range(6)  # LV_MT_GET_*
TOTALS = ("entries", "user_keys", "status")
# csrc/lvk/knobs.h: LVK_MT_TILE (entries per LDS-sorted tile and per merge
# output tile) and LVK_MT_PREFIX (key bytes held in a sort entry).  The GPU
# tests sweep around them.
MT_TILE = 512
MT_PREFIX = 16

RESULT_DTYPE = np.dtype([("val_off", "<u8"), ("val_len", "<u4"), ("op", "<u4"), ("status", "<u4"),
                         ("reserved", "<u4")])
assert RESULT_DTYPE.itemsize == 24

RANGE_HAS_HI, RANGE_RESUME, RANGE_SEEN = 1, 2, 4                      # LV_MT_RANGE_* query flags
RANGE_DONE, RANGE_MORE_LIMIT, RANGE_MORE_SCAN = 0, 1, 2               # LV_MT_RANGE_* statuses; 3-5 are Get's
RANGE_QUERY_DTYPE = np.dtype([("lo_off", "<u8"), ("hi_off", "<u8"), ("seq", "<u8"), ("pos", "<u8"),
                              ("lo_len", "<u4"), ("hi_len", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
RANGE_RESULT_DTYPE = np.dtype([("seek_pos", "<u8"), ("next_pos", "<u8"), ("unparsed", "<u8"), ("count", "<u4"),
                               ("status", "<u4"), ("seen", "<u4"), ("reserved", "<u4")])
assert RANGE_QUERY_DTYPE.itemsize == 48 and RANGE_RESULT_DTYPE.itemsize == 40


class Totals(ctypes.Structure):
    """lv_mt_totals."""
    _fields_ = [("entries", ctypes.c_uint64), ("user_keys", ctypes.c_uint64), ("status", ctypes.c_uint64)]


class GetResult(ctypes.Structure):
    """lv_mt_get_result."""
    _fields_ = [("val_off", ctypes.c_uint64), ("val_len", ctypes.c_uint32), ("op", ctypes.c_uint32),
                ("status", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


_bound = False


def _bind():
    global _bound
    L = lib()
    if _bound:
        return L
    vp, sz, u64, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32
    L.lv_internal_key_compare.restype = ctypes.c_int
    L.lv_internal_key_compare.argtypes = [vp, sz, u64, vp, sz, u64]
    L.lv_memtable_build_host.restype = ctypes.c_int
    L.lv_memtable_build_host.argtypes = [vp, sz, vp, sz, vp, ctypes.POINTER(Totals)]
    L.lv_memtable_get_host.restype = ctypes.c_int
    L.lv_memtable_get_host.argtypes = [vp, sz, vp, vp, ctypes.POINTER(Totals), vp, sz, u64,
                                       ctypes.POINTER(GetResult)]
    L.lv_memtable_build_workspace_bytes.restype = sz
    L.lv_memtable_build_workspace_bytes.argtypes = [sz]
    L.lv_memtable_build_device.restype = ctypes.c_int
    L.lv_memtable_build_device.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, u32, vp, sz, vp]
    L.lv_memtable_get_device.restype = ctypes.c_int
    L.lv_memtable_get_device.argtypes = [vp, sz, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp, u32, vp]
    L.lv_memtable_range_host.restype = ctypes.c_int
    L.lv_memtable_range_host.argtypes = [vp, sz, vp, vp, ctypes.POINTER(Totals), sz, vp, sz, vp, u32, u64, vp, vp]
    L.lv_memtable_range_device.restype = ctypes.c_int
    L.lv_memtable_range_device.argtypes = [vp, sz, vp, vp, vp, sz, vp, sz, vp, sz, u32, u64, vp, vp, u32, vp]
    _bound = True
    return L


def _buf(b):
    b = bytes(b)
    return ctypes.create_string_buffer(b, max(len(b), 1)), len(b)


def compare(a, a_tag, b, b_tag) -> int:
    """lv_internal_key_compare over (user key a, tag) and (user key b, tag)."""
    L = _bind()
    ab, an = _buf(a)
    bb, bn = _buf(b)
    return int(L.lv_internal_key_compare(ab, an, a_tag, bb, bn, b_tag))


def _ops_array(ops):
    arr = np.ascontiguousarray(ops, dtype=OP_DTYPE)
    return arr, (arr.ctypes.data if arr.size else None)


def build_host(payload, ops):
    """lv_memtable_build_host: (order as a uint32 array, totals dict).  With a
    status the order is empty."""
    L = _bind()
    pb, pn = _buf(payload)
    arr, ap = _ops_array(ops)
    order = np.zeros(max(arr.size, 1), dtype=np.uint32)
    tot = Totals()
    rc = L.lv_memtable_build_host(pb, pn, ap, arr.size, order.ctypes.data, ctypes.byref(tot))
    if rc != 0:
        raise LvError(f"lv_memtable_build_host: {rc}")
    t = dict(entries=int(tot.entries), user_keys=int(tot.user_keys), status=int(tot.status))
    return (order[:0] if t["status"] else order[: arr.size]), t


def get_host(payload, ops, order, totals, key, seq) -> dict:
    """lv_memtable_get_host for one query: a dict of the result's fields."""
    L = _bind()
    pb, pn = _buf(payload)
    arr, ap = _ops_array(ops)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    kb, kn = _buf(key)
    tot = Totals(totals["entries"], totals["user_keys"], totals["status"])
    r = GetResult()
    rc = L.lv_memtable_get_host(pb, pn, ap, order.ctypes.data if order.size else None, ctypes.byref(tot), kb, kn, seq,
                                ctypes.byref(r))
    if rc != 0:
        raise LvError(f"lv_memtable_get_host: {rc}")
    return dict(val_off=int(r.val_off), val_len=int(r.val_len), op=int(r.op), status=int(r.status),
                reserved=int(r.reserved))


def build_workspace_bytes(op_cap: int) -> int:
    return int(_bind().lv_memtable_build_workspace_bytes(op_cap))


class Table:
    """Outputs of build_device, CUDA tensors written asynchronously: order_t
    (int32, op_cap entries and the guard) and totals (int64[3], TOTALS), with
    the inputs a get needs."""

    def __init__(self, payload, ops_t, op_cap, order_t, totals, keep):
        self.payload, self.ops_t, self.op_cap, self.order_t, self.totals = payload, ops_t, op_cap, order_t, totals
        self._keep = keep  # the workspace and the counters, until the work has run
        self._tot = None

    def sync_totals(self, check: bool = True) -> dict:
        """Waits for the call; the totals as a dict.  Raises LvError naming the
        status bits if one is set (d_order was not written) unless check is
        False."""
        if self._tot is None:
            import torch
            torch.cuda.synchronize(self.totals.device)
            t = [int(v) for v in self.totals.cpu().numpy().view(np.uint64)]
            self._tot = dict(zip(TOTALS, t))
            self._keep = None
        st = self._tot["status"]
        if st and check:
            names = "|".join(n for b, n in BUILD_STATUS.items() if st & b)
            raise LvError(f"lv_memtable_build_device: status {names} (totals {self._tot})")
        return self._tot

    def order(self):
        """d_order[0, entries) as a uint32 numpy array (synchronises)."""
        n = self.sync_totals()["entries"]
        return self.order_t[:n].cpu().numpy().view(np.uint32).copy()


def build_device(payload, ops, n_ops, upstream_status=None, *, op_cap=None, workspace=None, stream=None, fill=None,
                 guard: int = 0, flags: int = 0):
    """lv_memtable_build_device.  `payload` and `ops` are uint8 CUDA tensors
    (ops: 32 bytes per lv_wb_op, e.g. Ops.ops_t of lvgpu.write_batch); `n_ops`
    and `upstream_status` int64 CUDA tensors whose first element is read on the
    device (e.g. Ops.totals[1:2] and Ops.totals[6:7]).  op_cap defaults to
    ops.numel() // 32.  fill, a byte value, initialises d_order with it first
    and guard allocates that many more bytes behind it (canaries).  Returns a
    Table; asynchronous on `stream`."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind()
    if payload.dtype != torch.uint8 or ops.dtype != torch.uint8:
        raise LvError("payload and ops must be uint8 tensors")
    dev = payload.device
    for name, t in (("n_ops", n_ops), ("upstream_status", upstream_status)):
        if t is None and name == "upstream_status":
            continue
        if t is None or t.dtype != torch.int64 or t.device != dev or t.numel() < 1:
            raise LvError(f"{name} must be an int64 tensor on the payload's device")
    if ops.device != dev or (workspace is not None and (workspace.dtype != torch.uint8 or workspace.device != dev)):
        raise LvError("ops and workspace must be uint8 tensors on the payload's device")
    op_cap = ops.numel() // 32 if op_cap is None else int(op_cap)
    if ops.numel() < op_cap * 32:
        raise LvError("ops must hold op_cap entries of 32 bytes")
    if workspace is None:
        workspace = torch.empty(max(L.lv_memtable_build_workspace_bytes(op_cap), 16), dtype=torch.uint8, device=dev)
    nbytes = (max(op_cap * 4, 16) + guard + 7) & ~7
    if fill is None:
        order_t = torch.empty(nbytes, dtype=torch.uint8, device=dev).view(torch.int32)
    else:
        order_t = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev).view(torch.int32)
    totals = torch.empty(len(TOTALS), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_memtable_build_device(_dev_ptr(payload, "payload"), payload.numel(), _dev_ptr(ops, "ops"),
                                        _dev_ptr(n_ops, "n_ops"), _dev_ptr(upstream_status, "upstream_status"),
                                        op_cap, _dev_ptr(order_t, "order"), _dev_ptr(totals, "totals"), flags,
                                        _dev_ptr(workspace, "workspace"), workspace.numel(), _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_memtable_build_device: {lib().lv_last_error().decode()}")
    return Table(payload, ops, op_cap, order_t, totals, (n_ops, upstream_status, workspace))


def get_device(table, qkeys, q_off, q_len, q_seq, *, nq=None, stream=None, fill=None, guard: int = 0,
               flags: int = 0):
    """lv_memtable_get_device over a Table.  `qkeys` is a uint8 CUDA tensor,
    q_off / q_seq int64 and q_len int32 CUDA tensors of nq entries.  Returns a
    uint8 CUDA tensor of nq lv_mt_get_result (view it with results(); fill /
    guard as in build_device); asynchronous on `stream`."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind()
    dev = table.payload.device
    if qkeys.dtype != torch.uint8 or q_off.dtype != torch.int64 or q_seq.dtype != torch.int64 or \
            q_len.dtype != torch.int32:
        raise LvError("qkeys must be uint8, q_off and q_seq int64, q_len int32")
    nq = int(min(q_off.numel(), q_len.numel(), q_seq.numel())) if nq is None else int(nq)
    if min(q_off.numel(), q_len.numel(), q_seq.numel()) < nq:
        raise LvError("the query arrays must hold nq entries")
    nbytes = (max(nq * 24, 16) + guard + 7) & ~7
    if fill is None:
        res = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        res = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.lv_memtable_get_device(_dev_ptr(table.payload, "payload"), table.payload.numel(),
                                      _dev_ptr(table.ops_t, "ops"), _dev_ptr(table.order_t, "order"),
                                      _dev_ptr(table.totals, "totals"), _dev_ptr(qkeys, "qkeys"), qkeys.numel(),
                                      _dev_ptr(q_off, "q_off"), _dev_ptr(q_len, "q_len"), _dev_ptr(q_seq, "q_seq"), nq,
                                      _dev_ptr(res, "results"), flags, _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_memtable_get_device: {lib().lv_last_error().decode()}")
    return res


def results(res, nq):
    """The first nq results of get_device's tensor as a structured array
    (RESULT_DTYPE; synchronises)."""
    return res[: nq * 24].cpu().numpy().view(RESULT_DTYPE).copy()


# ---- lv_memtable_range_*: DBIter's forward walk over a sorted table ------------
def pack_range_queries(queries, gaps=None):
    """(qkeys bytes, RANGE_QUERY_DTYPE array) of queries, each (lo, hi | None,
    seq) -- a seek to lo at snapshot seq, up to hi if one is given -- or the
    resume tuple ("resume", pos, seen, hi | None, seq), which continues a walk
    from a result's (next_pos, seen).  gaps[i] bytes of 0xDD go in front of
    query i's keys."""
    qk, rows = bytearray(), np.zeros(len(queries), dtype=RANGE_QUERY_DTYPE)
    for i, q in enumerate(queries):
        if gaps is not None:
            qk += b"\xDD" * int(gaps[i])
        row = rows[i]
        if q[0] == "resume":
            _, pos, seen, hi, seq = q
            row["pos"], row["flags"] = pos, RANGE_RESUME | (RANGE_SEEN if seen else 0)
        else:
            lo, hi, seq = q
            row["lo_off"], row["lo_len"] = len(qk), len(lo)
            qk += lo
        if hi is not None:
            row["hi_off"], row["hi_len"] = len(qk), len(hi)
            row["flags"] |= RANGE_HAS_HI
            qk += hi
        row["seq"] = seq
    return bytes(qk), rows


def range_host(payload, ops, order, totals, qkeys, query, limit, max_scan, *, op_cap=None, canary=None):
    """lv_memtable_range_host for one query (a RANGE_QUERY_DTYPE row over
    `qkeys`): (hits[0, count) as a uint32 array, the result's fields as a
    dict).  canary: a uint32 the hit slot holds first; the whole slot is then
    returned, for checks of what was left untouched."""
    L = _bind()
    pb, pn = _buf(payload)
    kb, kn = _buf(qkeys)
    arr, ap = _ops_array(ops)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    tot = Totals(totals["entries"], totals["user_keys"], totals["status"])
    row = np.ascontiguousarray(np.asarray(query, dtype=RANGE_QUERY_DTYPE).reshape(1))
    hits = np.full(max(int(limit), 1), 0 if canary is None else canary, dtype=np.uint32)
    res = np.zeros(1, dtype=RANGE_RESULT_DTYPE)
    rc = L.lv_memtable_range_host(pb, pn, ap, order.ctypes.data if order.size else None, ctypes.byref(tot),
                                  arr.size if op_cap is None else op_cap, kb, kn, row.ctypes.data, limit, max_scan,
                                  hits.ctypes.data, res.ctypes.data)
    if rc != 0:
        raise LvError(f"lv_memtable_range_host: {rc}")
    r = {k: int(res[0][k]) for k in RANGE_RESULT_DTYPE.names}
    return (hits if canary is not None else hits[: r["count"]].copy()), r


class Ranges:
    """Outputs of range_device, CUDA tensors written asynchronously: hits_t
    (int32, nq slots of `limit` op indices and the guard) and results_t (uint8,
    nq lv_mt_range_result and the guard)."""

    def __init__(self, nq, limit, hits_t, results_t, keep):
        self.nq, self.limit, self.hits_t, self.results_t = nq, limit, hits_t, results_t
        self._keep = keep  # the queries and their keys, until the work has run

    def sync(self):
        """Waits for the call: (hits as a uint32 array of shape (nq, limit),
        results as a RANGE_RESULT_DTYPE array).  Row q's hits are its first
        results[q]["count"] entries."""
        import torch
        torch.cuda.synchronize(self.results_t.device)
        self._keep = None
        res = self.results_t[: self.nq * 40].cpu().numpy().view(RANGE_RESULT_DTYPE).copy()
        hits = self.hits_t[: self.nq * self.limit].cpu().numpy().view(np.uint32).reshape(self.nq, self.limit).copy()
        return hits, res

    def hit_lists(self):
        """sync(), each query's hits cut to its count: (list of lists, results)."""
        hits, res = self.sync()
        return [hits[q, : int(res[q]["count"])].tolist() for q in range(self.nq)], res


def range_device(table, queries, qkeys, limit, max_scan, *, nq=None, stream=None, fill=None, guard: int = 0,
                 flags: int = 0):
    """lv_memtable_range_device over a Table (a build's, a Scanned.memtable()
    or a lvgpu.compact.Filtered): its payload, ops, order and totals, read on
    the device.  `queries` is a RANGE_QUERY_DTYPE array (copied to the device
    here) or a uint8 CUDA tensor of 48-byte lv_mt_range_query rows that is
    already there, `qkeys` the bytes their extents point into (bytes, or a
    uint8 CUDA tensor).  fill, a byte value, initialises d_hits and d_results
    with it first and guard allocates that many more bytes behind each
    (canaries).  Returns a Ranges; asynchronous on `stream`."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind()
    dev = table.payload.device
    if torch.is_tensor(queries):
        if queries.dtype != torch.uint8 or queries.device != dev:
            raise LvError("queries must be a uint8 tensor on the payload's device")
        d_q = queries
        nq = queries.numel() // 48 if nq is None else int(nq)
        if queries.numel() < nq * 48:
            raise LvError("queries must hold nq rows of 48 bytes")
    else:
        rows = np.ascontiguousarray(queries, dtype=RANGE_QUERY_DTYPE)
        nq = rows.size if nq is None else int(nq)
        if rows.size < nq:
            raise LvError("queries must hold nq rows")
        d_q = torch.frombuffer(bytearray(rows.tobytes()) + bytearray(8), dtype=torch.uint8).to(dev)
    if torch.is_tensor(qkeys):
        if qkeys.dtype != torch.uint8 or qkeys.device != dev:
            raise LvError("qkeys must be a uint8 tensor on the payload's device")
        d_qk, qk_bytes = qkeys, qkeys.numel()
    else:
        qk_bytes = len(qkeys)
        d_qk = torch.frombuffer(bytearray(qkeys), dtype=torch.uint8).to(dev) if qk_bytes else None
    limit, max_scan = int(limit), int(max_scan)

    def alloc(used):
        nbytes = (max(used, 16) + guard + 7) & ~7
        if fill is None:
            return torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)

    hits_t = alloc(nq * max(limit, 1) * 4).view(torch.int32)
    results_t = alloc(nq * 40)
    op_cap = int(table.op_cap)
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_memtable_range_device(_dev_ptr(table.payload, "payload") if table.payload.numel() else None,
                                        table.payload.numel(), _dev_ptr(table.ops_t, "ops") if op_cap else None,
                                        _dev_ptr(table.order_t, "order") if op_cap else None,
                                        _dev_ptr(table.totals, "totals"), op_cap,
                                        _dev_ptr(d_qk, "qkeys") if qk_bytes else None, qk_bytes,
                                        _dev_ptr(d_q, "queries"), nq, limit, max_scan, _dev_ptr(hits_t, "hits"),
                                        _dev_ptr(results_t, "results"), flags, _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_memtable_range_device: {lib().lv_last_error().decode()}")
    return Ranges(nq, limit, hits_t, results_t, (table, d_q, d_qk))
