"""Python mirror of the WAL record layer over the C ABI in include/lvgpu/wal.h.

    Scan.host(log, device)            GPU framing + CRC of every physical record
    scan_device(log_tensor, cap)      the same for a log already in HBM, no host sync
    Reader(log, scan, reporter, checksum, initial_offset)
                                      Reader::new / read_record / last_record_offset
                                      (log_reader.rs:75-120, :99)
    encode(records, dest_length)      Writer::add_record over many records with one
                                      GPU batch for the header CRCs (log_writer.rs:62-134)
    encode_size(rec_len, dest_length) bytes and fragments of that layout (host, no GPU)
    encode_device(payload_tensor, rec_off, rec_len, dest_length)
                                      the same log written in HBM from a payload in HBM:
                                      fragment CRCs + wal_frame_kernel, no host sync
    decode_device(log_tensor, hdr_off, crc, info, count)
                                      the inverse: Reader::read_record (initial_offset 0)
                                      replayed in HBM over scan_device's arrays -- records
                                      packed end to end, their offsets / lengths /
                                      last_record_offset, the corruption reports in order,
                                      totals; no host sync until .records() / .reports()
    decode_workspace_bytes(scan_cap)  device workspace of decode_device
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import LvError, lib

BLOCK_SIZE = 32768
HEADER_SIZE = 7
REC_OK, REC_BAD_LENGTH, REC_ZERO = 0, 1, 2

DECODE_NO_CHECKSUM = 0x1  # LV_WAL_DECODE_NO_CHECKSUM
# LV_WAL_DROP_*: the strings lv_wal_reader reports (log_reader.rs:120-364)
DROP_REASONS = {
    1: "bad record length",
    2: "checksum mismatch",
    3: "error in middle of record",
    4: "partial record without end(1)",
    5: "partial record without end(2)",
    6: "missing start of fragmented record(1)",
    7: "missing start of fragmented record(2)",
    8: "unexpected record type",
    9: "unknown record type",
}
# LV_WAL_DECODE_*_OVER
DECODE_STATUS = {1: "SCAN_OVER", 2: "REC_OVER", 4: "PAYLOAD_OVER", 8: "REPORT_OVER"}
DECODE_TILE = 1024  # entries per tile of the decode's scan (kDecTile, csrc/wal_decode.hip)


class DecodeOut(ctypes.Structure):
    """lv_wal_decode_out (include/lvgpu/wal.h)."""
    _fields_ = [("d_payload", ctypes.c_void_p), ("payload_cap", ctypes.c_size_t),
                ("d_rec_off", ctypes.c_void_p), ("d_rec_len", ctypes.c_void_p), ("d_rec_log_off", ctypes.c_void_p),
                ("rec_cap", ctypes.c_size_t),
                ("d_rep_bytes", ctypes.c_void_p), ("d_rep_log_off", ctypes.c_void_p), ("d_rep_reason", ctypes.c_void_p),
                ("rep_cap", ctypes.c_size_t),
                ("d_totals", ctypes.c_void_p)]


_REPORTER = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p)
_bound = False


def _bind():
    global _bound
    L = lib()
    if _bound:
        return L
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    L.lv_wal_scan_host.restype = vp
    L.lv_wal_scan_host.argtypes = [vp, sz, ctypes.c_int]
    L.lv_wal_scan_host_pipelined.restype = vp
    L.lv_wal_scan_host_pipelined.argtypes = [vp, sz, ctypes.c_int]
    L.lv_wal_scan_wait.restype = ctypes.c_int
    L.lv_wal_scan_wait.argtypes = [vp]
    L.lv_wal_scan_count.restype = sz
    L.lv_wal_scan_count.argtypes = [vp]
    for f in ("lv_wal_scan_offsets", "lv_wal_scan_crcs", "lv_wal_scan_info"):
        getattr(L, f).restype = vp
        getattr(L, f).argtypes = [vp]
    L.lv_wal_scan_from_arrays.restype = vp
    L.lv_wal_scan_from_arrays.argtypes = [vp, vp, vp, sz]
    L.lv_wal_scan_free.restype = None
    L.lv_wal_scan_free.argtypes = [vp]
    L.lv_wal_reader_new.restype = vp
    L.lv_wal_reader_new.argtypes = [vp, sz, vp, _REPORTER, vp, ctypes.c_int, u64]
    L.lv_wal_reader_read_record.restype = ctypes.c_int
    L.lv_wal_reader_read_record.argtypes = [vp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    L.lv_wal_reader_last_record_offset.restype = u64
    L.lv_wal_reader_last_record_offset.argtypes = [vp]
    L.lv_wal_reader_free.restype = None
    L.lv_wal_reader_free.argtypes = [vp]
    L.lv_wal_scan_workspace_bytes.restype = sz
    L.lv_wal_scan_workspace_bytes.argtypes = [sz, sz]
    L.lv_wal_scan_device.restype = ctypes.c_int
    L.lv_wal_scan_device.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, sz, vp]
    L.lv_wal_encode_host.restype = ctypes.c_int
    L.lv_wal_encode_host.argtypes = [vp, vp, vp, sz, u64, vp, sz, ctypes.POINTER(ctypes.c_size_t), ctypes.c_int]
    L.lv_wal_encode_size.restype = sz
    L.lv_wal_encode_size.argtypes = [vp, sz, u64, ctypes.POINTER(ctypes.c_size_t)]
    L.lv_wal_encode_workspace_bytes.restype = sz
    L.lv_wal_encode_workspace_bytes.argtypes = [sz]
    L.lv_wal_encode_device.restype = ctypes.c_int
    L.lv_wal_encode_device.argtypes = [vp, u64, vp, vp, sz, u64, vp, sz, ctypes.POINTER(ctypes.c_size_t), vp, sz, vp]
    L.lv_wal_decode_workspace_bytes.restype = sz
    L.lv_wal_decode_workspace_bytes.argtypes = [sz]
    L.lv_wal_decode_device.restype = ctypes.c_int
    L.lv_wal_decode_device.argtypes = [vp, sz, vp, vp, vp, vp, sz, ctypes.POINTER(DecodeOut), ctypes.c_uint32, vp, sz,
                                       vp]
    _bound = True
    return L


def _err(what):
    raise LvError(f"{what}: {lib().lv_last_error().decode()}")


class Scan:
    """Physical records of a log with their CRC units' value()."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def host(cls, log: bytes, device: int = 0) -> "Scan":
        L = _bind()
        buf = ctypes.create_string_buffer(bytes(log), max(len(log), 1))
        h = L.lv_wal_scan_host(buf, len(log), device)
        if not h:
            _err("lv_wal_scan_host")
        return cls(h)

    @classmethod
    def host_pipelined(cls, log: bytes, device: int = 0) -> "Scan":
        """lv_wal_scan_host_pipelined: returns at once; a Reader over it waits
        only for the 32 MiB chunk holding its next header."""
        L = _bind()
        buf = ctypes.create_string_buffer(bytes(log), max(len(log), 1))
        h = L.lv_wal_scan_host_pipelined(buf, len(log), device)
        if not h:
            _err("lv_wal_scan_host_pipelined")
        s = cls(h)
        s._buf = buf  # the worker reads the log until the scan is freed
        return s

    def wait(self) -> None:
        if _bind().lv_wal_scan_wait(self._h):
            _err("lv_wal_scan_wait")

    @classmethod
    def from_arrays(cls, offsets, crcs, info) -> "Scan":
        L = _bind()
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        c = np.ascontiguousarray(crcs, dtype=np.uint32)
        i = np.ascontiguousarray(info, dtype=np.uint32)
        h = L.lv_wal_scan_from_arrays(o.ctypes.data, c.ctypes.data, i.ctypes.data, o.size)
        if not h:
            _err("lv_wal_scan_from_arrays")
        return cls(h)

    def _arr(self, fn, dtype):
        L = _bind()
        n = L.lv_wal_scan_count(self._h)
        if n == 0:
            return np.zeros(0, dtype=dtype)
        p = getattr(L, fn)(self._h)
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dtype))),
                                     shape=(n,)).copy()

    @property
    def offsets(self):
        return self._arr("lv_wal_scan_offsets", np.uint64)

    @property
    def crcs(self):
        return self._arr("lv_wal_scan_crcs", np.uint32)

    @property
    def info(self):
        return self._arr("lv_wal_scan_info", np.uint32)

    def __del__(self):
        if getattr(self, "_h", None):
            _bind().lv_wal_scan_free(self._h)
            self._h = None


def scan_device(log, cap: int, workspace=None, stream=None):
    """lv_wal_scan_device over a uint8 CUDA tensor holding the log (8-B
    aligned): returns (hdr_off int64, crc int32, info int32, count int64[1])
    CUDA tensors, asynchronous on `stream`.  count[0] > cap means the capacity
    was too small and nothing else was written."""
    import torch
    from . import LvError, _dev_ptr, _stream_ptr
    L = _bind()
    if log.dtype != torch.uint8:
        raise LvError(f"log must be a uint8 tensor (got {log.dtype}: numel() would not count bytes)")
    if workspace is not None and (workspace.dtype != torch.uint8 or workspace.device != log.device):
        raise LvError("workspace must be a uint8 tensor on the log's device")
    dev = log.device
    hdr = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
    crc = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    info = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    need = L.lv_wal_scan_workspace_bytes(log.numel(), cap)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_wal_scan_device(_dev_ptr(log, "log"), log.numel(), _dev_ptr(hdr, "hdr"), _dev_ptr(crc, "crc"),
                                  _dev_ptr(info, "info"), cap, _dev_ptr(count, "count"),
                                  _dev_ptr(workspace, "workspace"), workspace.numel(), _stream_ptr(stream))
    if rc != 0:
        _err("lv_wal_scan_device")
    return hdr, crc, info, count


def scan_workspace_bytes(nbytes: int, cap: int) -> int:
    return int(_bind().lv_wal_scan_workspace_bytes(nbytes, cap))


class Reader:
    """log_reader.rs Reader over an in-memory log whose CRCs come from `scan`.
    `reporter` needs .corruption(nbytes, reason) (log_reader.rs:37-42)."""

    def __init__(self, log: bytes, scan: Scan, reporter=None, checksum: bool = True, initial_offset: int = 0):
        L = _bind()
        self._log = ctypes.create_string_buffer(bytes(log), max(len(log), 1))
        self._scan = scan
        self._reporter = reporter

        def cb(_ctx, nbytes, reason):
            if self._reporter is not None:
                self._reporter.corruption(int(nbytes), reason.decode())
        self._cb = _REPORTER(cb)
        self._h = L.lv_wal_reader_new(self._log, len(log), scan._h if scan else None,
                                      self._cb if reporter is not None else _REPORTER(0), None,
                                      1 if checksum else 0, initial_offset)
        if not self._h:
            _err("lv_wal_reader_new")

    def read_record(self):
        """The next logical record (bytes), or None at end of input."""
        L = _bind()
        p = ctypes.c_void_p()
        n = ctypes.c_size_t()
        rc = L.lv_wal_reader_read_record(self._h, ctypes.byref(p), ctypes.byref(n))
        if rc < 0:
            _err("lv_wal_reader_read_record")
        if rc == 0:
            return None
        return ctypes.string_at(p.value, n.value) if n.value else b""

    def last_record_offset(self) -> int:
        return int(_bind().lv_wal_reader_last_record_offset(self._h))

    def __del__(self):
        if getattr(self, "_h", None):
            _bind().lv_wal_reader_free(self._h)
            self._h = None


def encode(records, dest_length: int = 0, device: int = 0) -> bytes:
    """Bytes Writer::add_record appends for `records` (log_writer.rs:62-134),
    header CRCs computed in one GPU batch."""
    L = _bind()
    recs = [bytes(r) for r in records]
    payload = b"".join(recs)
    off = np.zeros(len(recs), dtype=np.uint64)
    ln = np.array([len(r) for r in recs], dtype=np.uint64)
    if len(recs) > 1:
        off[1:] = np.cumsum(ln[:-1])
    pbuf = ctypes.create_string_buffer(payload, max(len(payload), 1))
    need = ctypes.c_size_t()
    L.lv_wal_encode_host(pbuf, off.ctypes.data, ln.ctypes.data, len(recs), dest_length, None, 0,
                         ctypes.byref(need), device)
    out = ctypes.create_string_buffer(max(need.value, 1))
    rc = L.lv_wal_encode_host(pbuf, off.ctypes.data, ln.ctypes.data, len(recs), dest_length, out, need.value,
                              ctypes.byref(need), device)
    if rc != 0:
        _err("lv_wal_encode_host")
    return out.raw[: need.value]


def encode_size(rec_len, dest_length: int = 0):
    """(bytes, fragments) Writer::add_record appends for records of these
    lengths to a log of dest_length bytes (lv_wal_encode_size; host, no GPU)."""
    L = _bind()
    ln = np.ascontiguousarray(rec_len, dtype=np.uint64)
    frags = ctypes.c_size_t()
    nbytes = L.lv_wal_encode_size(ln.ctypes.data, ln.size, dest_length, ctypes.byref(frags))
    return int(nbytes), int(frags.value)


def encode_workspace_bytes(fragments: int) -> int:
    return int(_bind().lv_wal_encode_workspace_bytes(fragments))


def encode_device(payload, rec_off, rec_len, dest_length: int = 0, out=None, workspace=None, stream=None):
    """lv_wal_encode_device: the bytes Writer::add_record appends for the
    records payload[rec_off[i] : rec_off[i] + rec_len[i]] (host arrays; any
    order, overlaps allowed), written in HBM.  `payload` is a uint8 CUDA tensor;
    returns a uint8 CUDA tensor view of exactly the appended bytes (of `out` if
    given: a uint8 tensor on the payload's device, at least encode_size bytes).
    Asynchronous on `stream`."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind()
    if payload.dtype != torch.uint8:
        raise LvError(f"payload must be a uint8 tensor (got {payload.dtype}: numel() would not count bytes)")
    dev = payload.device
    for name, t in (("out", out), ("workspace", workspace)):
        if t is not None and (t.dtype != torch.uint8 or t.device != dev):
            raise LvError(f"{name} must be a uint8 tensor on the payload's device")
    off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    ln = np.ascontiguousarray(rec_len, dtype=np.uint64)
    if off.size != ln.size:
        raise LvError("rec_off/rec_len size mismatch")
    nbytes, frags = encode_size(ln, dest_length)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(L.lv_wal_encode_workspace_bytes(frags), dtype=torch.uint8, device=dev)
    got = ctypes.c_size_t()
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_wal_encode_device(_dev_ptr(payload, "payload"), payload.numel(), off.ctypes.data, ln.ctypes.data,
                                    ln.size, dest_length, _dev_ptr(out, "out"), out.numel(), ctypes.byref(got),
                                    _dev_ptr(workspace, "workspace"), workspace.numel(), _stream_ptr(stream))
    if rc != 0:
        _err("lv_wal_encode_device")
    return out[: got.value]


def decode_workspace_bytes(scan_cap: int) -> int:
    return int(_bind().lv_wal_decode_workspace_bytes(scan_cap))


class Decoded:
    """Outputs of decode_device, all CUDA tensors written asynchronously:
    payload (uint8), rec_off / rec_len / rec_log_off (int64), rep_bytes /
    rep_log_off (int64) and rep_reason (int32) -- None when reports are only
    counted -- and totals (int64[5]: records, payload_bytes, reports,
    dropped_bytes, status)."""

    def __init__(self, payload, rec_off, rec_len, rec_log_off, rep_bytes, rep_log_off, rep_reason, totals, keep):
        self.payload, self.rec_off, self.rec_len, self.rec_log_off = payload, rec_off, rec_len, rec_log_off
        self.rep_bytes, self.rep_log_off, self.rep_reason, self.totals = rep_bytes, rep_log_off, rep_reason, totals
        self._keep = keep  # the inputs and the workspace, until the work has run
        self._tot = None

    def sync_totals(self) -> dict:
        """Waits for the decode; the totals as a dict.  Raises LvError naming
        the status bits if a capacity was exceeded (nothing else was written)."""
        if self._tot is None:
            import torch
            torch.cuda.synchronize(self.totals.device)
            t = [int(v) for v in self.totals.cpu().numpy().view(np.uint64)]
            self._tot = dict(zip(("records", "payload_bytes", "reports", "dropped_bytes", "status"), t))
            self._keep = None
        st = self._tot["status"]
        if st:
            names = "|".join(n for b, n in DECODE_STATUS.items() if st & b)
            raise LvError(f"lv_wal_decode_device: status {names} (totals {self._tot})")
        return self._tot

    def records(self):
        """The logical records, list[bytes] (synchronises)."""
        t = self.sync_totals()
        n = t["records"]
        pay = self.payload[: t["payload_bytes"]].cpu().numpy().tobytes()
        off = self.rec_off[:n].cpu().numpy()
        ln = self.rec_len[:n].cpu().numpy()
        return [pay[int(o):int(o + k)] for o, k in zip(off, ln)]

    def record_log_offsets(self):
        """Reader::last_record_offset after each record (synchronises)."""
        return [int(v) for v in self.rec_log_off[: self.sync_totals()["records"]].cpu().numpy()]

    def reports(self):
        """[(bytes, reason string)] in the Reader's order (synchronises)."""
        t = self.sync_totals()
        if self.rep_bytes is None:
            raise LvError("decode_device ran with reports=False: they were only counted")
        n = t["reports"]
        b = self.rep_bytes[:n].cpu().numpy()
        r = self.rep_reason[:n].cpu().numpy()
        return [(int(x), DROP_REASONS[int(y)]) for x, y in zip(b, r)]


def decode_device(log, hdr_off, crc, info, count, *, checksum: bool = True, payload=None, workspace=None,
                  stream=None, reports: bool = True, rec_cap=None, rep_cap=None, scan_cap=None, fill=None):
    """lv_wal_decode_device over the tensors scan_device returned for `log` (a
    uint8 CUDA tensor, 8-B aligned): Reader::read_record with initial_offset 0,
    replayed in HBM.  Returns a Decoded; asynchronous on `stream`.  `payload`
    (uint8, any alignment, not overlapping the log) defaults to log.numel()
    bytes; rec_cap / rep_cap default to scan_cap / 2 * scan_cap, which always
    suffice.  checksum=False is LV_WAL_DECODE_NO_CHECKSUM (crc may be None);
    reports=False passes NULL report arrays: reports are only counted.
    scan_cap is the capacity scan_device ran with (default hdr_off.numel(),
    right for any cap >= 1); fill, a byte value, initialises the record and
    report arrays with it first (canaries)."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind()
    if log.dtype != torch.uint8:
        raise LvError(f"log must be a uint8 tensor (got {log.dtype}: numel() would not count bytes)")
    dev = log.device
    for name, t, dt in (("hdr_off", hdr_off, torch.int64), ("crc", crc, torch.int32), ("info", info, torch.int32),
                        ("count", count, torch.int64), ("payload", payload, torch.uint8),
                        ("workspace", workspace, torch.uint8)):
        if t is None and (name in ("payload", "workspace") or (name == "crc" and not checksum)):
            continue
        if t is None or t.dtype != dt or t.device != dev:
            raise LvError(f"{name} must be a {dt} tensor on the log's device")
    scan_cap = int(hdr_off.numel()) if scan_cap is None else int(scan_cap)
    if hdr_off.numel() < scan_cap or info.numel() < scan_cap or (crc is not None and crc.numel() < scan_cap) or count.numel() < 1:
        raise LvError("crc / info must hold hdr_off.numel() entries and count one")
    rec_cap = scan_cap if rec_cap is None else int(rec_cap)
    rep_cap = (2 * scan_cap if rep_cap is None else int(rep_cap)) if reports else 0
    if payload is None:
        payload = torch.empty(log.numel(), dtype=torch.uint8, device=dev)
    if workspace is None:
        workspace = torch.empty(L.lv_wal_decode_workspace_bytes(scan_cap), dtype=torch.uint8, device=dev)
    def alloc(n, dt):
        if fill is None:
            return torch.empty(max(n, 1), dtype=dt, device=dev)
        width = torch.empty(0, dtype=dt).element_size()
        return torch.full((max(n, 1) * width,), fill, dtype=torch.uint8, device=dev).view(dt)
    i64 = lambda n: alloc(n, torch.int64)
    rec_off, rec_len, rec_log = i64(rec_cap), i64(rec_cap), i64(rec_cap)
    rep_bytes = rep_log = rep_reason = None
    if reports:
        rep_bytes, rep_log = i64(rep_cap), i64(rep_cap)
        rep_reason = alloc(rep_cap, torch.int32)
    totals = torch.empty(5, dtype=torch.int64, device=dev)
    o = DecodeOut()
    o.d_payload, o.payload_cap = _dev_ptr(payload, "payload"), payload.numel()
    o.d_rec_off, o.d_rec_len, o.d_rec_log_off = (_dev_ptr(t, "rec") for t in (rec_off, rec_len, rec_log))
    o.rec_cap = rec_cap
    o.d_rep_bytes, o.d_rep_log_off, o.d_rep_reason = (_dev_ptr(t, "rep") for t in (rep_bytes, rep_log, rep_reason))
    o.rep_cap = rep_cap
    o.d_totals = _dev_ptr(totals, "totals")
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_wal_decode_device(_dev_ptr(log, "log"), log.numel(), _dev_ptr(hdr_off, "hdr_off"),
                                    _dev_ptr(crc, "crc"), _dev_ptr(info, "info"), _dev_ptr(count, "count"), scan_cap,
                                    ctypes.byref(o), 0 if checksum else DECODE_NO_CHECKSUM,
                                    _dev_ptr(workspace, "workspace"), workspace.numel(), _stream_ptr(stream))
    if rc != 0:
        _err("lv_wal_decode_device")
    return Decoded(payload, rec_off, rec_len, rec_log, rep_bytes, rep_log, rep_reason, totals,
                   (log, hdr_off, crc, info, count, workspace))
