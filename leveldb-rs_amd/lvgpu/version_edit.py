"""Python mirror of include/lvgpu/version_edit.h: VersionEdit::decode_from and
encode_to (version_edit.rs:192-319) on the host and over records in HBM.

    decode_host(rec)                  lv_version_edit_decode_host: (status, edit dict,
                                      files, deleted, pointers) as structured arrays
    encode_host(src, edits, files, rec_file, deleted, rec_deleted, pointers, rec_pointer)
                                      lv_version_edit_encode_host: (out bytes, rec_off,
                                      rec_len, totals dict)
    decode_device(payload, rec_off, rec_len, records, upstream_status)
                                      lv_version_edit_decode_device: a Decoded with lazy
                                      .sync_totals() / .edits() / .files() / ...
    encode_device(src, edits, files, rec_file, deleted, rec_deleted, pointers,
                  rec_pointer, records, upstream_status)
                                      lv_version_edit_encode_device: an Encoded with lazy
                                      .sync_totals() / .out() / ...
    files_device(version_files, tables, file_count)
                                      lv_version_edit_files_device: a compaction's files
                                      as NewFile rows
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import LvError, lib

NUM_LEVELS = 7
(OK, UNKNOWN_TAG, INVALID_TAG, BAD_VARINT32, BAD_VARINT64, BAD_LENGTH, BAD_LEVEL, OUT_OF_RANGE) = range(8)  # LV_VE_*
STATUS_TEXT = {
    1: "unknown tag",
    2: "invalid tag",
    3: "Error when decoding varint-32",
    4: "Input doesn't contain a valid varint-64.",
    5: "Input slice doesn't contain a length-prefixed encoded value.",
    6: "exceeded max level",
}
HAS_COMPARATOR, HAS_LOG_NUMBER, HAS_PREV_LOG_NUMBER, HAS_NEXT_FILE, HAS_LAST_SEQUENCE = 1, 2, 4, 8, 16  # LV_VE_HAS_*
FLAG_NEG_LEVEL, FLAG_SHORT_KEY = 1, 2                                                                  # LV_VE_FLAG_*
DECODE_STATUS = {1: "UPSTREAM", 2: "REC_OVER", 4: "FILE_OVER", 8: "DELETED_OVER", 16: "POINTER_OVER"}
ENCODE_STATUS = {1: "UPSTREAM", 2: "REC_OVER", 4: "BAD_BOUNDS", 8: "BAD_ROW", 16: "OUT_OVER"}
KIND_EDIT, KIND_POINTER, KIND_DELETED, KIND_FILE = range(4)                                            # LV_VE_KIND_*
TOTALS = ("records", "files", "deleted", "pointers", "bad_records", "first_bad", "last_has0", "last_has1", "last_has2",
          "last_has3", "last_has4", "status")
ENCODE_TOTALS = ("records", "files", "deleted", "pointers", "key_bytes", "out_bytes", "status", "bad_record",
                 "bad_kind", "bad_row")
MAX_REC_CAP = (1 << 32) - 2
ENCODE_MAX_ROWS = 1 << 30
# csrc/version_edit.hip: kVdTile (records per decode tile), kVdSmall (records up
# to this many bytes take one lane), kVdWindow / kVdRound (the wave class's LDS
# window and its first load); kVeTile (items per encode scan tile), kVeWaveCopy /
# kVeCopyLanes (lvk::group_copy's classes).  The GPU tests sweep around them.
VD_TILE = 256
VD_SMALL = 16384
VD_WINDOW = 4096
VD_ROUND = 1024
VE_TILE = 1024
VE_WAVE_COPY = 64
VE_COPY_LANES = 16

EDIT_DTYPE = np.dtype([("log_number", "<u8"), ("prev_log_number", "<u8"), ("next_file_number", "<u8"),
                       ("last_sequence", "<u8"), ("comparator_off", "<u8"), ("comparator_len", "<u4"), ("has", "<u4"),
                       ("status", "<u4"), ("flags", "<u4"), ("reserved", "<u8")])
FILE_DTYPE = np.dtype([("number", "<u8"), ("file_size", "<u8"), ("smallest_off", "<u8"), ("largest_off", "<u8"),
                       ("smallest_len", "<u4"), ("largest_len", "<u4"), ("level", "<u4"), ("reserved", "<u4")])
DELETED_DTYPE = np.dtype([("number", "<u8"), ("level", "<u4"), ("reserved", "<u4")])
POINTER_DTYPE = np.dtype([("key_off", "<u8"), ("key_len", "<u4"), ("level", "<u4")])
assert (EDIT_DTYPE.itemsize, FILE_DTYPE.itemsize, DELETED_DTYPE.itemsize, POINTER_DTYPE.itemsize) == (64, 48, 16, 16)


class DecodeOut(ctypes.Structure):
    """lv_ve_decode_out."""
    _fields_ = [("d_edits", ctypes.c_void_p),
                ("d_files", ctypes.c_void_p), ("file_cap", ctypes.c_size_t), ("d_rec_file", ctypes.c_void_p),
                ("d_deleted", ctypes.c_void_p), ("deleted_cap", ctypes.c_size_t), ("d_rec_deleted", ctypes.c_void_p),
                ("d_pointers", ctypes.c_void_p), ("pointer_cap", ctypes.c_size_t), ("d_rec_pointer", ctypes.c_void_p),
                ("d_totals", ctypes.c_void_p)]


class EncodeIn(ctypes.Structure):
    """lv_ve_encode_in."""
    _fields_ = DecodeOut._fields_[:-1]


class EncodeTotals(ctypes.Structure):
    """lv_ve_encode_totals."""
    _fields_ = [(n, ctypes.c_uint64) for n in ENCODE_TOTALS]


class EncodeOut(ctypes.Structure):
    """lv_ve_encode_out."""
    _fields_ = [("d_out", ctypes.c_void_p), ("out_cap", ctypes.c_size_t), ("d_rec_off", ctypes.c_void_p),
                ("d_rec_len", ctypes.c_void_p), ("d_totals", ctypes.c_void_p)]


_bound = False


def _bind():
    global _bound
    L = lib()
    if _bound:
        return L
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.lv_version_edit_decode_host.restype = ctypes.c_uint32
    L.lv_version_edit_decode_host.argtypes = [vp, sz, vp, vp, sz, vp, sz, vp, sz, vp]
    L.lv_version_edit_decode_workspace_bytes.restype = sz
    L.lv_version_edit_decode_workspace_bytes.argtypes = [sz]
    L.lv_version_edit_decode_device.restype = ctypes.c_int
    L.lv_version_edit_decode_device.argtypes = [vp, sz, vp, vp, vp, vp, sz, ctypes.POINTER(DecodeOut), ctypes.c_uint32,
                                                vp, sz, vp]
    L.lv_version_edit_encode_workspace_bytes.restype = sz
    L.lv_version_edit_encode_workspace_bytes.argtypes = [sz, sz, sz, sz]
    L.lv_version_edit_encode_device.restype = ctypes.c_int
    L.lv_version_edit_encode_device.argtypes = [vp, sz, ctypes.POINTER(EncodeIn), vp, vp, sz,
                                                ctypes.POINTER(EncodeOut), ctypes.c_uint32, vp, sz, vp]
    L.lv_version_edit_encode_host.restype = ctypes.c_int
    L.lv_version_edit_encode_host.argtypes = [vp, sz, ctypes.POINTER(EncodeIn), sz, ctypes.POINTER(EncodeOut)]
    L.lv_version_edit_files_device.restype = ctypes.c_int
    L.lv_version_edit_files_device.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp]
    _bound = True
    return L


def encode_bound(records, pointers, deleted, files, key_bytes) -> int:
    """An out_cap that always suffices (version_edit.h, OUT_OVER)."""
    return 50 * records + 7 * pointers + 12 * deleted + 32 * files + key_bytes


# ---- host twins -------------------------------------------------------------------
def decode_host(rec, caps=None):
    """lv_version_edit_decode_host over `rec`: (status, edit, files, deleted,
    pointers, counts).  edit is a one-element EDIT_DTYPE array, the rows
    structured arrays with offsets into rec -- min(count, cap) of each (caps
    None: all of them; else a (file, deleted, pointer) triple); counts the
    rows found."""
    L = _bind()
    rec = bytes(rec)
    buf = ctypes.create_string_buffer(rec, max(len(rec), 1))
    counts = (ctypes.c_size_t * 3)()
    edit = np.zeros(1, dtype=EDIT_DTYPE)
    if caps is None:  # count, then fetch all
        L.lv_version_edit_decode_host(buf, len(rec), None, None, 0, None, 0, None, 0, counts)
        caps = tuple(counts)
    f = np.zeros(max(caps[0], 1), dtype=FILE_DTYPE)
    d = np.zeros(max(caps[1], 1), dtype=DELETED_DTYPE)
    p = np.zeros(max(caps[2], 1), dtype=POINTER_DTYPE)
    st = L.lv_version_edit_decode_host(buf, len(rec), edit.ctypes.data, f.ctypes.data if caps[0] else None, caps[0],
                                       d.ctypes.data if caps[1] else None, caps[1],
                                       p.ctypes.data if caps[2] else None, caps[2], counts)
    c = tuple(int(x) for x in counts)
    return int(st), edit, f[:min(c[0], caps[0])].copy(), d[:min(c[1], caps[1])].copy(), p[:min(c[2], caps[2])].copy(), c


def encode_host(src, edits, files, rec_file, deleted, rec_deleted, pointers, rec_pointer, *, records=None,
                caps=None, out_cap=None, sizing=False, src_bytes=None):
    """lv_version_edit_encode_host: (out bytes, rec_off, rec_len, totals dict).
    The tables are structured arrays (EDIT_DTYPE, ...), the bounds records + 1
    entries each.  out_cap defaults to the size a sizing call reports;
    sizing=True is the sizing mode alone (out is None; src may be None with
    src_bytes).  caps = (file, deleted, pointer) capacities (default: the table
    sizes).  With a status only the totals are meaningful."""
    L = _bind()
    e = np.ascontiguousarray(edits, dtype=EDIT_DTYPE)
    f = np.ascontiguousarray(files, dtype=FILE_DTYPE)
    d = np.ascontiguousarray(deleted, dtype=DELETED_DTYPE)
    p = np.ascontiguousarray(pointers, dtype=POINTER_DTYPE)
    bf = np.ascontiguousarray(rec_file, dtype=np.uint64)
    bd = np.ascontiguousarray(rec_deleted, dtype=np.uint64)
    bp = np.ascontiguousarray(rec_pointer, dtype=np.uint64)
    records = e.size if records is None else int(records)
    caps = (f.size, d.size, p.size) if caps is None else tuple(int(c) for c in caps)
    if src is None:
        sbuf, sn = None, int(src_bytes or 0)
    else:
        src = bytes(src)
        sbuf, sn = ctypes.create_string_buffer(src, max(len(src), 1)), (len(src) if src_bytes is None else int(src_bytes))
    rec_off = np.zeros(max(records, 1), dtype=np.uint64)
    rec_len = np.zeros(max(records, 1), dtype=np.uint64)
    tot = EncodeTotals()
    i = EncodeIn()
    i.d_edits = e.ctypes.data if e.size else None
    i.d_files, i.file_cap, i.d_rec_file = (f.ctypes.data if f.size else None), caps[0], bf.ctypes.data
    i.d_deleted, i.deleted_cap, i.d_rec_deleted = (d.ctypes.data if d.size else None), caps[1], bd.ctypes.data
    i.d_pointers, i.pointer_cap, i.d_rec_pointer = (p.ctypes.data if p.size else None), caps[2], bp.ctypes.data

    def call(out, cap):
        o = EncodeOut()
        o.d_out, o.out_cap = out, cap
        o.d_rec_off, o.d_rec_len = rec_off.ctypes.data, rec_len.ctypes.data
        o.d_totals = ctypes.addressof(tot)
        rc = L.lv_version_edit_encode_host(sbuf, sn, ctypes.byref(i), records, ctypes.byref(o))
        if rc != 0:
            raise LvError(f"lv_version_edit_encode_host: {rc}")
        return {n: int(getattr(tot, n)) for n in ENCODE_TOTALS}

    t = call(None, 0)
    out = None
    if not sizing and not t["status"]:
        cap = t["out_bytes"] if out_cap is None else int(out_cap)
        buf = np.zeros(max(cap, 1), dtype=np.uint8)
        t = call(buf.ctypes.data, cap)
        out = b"" if t["status"] else buf[: t["out_bytes"]].tobytes()
    n = 0 if t["status"] else t["records"]
    return out, rec_off[:n].copy(), rec_len[:n].copy(), t


# ---- device -----------------------------------------------------------------------
def decode_workspace_bytes(rec_cap: int) -> int:
    return int(_bind().lv_version_edit_decode_workspace_bytes(rec_cap))


def encode_workspace_bytes(rec_cap: int, file_cap: int, deleted_cap: int, pointer_cap: int) -> int:
    return int(_bind().lv_version_edit_encode_workspace_bytes(rec_cap, file_cap, deleted_cap, pointer_cap))


def _alloc(dev, nbytes, fill, guard):
    import torch
    nbytes = (max(nbytes, 16) + guard + 15) & ~15
    if fill is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)


def _sync(obj, names, status_names, what, check):
    if obj._tot is None:
        import torch
        torch.cuda.synchronize(obj.totals.device)
        obj._tot = dict(zip(names, (int(v) for v in obj.totals.cpu().numpy().view(np.uint64))))
        obj._keep = None
    st = obj._tot["status"]
    if st and check:
        bits = "|".join(n for b, n in status_names.items() if st & b)
        raise LvError(f"{what}: status {bits} (totals {obj._tot})")
    return obj._tot


class Decoded:
    """Outputs of decode_device, CUDA tensors written asynchronously: edits_t,
    files_t, deleted_t, pointers_t (uint8), rec_file / rec_deleted /
    rec_pointer (int64, rec_cap + 1) and totals (int64[12], TOTALS).  The
    tensors and caps feed encode_device as they are."""

    def __init__(self, edits_t, files_t, deleted_t, pointers_t, caps, rec_file, rec_deleted, rec_pointer, totals, keep):
        self.edits_t, self.files_t, self.deleted_t, self.pointers_t, self.caps = edits_t, files_t, deleted_t, pointers_t, caps
        self.rec_file, self.rec_deleted, self.rec_pointer, self.totals = rec_file, rec_deleted, rec_pointer, totals
        self._keep = keep  # the inputs and the workspace, until the work has run
        self._tot = None

    def sync_totals(self, check: bool = True) -> dict:
        """Waits for the call; the totals as a dict (last_has as last_has0..4).
        Raises LvError naming the status bits if one is set unless check is False."""
        return _sync(self, TOTALS, DECODE_STATUS, "lv_version_edit_decode_device", check)

    def _rows(self, t, dtype, n):
        return t[: n * dtype.itemsize].cpu().numpy().view(dtype).copy()

    def edits(self):
        return self._rows(self.edits_t, EDIT_DTYPE, self.sync_totals()["records"])

    def files(self):
        return self._rows(self.files_t, FILE_DTYPE, self.sync_totals()["files"])

    def deleted(self):
        return self._rows(self.deleted_t, DELETED_DTYPE, self.sync_totals()["deleted"])

    def pointers(self):
        return self._rows(self.pointers_t, POINTER_DTYPE, self.sync_totals()["pointers"])

    def bounds(self):
        """(rec_file, rec_deleted, rec_pointer), records + 1 entries each (synchronises)."""
        n = self.sync_totals()["records"]
        return tuple(t[: n + 1].cpu().numpy().view(np.uint64).copy() for t in (self.rec_file, self.rec_deleted, self.rec_pointer))


def decode_device(payload, rec_off, rec_len, records, upstream_status=None, *, rec_cap=None, caps=None, workspace=None,
                  stream=None, fill=None, guard: int = 0, flags: int = 0):
    """lv_version_edit_decode_device.  `payload` is a uint8 CUDA tensor; rec_off
    / rec_len int64 CUDA tensors; `records` and `upstream_status` int64 CUDA
    tensors whose first element is read on the device.  rec_cap defaults to
    rec_off.numel(); caps = (file, deleted, pointer) capacities, by default
    (payload // 6, payload // 3, payload // 3), which suffice when records do
    not overlap.  fill / guard: canaries as in lvgpu.write_batch.  Returns a
    Decoded; asynchronous on `stream`."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind()
    if payload.dtype != torch.uint8:
        raise LvError(f"payload must be a uint8 tensor (got {payload.dtype})")
    dev = payload.device
    for name, t in (("rec_off", rec_off), ("rec_len", rec_len), ("records", records), ("upstream_status", upstream_status)):
        if t is None and name == "upstream_status":
            continue
        if t is None or t.dtype != torch.int64 or t.device != dev:
            raise LvError(f"{name} must be an int64 tensor on the payload's device")
    rec_cap = int(min(rec_off.numel(), rec_len.numel())) if rec_cap is None else int(rec_cap)
    if rec_off.numel() < rec_cap or rec_len.numel() < rec_cap or records.numel() < 1:
        raise LvError("rec_off / rec_len must hold rec_cap entries and records one")
    nb = payload.numel()
    caps = (nb // 6, nb // 3, nb // 3) if caps is None else tuple(int(c) for c in caps)
    if workspace is None:
        workspace = torch.empty(max(L.lv_version_edit_decode_workspace_bytes(rec_cap), 16), dtype=torch.uint8, device=dev)
    edits_t = _alloc(dev, rec_cap * 64, fill, guard)
    files_t = _alloc(dev, caps[0] * 48, fill, guard)
    deleted_t = _alloc(dev, caps[1] * 16, fill, guard)
    pointers_t = _alloc(dev, caps[2] * 16, fill, guard)
    bounds = [_alloc(dev, (rec_cap + 1) * 8, fill, guard).view(torch.int64) for _ in range(3)]
    totals = torch.empty(len(TOTALS), dtype=torch.int64, device=dev)
    o = DecodeOut()
    o.d_edits = _dev_ptr(edits_t, "edits")
    o.d_files, o.file_cap, o.d_rec_file = _dev_ptr(files_t, "files"), caps[0], _dev_ptr(bounds[0], "rec_file")
    o.d_deleted, o.deleted_cap, o.d_rec_deleted = _dev_ptr(deleted_t, "deleted"), caps[1], _dev_ptr(bounds[1], "rec_deleted")
    o.d_pointers, o.pointer_cap, o.d_rec_pointer = _dev_ptr(pointers_t, "pointers"), caps[2], _dev_ptr(bounds[2], "rec_pointer")
    o.d_totals = _dev_ptr(totals, "totals")
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_version_edit_decode_device(_dev_ptr(payload, "payload"), payload.numel(), _dev_ptr(rec_off, "rec_off"),
                                             _dev_ptr(rec_len, "rec_len"), _dev_ptr(records, "records"),
                                             _dev_ptr(upstream_status, "upstream_status"), rec_cap, ctypes.byref(o),
                                             flags, _dev_ptr(workspace, "workspace"), workspace.numel(),
                                             _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_version_edit_decode_device: {lib().lv_last_error().decode()}")
    return Decoded(edits_t, files_t, deleted_t, pointers_t, caps, bounds[0], bounds[1], bounds[2], totals,
                   (payload, rec_off, rec_len, records, upstream_status, workspace))


class Encoded:
    """Outputs of encode_device, CUDA tensors written asynchronously: out_t
    (uint8, out_cap bytes), rec_off_t / rec_len_t (int64, rec_cap) and totals
    (int64[10], ENCODE_TOTALS).  (out_t, rec_off_t, rec_len_t, totals[0:1],
    totals[6:7]) is what decode_device takes."""

    def __init__(self, out_t, out_cap, rec_off, rec_len, totals, keep):
        self.out_t, self.out_cap, self.rec_off_t, self.rec_len_t, self.totals = out_t, out_cap, rec_off, rec_len, totals
        self._keep = keep
        self._tot = None

    def sync_totals(self, check: bool = True) -> dict:
        return _sync(self, ENCODE_TOTALS, ENCODE_STATUS, "lv_version_edit_encode_device", check)

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


def encode_device(src, edits, files, rec_file, deleted, rec_deleted, pointers, rec_pointer, records,
                  upstream_status=None, *, rec_cap=None, caps=None, out_cap=None, out=None, workspace=None, stream=None,
                  fill=None, guard: int = 0, flags: int = 0):
    """lv_version_edit_encode_device.  `src` and the four tables are uint8 CUDA
    tensors (64 / 48 / 16 / 16 bytes per entry, e.g. a Decoded's), the bounds
    int64 CUDA tensors of rec_cap + 1 entries; `records` and `upstream_status`
    int64 CUDA tensors whose first element is read on the device.  rec_cap
    defaults to rec_file.numel() - 1, caps = (file, deleted, pointer) to the
    tables' sizes, out_cap to encode_bound over the capacities with src.numel()
    key bytes -- pass it when extents overlap or repeat.  `out`, a uint8 CUDA
    tensor, is written instead of a fresh allocation.  Returns an Encoded;
    asynchronous on `stream`."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind()
    dev = src.device
    for name, t in (("src", src), ("edits", edits), ("files", files), ("deleted", deleted), ("pointers", pointers)):
        if t.dtype != torch.uint8 or t.device != dev:
            raise LvError(f"{name} must be a uint8 tensor on the source's device")
    for name, t in (("rec_file", rec_file), ("rec_deleted", rec_deleted), ("rec_pointer", rec_pointer),
                    ("records", records), ("upstream_status", upstream_status)):
        if t is None and name == "upstream_status":
            continue
        if t is None or t.dtype != torch.int64 or t.device != dev or t.numel() < 1:
            raise LvError(f"{name} must be an int64 tensor on the source's device")
    rec_cap = rec_file.numel() - 1 if rec_cap is None else int(rec_cap)
    caps = (files.numel() // 48, deleted.numel() // 16, pointers.numel() // 16) if caps is None else tuple(int(c) for c in caps)
    if (min(rec_file.numel(), rec_deleted.numel(), rec_pointer.numel()) < rec_cap + 1 or edits.numel() < rec_cap * 64 or
            files.numel() < caps[0] * 48 or deleted.numel() < caps[1] * 16 or pointers.numel() < caps[2] * 16):
        raise LvError("a table or bounds array is shorter than its capacity")
    if out is not None:
        if out.dtype != torch.uint8 or out.device != dev:
            raise LvError("out must be a uint8 tensor on the source's device")
        out_cap = out.numel() if out_cap is None else int(out_cap)
        if out.numel() < out_cap:
            raise LvError("out must hold out_cap bytes")
    elif out_cap is None:
        out_cap = encode_bound(rec_cap, caps[2], caps[1], caps[0], src.numel())
    out_cap = int(out_cap)
    if workspace is None:
        workspace = torch.empty(max(L.lv_version_edit_encode_workspace_bytes(rec_cap, *caps), 16), dtype=torch.uint8,
                                device=dev)
    out_t = _alloc(dev, out_cap, fill, guard) if out is None else out
    rec_off = _alloc(dev, rec_cap * 8, fill, guard).view(torch.int64)
    rec_len = _alloc(dev, rec_cap * 8, fill, guard).view(torch.int64)
    totals = torch.empty(len(ENCODE_TOTALS), dtype=torch.int64, device=dev)
    i = EncodeIn()
    i.d_edits = _dev_ptr(edits, "edits")
    i.d_files, i.file_cap, i.d_rec_file = _dev_ptr(files, "files"), caps[0], _dev_ptr(rec_file, "rec_file")
    i.d_deleted, i.deleted_cap, i.d_rec_deleted = _dev_ptr(deleted, "deleted"), caps[1], _dev_ptr(rec_deleted, "rec_deleted")
    i.d_pointers, i.pointer_cap, i.d_rec_pointer = _dev_ptr(pointers, "pointers"), caps[2], _dev_ptr(rec_pointer, "rec_pointer")
    o = EncodeOut()
    o.d_out, o.out_cap = _dev_ptr(out_t, "out"), out_cap
    o.d_rec_off, o.d_rec_len = _dev_ptr(rec_off, "rec_off"), _dev_ptr(rec_len, "rec_len")
    o.d_totals = _dev_ptr(totals, "totals")
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_version_edit_encode_device(_dev_ptr(src, "src"), src.numel(), ctypes.byref(i),
                                             _dev_ptr(records, "records"), _dev_ptr(upstream_status, "upstream_status"),
                                             rec_cap, ctypes.byref(o), flags, _dev_ptr(workspace, "workspace"),
                                             workspace.numel(), _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_version_edit_encode_device: {lib().lv_last_error().decode()}")
    return Encoded(out_t, out_cap, rec_off, rec_len, totals,
                   (src, edits, files, rec_file, deleted, rec_deleted, pointers, rec_pointer, records, upstream_status,
                    workspace))


def files_device(version_files, tables, file_count, *, files_cap=None, stream=None):
    """lv_version_edit_files_device over lvgpu.compact's output: version_files
    and tables are uint8 CUDA tensors (64 bytes per record each), file_count an
    int64 CUDA tensor whose first element is read on the device.  Returns
    (files_t uint8 of 48-byte rows, rec_file int64[2], status int64[1]), written
    asynchronously on `stream`."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind()
    dev = version_files.device
    files_cap = min(version_files.numel(), tables.numel()) // 64 if files_cap is None else int(files_cap)
    files_t = torch.empty(max(files_cap * 48, 16), dtype=torch.uint8, device=dev)
    rec_file = torch.empty(2, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = L.lv_version_edit_files_device(_dev_ptr(version_files, "version_files"), _dev_ptr(tables, "tables"),
                                            _dev_ptr(file_count, "file_count"), files_cap, _dev_ptr(files_t, "files"),
                                            _dev_ptr(rec_file, "rec_file"), _dev_ptr(status, "status"),
                                            _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_version_edit_files_device: {lib().lv_last_error().decode()}")
    return files_t, rec_file, status
