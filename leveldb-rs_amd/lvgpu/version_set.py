"""Python mirror of include/lvgpu/version_set.h: the edits of a MANIFEST applied
to a version (upstream's VersionSet::Builder and Recover's bookkeeping).

    apply_host(src, edits, files, rec_file, deleted, rec_deleted, pointers, rec_pointer,
               directory)             lv_version_apply_host: (lv_version_file rows,
                                      dir_index, totals dict)
    apply_device(src, edits, files, rec_file, deleted, rec_deleted, pointers, rec_pointer,
                 records, upstream_status, directory=...)
                                      lv_version_apply_device: an Applied with lazy
                                      .sync_totals() / .files() / .dir_index()

The tables are lvgpu.version_edit's (EDIT_DTYPE, FILE_DTYPE, ...), the rows
lvgpu.version's FILE_DTYPE, so a Decoded feeds in and lvgpu.version.open_device
takes what comes out, with `src` as its bound keys.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import LvError, lib
from .version import FILE_DTYPE as VERSION_FILE_DTYPE
from .version import FILE_UNPLACED, MAX_FILES, NUM_LEVELS  # FILE_UNPLACED: LV_VERSION_FILE_UNPLACED
from .version_edit import (DELETED_DTYPE, EDIT_DTYPE, FILE_DTYPE, KIND_DELETED, KIND_FILE, KIND_POINTER, POINTER_DTYPE,
                           EncodeIn, _alloc)

UPSTREAM, REC_OVER, BAD_BOUNDS, BAD_ROW, DUPLICATE, BAD_DIRECTORY, FILE_OVER = 1, 2, 4, 8, 16, 32, 64  # LV_VS_*
STATUS = {1: "UPSTREAM", 2: "REC_OVER", 4: "BAD_BOUNDS", 8: "BAD_ROW", 16: "DUPLICATE", 32: "BAD_DIRECTORY",
          64: "FILE_OVER"}
KIND_DIRECTORY = 4              # LV_VS_KIND_DIRECTORY
MAX_NUMBER = 1 << 56            # LV_VS_MAX_NUMBER
NO_DIR_INDEX = 0xFFFFFFFF       # LV_VS_NO_DIR_INDEX
MAX_REC_CAP = (1 << 32) - 2
MAX_ROWS = 1 << 30
NONE = (1 << 64) - 1            # bad_kind / bad_row when no bit sets them
# csrc/version_set.hip: kVsTile (NewFile rows per scan tile, live files per sort
# tile), kVsThreads (items per workgroup), kVsPrefix (user-key bytes in a sort
# entry).  The GPU tests choose their shapes around them.
VS_TILE = 1024
VS_THREADS = 256
VS_PREFIX = 16

PLACEMENT_DTYPE = np.dtype([("number", "<u8"), ("file_off", "<u8"), ("file_cap", "<u8"), ("reserved", "<u8")])
_SCALARS = ("records", "new_files", "deleted", "pointers", "live", "unplaced")
_ARRAYS = ("level_files", "level_bytes", "compact_pointer")
_TAIL = ("log_number", "prev_log_number", "next_file_number", "last_sequence", "comparator_off", "comparator_len", "has",
         "max_file_number", "status", "bad_kind", "bad_row")
TOTALS_WORDS = len(_SCALARS) + NUM_LEVELS * len(_ARRAYS) + len(_TAIL)  # lv_vs_totals as u64 words
assert PLACEMENT_DTYPE.itemsize == 32 and TOTALS_WORDS == 38


def totals_dict(words) -> dict:
    """The 38 words of an lv_vs_totals: scalars as ints, the per-level arrays as lists."""
    w = [int(x) for x in words]
    t = dict(zip(_SCALARS, w))
    at = len(_SCALARS)
    for name in _ARRAYS:
        t[name] = w[at: at + NUM_LEVELS]
        at += NUM_LEVELS
    t.update(zip(_TAIL, w[at:]))
    return t


class ApplyOut(ctypes.Structure):
    """lv_vs_out."""
    _fields_ = [("d_files_out", ctypes.c_void_p), ("files_cap", ctypes.c_size_t), ("d_dir_index", ctypes.c_void_p),
                ("d_totals", ctypes.c_void_p)]


_bound = False


def _bind():
    global _bound
    L = lib()
    if _bound:
        return L
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.lv_version_apply_workspace_bytes.restype = sz
    L.lv_version_apply_workspace_bytes.argtypes = [sz, sz, sz]
    L.lv_version_apply_device.restype = ctypes.c_int
    L.lv_version_apply_device.argtypes = [vp, sz, ctypes.POINTER(EncodeIn), vp, vp, sz, vp, sz, ctypes.POINTER(ApplyOut),
                                          ctypes.c_uint32, vp, sz, vp]
    L.lv_version_apply_host.restype = ctypes.c_int
    L.lv_version_apply_host.argtypes = [vp, sz, ctypes.POINTER(EncodeIn), sz, vp, sz, ctypes.POINTER(ApplyOut)]
    _bound = True
    return L


def placements(rows) -> np.ndarray:
    """[(number, file_off, file_cap)] or {number: (file_off, file_cap)} as a
    PLACEMENT_DTYPE array; a dict comes out ascending by number."""
    if isinstance(rows, dict):
        rows = [(n,) + tuple(rows[n]) for n in sorted(rows)]
    a = np.zeros(len(rows), dtype=PLACEMENT_DTYPE)
    for r, (number, off, cap) in zip(a, rows):
        r["number"], r["file_off"], r["file_cap"] = number, off, cap
    return a


# ---- the host twin ----------------------------------------------------------------
def apply_host(src, edits, files, rec_file, deleted, rec_deleted, pointers, rec_pointer, directory=None, *,
               records=None, caps=None, files_cap=None, src_bytes=None, dir_n=None, dir_index=True):
    """lv_version_apply_host: (rows, dir_index, totals dict).  The tables are
    structured arrays (lvgpu.version_edit's dtypes), the bounds records + 1
    entries each, `directory` a PLACEMENT_DTYPE array or None.  files_cap
    defaults to the NewFile rows (which always suffice); caps = (file,
    deleted, pointer) capacities (default: the table sizes).  rows is a
    lvgpu.version.FILE_DTYPE array of `live` entries and dir_index uint32 (None
    with dir_index=False) -- both empty when a status is set."""
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
    src = bytes(src)
    sbuf, sn = ctypes.create_string_buffer(src, max(len(src), 1)), (len(src) if src_bytes is None else int(src_bytes))
    pl = None if directory is None else np.ascontiguousarray(directory, dtype=PLACEMENT_DTYPE)
    n_dir = (0 if pl is None else pl.size) if dir_n is None else int(dir_n)
    files_cap = min(f.size, MAX_FILES) if files_cap is None else int(files_cap)
    rows = np.zeros(max(files_cap, 1), dtype=VERSION_FILE_DTYPE)
    idx = np.zeros(max(files_cap, 1), dtype=np.uint32)
    tot = np.zeros(TOTALS_WORDS, dtype=np.uint64)
    i = EncodeIn()
    i.d_edits = e.ctypes.data if e.size else None
    i.d_files, i.file_cap, i.d_rec_file = (f.ctypes.data if f.size else None), caps[0], bf.ctypes.data
    i.d_deleted, i.deleted_cap, i.d_rec_deleted = (d.ctypes.data if d.size else None), caps[1], bd.ctypes.data
    i.d_pointers, i.pointer_cap, i.d_rec_pointer = (p.ctypes.data if p.size else None), caps[2], bp.ctypes.data
    o = ApplyOut()
    o.d_files_out, o.files_cap = (rows.ctypes.data if files_cap else None), files_cap
    o.d_dir_index = idx.ctypes.data if dir_index else None
    o.d_totals = tot.ctypes.data
    rc = L.lv_version_apply_host(sbuf, sn, ctypes.byref(i), records, pl.ctypes.data if n_dir else None, n_dir,
                                 ctypes.byref(o))
    if rc != 0:
        raise LvError(f"lv_version_apply_host: {rc}")
    t = totals_dict(tot)
    n = 0 if t["status"] else t["live"]
    return rows[:n].copy(), (idx[:n].copy() if dir_index else None), t


# ---- the device -------------------------------------------------------------------
def workspace_bytes(file_cap: int, deleted_cap: int, files_cap: int) -> int:
    return int(_bind().lv_version_apply_workspace_bytes(file_cap, deleted_cap, files_cap))


class Applied:
    """Outputs of apply_device, CUDA tensors written asynchronously: files_t
    (uint8, files_cap rows of 64 bytes: what lvgpu.version.open_device takes),
    dir_index_t (int32 bit patterns of the uint32 indices, or None) and totals
    (int64[38]; totals[4:5] is `live`, totals[35:36] the status)."""

    def __init__(self, files_t, files_cap, dir_index_t, totals, keep):
        self.files_t, self.files_cap, self.dir_index_t, self.totals = files_t, files_cap, dir_index_t, totals
        self._keep = keep  # the inputs and the workspace, until the work has run
        self._tot = None

    def sync_totals(self, check: bool = True) -> dict:
        """Waits for the call; the totals as a dict.  Raises LvError naming the
        status bits if one is set unless check is False."""
        if self._tot is None:
            import torch
            torch.cuda.synchronize(self.totals.device)
            self._tot = totals_dict(self.totals.cpu().numpy().view(np.uint64))
            self._keep = None
        st = self._tot["status"]
        if st and check:
            bits = "|".join(n for b, n in STATUS.items() if st & b)
            raise LvError(f"lv_version_apply_device: status {bits} (totals {self._tot})")
        return self._tot

    def _live(self):
        t = self.sync_totals(check=False)
        return 0 if t["status"] else t["live"]

    def files(self) -> np.ndarray:
        return self.files_t[: self._live() * 64].cpu().numpy().view(VERSION_FILE_DTYPE).copy()

    def dir_index(self) -> np.ndarray:
        return self.dir_index_t[: self._live()].cpu().numpy().view(np.uint32).copy()


def apply_device(src, edits, files, rec_file, deleted, rec_deleted, pointers, rec_pointer, records,
                 upstream_status=None, *, directory=None, dir_n=None, rec_cap=None, caps=None, files_cap=None,
                 dir_index=True, workspace=None, stream=None, fill=None, guard: int = 0, flags: int = 0):
    """lv_version_apply_device.  `src` and the four tables are uint8 CUDA
    tensors (64 / 48 / 16 / 16 bytes per entry, e.g. a Decoded's), the bounds
    int64 CUDA tensors of rec_cap + 1 entries; `records` and `upstream_status`
    int64 CUDA tensors whose first element is read on the device; `directory`
    a uint8 CUDA tensor of 32-byte lv_vs_placement entries or None.  rec_cap
    defaults to rec_file.numel() - 1, caps = (file, deleted, pointer) to the
    tables' sizes, files_cap to min(file cap, 2^20).  fill / guard: canaries as
    in lvgpu.write_batch.  Returns an Applied; asynchronous on `stream`."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind()
    dev = src.device
    for name, t in (("src", src), ("edits", edits), ("files", files), ("deleted", deleted), ("pointers", pointers),
                    ("directory", directory)):
        if t is None and name == "directory":
            continue
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
    n_dir = (0 if directory is None else directory.numel() // 32) if dir_n is None else int(dir_n)
    if n_dir and (directory is None or directory.numel() < n_dir * 32):
        raise LvError("directory must hold dir_n entries of 32 bytes")
    files_cap = min(caps[0], MAX_FILES) if files_cap is None else int(files_cap)
    if workspace is None:
        workspace = torch.empty(max(L.lv_version_apply_workspace_bytes(caps[0], caps[1], files_cap), 16), dtype=torch.uint8,
                                device=dev)
    files_t = _alloc(dev, files_cap * 64, fill, guard)
    index_t = _alloc(dev, files_cap * 4, fill, guard).view(torch.int32) if dir_index else None
    totals = torch.empty(TOTALS_WORDS, dtype=torch.int64, device=dev)
    i = EncodeIn()
    i.d_edits = _dev_ptr(edits, "edits")
    i.d_files, i.file_cap, i.d_rec_file = _dev_ptr(files, "files"), caps[0], _dev_ptr(rec_file, "rec_file")
    i.d_deleted, i.deleted_cap, i.d_rec_deleted = _dev_ptr(deleted, "deleted"), caps[1], _dev_ptr(rec_deleted, "rec_deleted")
    i.d_pointers, i.pointer_cap, i.d_rec_pointer = _dev_ptr(pointers, "pointers"), caps[2], _dev_ptr(rec_pointer, "rec_pointer")
    o = ApplyOut()
    o.d_files_out, o.files_cap = _dev_ptr(files_t, "files_out"), files_cap
    o.d_dir_index = _dev_ptr(index_t, "dir_index")
    o.d_totals = _dev_ptr(totals, "totals")
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_version_apply_device(_dev_ptr(src, "src"), src.numel(), ctypes.byref(i), _dev_ptr(records, "records"),
                                       _dev_ptr(upstream_status, "upstream_status"), rec_cap,
                                       _dev_ptr(directory, "directory") if n_dir else None, n_dir, ctypes.byref(o), flags,
                                       _dev_ptr(workspace, "workspace"), workspace.numel(), _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_version_apply_device: {lib().lv_last_error().decode()}")
    return Applied(files_t, files_cap, index_t, totals,
                   (src, edits, files, rec_file, deleted, rec_deleted, pointers, rec_pointer, records, upstream_status,
                    directory, workspace))
