"""Python binding of include/lvgpu/version.h: Version::Get over the tables of a
version (several overlapping level-0 tables, sorted runs on levels 1-6).

    HostVersion(images, files, tables, blooms, bounds)
                                      the host twins over host arrays: .open()
                                      is lv_version_open_host's dict, .get(key,
                                      seq) lv_version_get_host's
    file_host(images, file_off, file_cap, table, number, level, bounds, used)
                                      lv_version_file_host: (file dict, cursor)
    file_device(...)                  lv_version_file_device, asynchronous
    open_device(images_t, files_t, tables_t, n_files, bounds_t, ...)
                                      lv_version_open_device: an Opened (what a
                                      get needs, and the lv_version_state in
                                      HBM), asynchronous until .sync()
    get_device(opened, qkeys, q_off, q_len, q_seq)
                                      lv_version_get_device: a Gets,
                                      asynchronous until .sync()
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import LvError, _dev_ptr, _stream_ptr, _torch, lib
from .table import BLOOM_FIELDS, TABLE_FIELDS

NUM_LEVELS = 7                # LV_NUM_LEVELS
MAX_FILES = 1 << 20           # LV_VERSION_MAX_FILES
FILE_STATUS = {1: "NO_TABLE", 2: "BAD_EXTENT", 3: "EMPTY", 4: "CORRUPT", 5: "BOUND_OVER",
               6: "UNPLACED"}  # LV_VERSION_FILE_*; UNPLACED is lv_version_apply_device's (lvgpu.version_set)
FILE_NO_TABLE, FILE_BAD_EXTENT, FILE_EMPTY, FILE_CORRUPT, FILE_BOUND_OVER, FILE_UNPLACED = FILE_STATUS
OPEN_STATUS = {1: "UPSTREAM", 2: "BAD_FILE", 4: "BAD_TABLE", 8: "BAD_BOUND", 16: "UNSORTED"}  # LV_VERSION_OPEN_*
OPEN_UPSTREAM, OPEN_BAD_FILE, OPEN_BAD_TABLE, OPEN_BAD_BOUND, OPEN_UNSORTED = OPEN_STATUS
FILE_DTYPE = np.dtype([("number", "<u8"), ("file_off", "<u8"), ("file_cap", "<u8"), ("smallest_off", "<u8"),
                       ("largest_off", "<u8"), ("smallest_len", "<u4"), ("largest_len", "<u4"), ("level", "<u4"),
                       ("status", "<u4"), ("reserved", "<u8")])  # lv_version_file
GET_DTYPE = np.dtype([("val_off", "<u8"), ("tag", "<u8"), ("val_len", "<u4"), ("block", "<u4"), ("status", "<u4"),
                      ("file", "<u4"), ("level", "<u4"), ("files_read", "<u4"), ("seek_file", "<u4"),
                      ("filtered", "<u4")])  # lv_version_get_result
assert FILE_DTYPE.itemsize == 64 and GET_DTYPE.itemsize == 48
VERSION_WORDS = 3 + NUM_LEVELS + 1  # lv_version_state: files, level_start[8], first_bad, status
_bound = False


def _bind():
    global _bound
    L = lib()
    if not _bound:
        vp, sz, u64, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32
        L.lv_version_file_device.restype = ctypes.c_int
        L.lv_version_file_device.argtypes = [vp, u64, u64, u64, vp, u64, u32, vp, u64, vp, vp, u32, vp]
        L.lv_version_open_device.restype = ctypes.c_int
        L.lv_version_open_device.argtypes = [u64, vp, vp, sz, vp, u64, vp, vp, u32, vp]
        L.lv_version_get_device.restype = ctypes.c_int
        L.lv_version_get_device.argtypes = [vp, u64, vp, vp, vp, sz, vp, u64, vp, vp, sz, vp, vp, vp, sz, vp, u32, vp]
        L.lv_version_file_host.restype = ctypes.c_int
        L.lv_version_file_host.argtypes = [vp, u64, u64, u64, vp, u64, u32, vp, u64, vp, vp]
        L.lv_version_open_host.restype = ctypes.c_int
        L.lv_version_open_host.argtypes = [u64, vp, vp, sz, vp, u64, vp]
        L.lv_version_get_host.restype = ctypes.c_int
        L.lv_version_get_host.argtypes = [vp, u64, vp, vp, vp, sz, vp, u64, vp, vp, sz, u64, vp]
        _bound = True
    return L


def version_dict(words) -> dict:
    """The 11 words of an lv_version_state as a dict."""
    w = [int(x) for x in words]
    return dict(files=w[0], level_start=w[1:2 + NUM_LEVELS], first_bad=w[2 + NUM_LEVELS], status=w[3 + NUM_LEVELS])


def version_words(v) -> np.ndarray:
    return np.array([v["files"], *v["level_start"], v["first_bad"], v["status"]], dtype=np.uint64)


def tables_array(tables) -> np.ndarray:
    """Table dicts (lvgpu.table.TABLE_FIELDS) as the uint64 [n, 8] array of lv_sst_table."""
    return np.array([[int(t[f]) for f in TABLE_FIELDS] for t in tables], dtype=np.uint64).reshape(-1, 8)


def blooms_array(blooms) -> np.ndarray:
    return np.array([[int(b[f]) for f in BLOOM_FIELDS] for b in blooms], dtype=np.uint64).reshape(-1, 8)


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def file_host(images, file_off, file_cap, table, number, level, bounds, used, *, bound_cap=None, images_bytes=None):
    """lv_version_file_host.  images: a uint8 array; table: a table dict;
    bounds: a writable uint8 array (the boundary keys go in behind `used`).
    Returns (the lv_version_file as a dict, the new cursor)."""
    L = _bind()
    t = np.array([int(table[f]) for f in TABLE_FIELDS], dtype=np.uint64)
    out = np.zeros(1, dtype=FILE_DTYPE)
    cur = ctypes.c_uint64(used)
    rc = L.lv_version_file_host(_ptr(images), len(images) if images_bytes is None else images_bytes, file_off, file_cap,
                                t.ctypes.data, number, level, _ptr(bounds), len(bounds) if bound_cap is None else bound_cap,
                                ctypes.byref(cur), out.ctypes.data)
    if rc != 0:
        raise LvError(f"lv_version_file_host: {rc}")
    return {n: int(out[0][n]) for n in FILE_DTYPE.names}, int(cur.value)


class HostVersion:
    """The arrays of a version in host memory, for the host twins.  images and
    bounds are bytes or uint8 arrays (copied into exact-size arrays), files a
    FILE_DTYPE array, tables / blooms uint64 [n, 8] arrays (blooms may be
    None)."""

    def __init__(self, images, files, tables, blooms, bounds, *, images_bytes=None, bounds_bytes=None):
        self.images = np.frombuffer(bytes(images), dtype=np.uint8).copy() if not isinstance(images, np.ndarray) else images
        self.bounds = np.frombuffer(bytes(bounds), dtype=np.uint8).copy() if not isinstance(bounds, np.ndarray) else bounds
        self.files = np.ascontiguousarray(files, dtype=FILE_DTYPE)
        self.tables = np.ascontiguousarray(tables, dtype=np.uint64).reshape(-1, 8)
        self.blooms = None if blooms is None else np.ascontiguousarray(blooms, dtype=np.uint64).reshape(-1, 8)
        self.n = len(self.files)
        self.images_bytes = len(self.images) if images_bytes is None else images_bytes
        self.bounds_bytes = len(self.bounds) if bounds_bytes is None else bounds_bytes
        self.version = None  # the words of the open

    def open(self) -> dict:
        L = _bind()
        w = np.zeros(VERSION_WORDS, dtype=np.uint64)
        rc = L.lv_version_open_host(self.images_bytes, _ptr(self.files), _ptr(self.tables), self.n, _ptr(self.bounds),
                                    self.bounds_bytes, w.ctypes.data)
        if rc != 0:
            raise LvError(f"lv_version_open_host: {rc}")
        self.version = w
        return version_dict(w)

    def get(self, key, seq, version=None) -> dict:
        """lv_version_get_host for one query, by the open's version or the
        given dict."""
        L = _bind()
        if version is not None:
            w = version_words(version)
        else:
            if self.version is None:
                self.open()
            w = self.version
        kb = bytes(key)
        r = np.zeros(1, dtype=GET_DTYPE)
        rc = L.lv_version_get_host(_ptr(self.images), self.images_bytes, _ptr(self.files), _ptr(self.tables),
                                   _ptr(self.blooms), self.n, _ptr(self.bounds), self.bounds_bytes, w.ctypes.data, kb,
                                   len(kb), seq, r.ctypes.data)
        if rc != 0:
            raise LvError(f"lv_version_get_host: {rc}")
        return {n: int(r[0][n]) for n in GET_DTYPE.names}


# ---- the device ----
def file_device(images_t, images_bytes, file_off, file_cap, table_t, number, level, bounds_t, bound_cap, used_t, out_t,
                *, stream=None, flags: int = 0):
    """lv_version_file_device.  table_t: the int64[8] lv_sst_table tensor of
    lvgpu.table.open_device; used_t: an int64[1] cursor; out_t: a uint8 tensor
    (or slice) of 64 bytes.  Asynchronous on `stream`."""
    torch = _torch()
    L = _bind()
    with torch.cuda.device(images_t.device):
        rc = L.lv_version_file_device(_dev_ptr(images_t, "images") if images_bytes else None, images_bytes, file_off,
                                      file_cap, _dev_ptr(table_t, "table"), number, level,
                                      _dev_ptr(bounds_t, "bound_keys") if bound_cap else None, bound_cap,
                                      _dev_ptr(used_t, "bound_used"), _dev_ptr(out_t, "out"), flags, _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_version_file_device: {lib().lv_last_error().decode()}")
    return out_t


class Opened:
    """Outputs of open_device and what a get needs: images_t (uint8), files_t
    (uint8, 64 bytes per lv_version_file), tables_t (int64, 8 per file),
    blooms_t (int64, 8 per file, or None), bounds_t (uint8) and version
    (int64[11], the lv_version_state, written asynchronously)."""

    def __init__(self, images_t, images_bytes, files_t, tables_t, blooms_t, n_files, bounds_t, bounds_bytes, version,
                 keep=None):
        self.images_t, self.images_bytes, self.files_t, self.tables_t, self.blooms_t = images_t, images_bytes, files_t, tables_t, blooms_t
        self.n_files, self.bounds_t, self.bounds_bytes, self.version = n_files, bounds_t, bounds_bytes, version
        self._keep = keep

    def sync(self, check: bool = True) -> dict:
        """Waits for the call; the lv_version_state as a dict.  Raises LvError
        naming the status bits if one is set unless check is False."""
        _torch().cuda.synchronize(self.version.device)
        v = version_dict(self.version.cpu().numpy().view(np.uint64))
        if v["status"] and check:
            names = "|".join(n for b, n in OPEN_STATUS.items() if v["status"] & b)
            raise LvError(f"lv_version_open_device: status {names} (version {v})")
        return v

    def files(self) -> np.ndarray:
        """d_files as a FILE_DTYPE array (synchronises)."""
        _torch().cuda.synchronize(self.files_t.device)
        return self.files_t[: 64 * self.n_files].cpu().numpy().view(FILE_DTYPE).copy()


def open_device(images_t, files_t, tables_t, n_files, bounds_t, *, blooms_t=None, images_bytes=None, bounds_bytes=None,
                upstream_status=None, version=None, stream=None, flags: int = 0):
    """lv_version_open_device.  blooms_t is only carried along for the gets.
    version reuses an earlier call's tensor (graph replays).  Returns an
    Opened; asynchronous on `stream`."""
    torch = _torch()
    L = _bind()
    dev = images_t.device
    images_bytes = images_t.numel() if images_bytes is None else int(images_bytes)
    bounds_bytes = bounds_t.numel() if bounds_bytes is None else int(bounds_bytes)
    if version is None:
        version = torch.empty(VERSION_WORDS, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = L.lv_version_open_device(images_bytes, _dev_ptr(files_t, "files") if n_files else None,
                                      _dev_ptr(tables_t, "tables") if n_files else None, n_files,
                                      _dev_ptr(bounds_t, "bound_keys") if bounds_bytes else None, bounds_bytes,
                                      _dev_ptr(upstream_status, "upstream_status"), _dev_ptr(version, "version"), flags,
                                      _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_version_open_device: {lib().lv_last_error().decode()}")
    return Opened(images_t, images_bytes, files_t, tables_t, blooms_t, n_files, bounds_t, bounds_bytes, version,
                  (upstream_status,))


class Gets:
    """Output of get_device: res, a uint8 CUDA tensor of nq
    lv_version_get_result (and the guard), written asynchronously."""

    def __init__(self, res, nq, keep):
        self.res, self.nq = res, nq
        self._keep = keep
        self._out = None

    def sync(self):
        """Waits for the call; the results as a structured array (GET_DTYPE)."""
        if self._out is None:
            _torch().cuda.synchronize(self.res.device)
            self._out = self.res[: self.nq * 48].cpu().numpy().view(GET_DTYPE).copy()
            self._keep = None
        return self._out


def get_device(opened, qkeys, q_off, q_len, q_seq, *, nq=None, res=None, bloom=True, stream=None, fill=None,
               guard: int = 0, flags: int = 0):
    """lv_version_get_device over an Opened.  qkeys is a uint8 CUDA tensor,
    q_off / q_seq int64 and q_len int32 CUDA tensors of nq entries.  bloom=False
    passes a NULL d_blooms.  res reuses an earlier call's tensor.  Returns a
    Gets; asynchronous on `stream`."""
    torch = _torch()
    L = _bind()
    o = opened
    dev = o.images_t.device
    if qkeys.dtype != torch.uint8 or q_off.dtype != torch.int64 or q_seq.dtype != torch.int64 or \
            q_len.dtype != torch.int32:
        raise LvError("qkeys must be uint8, q_off and q_seq int64, q_len int32")
    nq = int(min(q_off.numel(), q_len.numel(), q_seq.numel())) if nq is None else int(nq)
    if min(q_off.numel(), q_len.numel(), q_seq.numel()) < nq:
        raise LvError("the query arrays must hold nq entries")
    if res is None:
        nbytes = (max(nq * 48, 16) + guard + 7) & ~7
        res = (torch.empty(nbytes, dtype=torch.uint8, device=dev) if fill is None
               else torch.full((nbytes,), fill, dtype=torch.uint8, device=dev))
    blooms_t = o.blooms_t if bloom else None
    with torch.cuda.device(dev):
        rc = L.lv_version_get_device(_dev_ptr(o.images_t, "images") if o.images_bytes else None, o.images_bytes,
                                     _dev_ptr(o.files_t, "files") if o.n_files else None,
                                     _dev_ptr(o.tables_t, "tables") if o.n_files else None,
                                     _dev_ptr(blooms_t, "blooms") if o.n_files else None, o.n_files,
                                     _dev_ptr(o.bounds_t, "bound_keys") if o.bounds_bytes else None, o.bounds_bytes,
                                     _dev_ptr(o.version, "version"),
                                     _dev_ptr(qkeys, "qkeys") if qkeys.numel() else None, qkeys.numel(),
                                     _dev_ptr(q_off, "q_off"), _dev_ptr(q_len, "q_len"), _dev_ptr(q_seq, "q_seq"), nq,
                                     _dev_ptr(res, "results"), flags, _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_version_get_device: {lib().lv_last_error().decode()}")
    return Gets(res, nq, (opened, qkeys, q_off, q_len, q_seq))
