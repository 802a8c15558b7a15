"""Python mirror of src/table/format.rs (BlockHandle, Footer), the GPU
block-trailer seal/verify and the SSTable build over include/lvgpu/table.h.

    build_host(payload, ops, order, mt_totals, block_size, restart_interval)
                                      lv_sst_build_host: (file, handles, totals)
    build_workspace_bytes(op_cap, block_cap)
                                      device workspace of build_device
    file_bound(payload_bytes, op_cap) lv_sst_build_file_bound
    build_device(table)               lv_sst_build_device over a
                                      lvgpu.memtable.Table; no host sync until
                                      .sync_totals() / .file() / .handles()
    open_host(file)                   lv_sst_open_host: (table dict, handles)
    get_host(file, table, key, seq)   lv_sst_get_host: a result dict
    open_device(file_t, file_bytes)   lv_sst_open_device: an Opened (the table and
                                      the handles in HBM), asynchronous
    get_device(opened, qkeys, q_off, q_len, q_seq)
                                      lv_sst_get_device: a Gets, asynchronous until
                                      .sync()
    scan_host(file, table, prev)      lv_sst_scan_host: (totals dict, ops, arena,
                                      memtable totals)
    scan_workspace_bytes(op_cap, block_cap)
                                      device workspace of scan_device
    scan_device(opened, prev)         lv_sst_scan_device: a Scanned (ops, arena,
                                      totals; .memtable() is what build_device and
                                      lvgpu.memtable.get_device take), asynchronous
                                      until .sync()
    bloom_hash / bloom_filter_bytes / bloom_create_filter / bloom_key_may_match
                                      the lv_bloom_* host scalars
    build_bloom_host(...) / build_bloom_device(table, bits_per_key)
                                      lv_sst_build_bloom_*: the build with a filter
                                      block; a BuiltBloom (data_blocks + 3 handles,
                                      .sync_bloom_totals())
    bloom_open_host(file, table) / bloom_open_device(opened)
                                      lv_sst_bloom_open_*: the lv_sst_bloom as a dict /
                                      as an int64[8] CUDA tensor (bloom_dict reads it)
    get_bloom_host(...) / get_bloom_device(opened, bloom, qkeys, ...)
                                      lv_sst_get_bloom_*: the get that asks the filter
                                      first; reserved == GET_FILTERED where it said no
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import LvError, _check, _dev_ptr, _stream_ptr, _torch, lib
from .memtable import Totals as MtTotals  # lv_mt_totals

MAGIC = 0xDB4775248B80FB57
BLOCK_HANDLE_MAX_ENCODED_LENGTH = 20
FOOTER_ENCODED_LENGTH = 48
TRAILER_SIZE = 5
BLOCK_OK, BLOCK_CHECKSUM_MISMATCH, BLOCK_OUT_OF_RANGE = 0, 1, 2
ERR_CORRUPTION = -3
_bound = False


class Corruption(LvError):
    """ErrorType::Corruption from the format decoders."""


def _bind():
    global _bound
    L = lib()
    if not _bound:
        vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
        L.lv_sst_block_handle_encode.restype = sz
        L.lv_sst_block_handle_encode.argtypes = [u64, u64, ctypes.c_char_p]
        L.lv_sst_block_handle_decode.restype = ctypes.c_int
        L.lv_sst_block_handle_decode.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                                 ctypes.POINTER(sz)]
        L.lv_sst_footer_encode.restype = None
        L.lv_sst_footer_encode.argtypes = [u64, u64, u64, u64, ctypes.c_char_p]
        L.lv_sst_footer_decode.restype = ctypes.c_int
        L.lv_sst_footer_decode.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(u64 * 4)]
        L.lv_sst_seal_blocks_device.restype = ctypes.c_int
        L.lv_sst_seal_blocks_device.argtypes = [vp, u64, vp, vp, sz, vp]
        L.lv_sst_verify_blocks_device.restype = ctypes.c_int
        L.lv_sst_verify_blocks_device.argtypes = [vp, u64, vp, sz, vp, vp, vp]
        L.lv_sst_verify_blocks_host.restype = ctypes.c_int
        L.lv_sst_verify_blocks_host.argtypes = [vp, u64, vp, sz, vp, ctypes.c_int]
        _bound = True
    return L


def _decode_check(rc, L):
    if rc == ERR_CORRUPTION:
        raise Corruption(L.lv_last_error().decode())
    _check(rc)


class BlockHandle:  # format.rs:26-50
    def __init__(self, offset: int, size: int):
        self.offset, self.size = offset, size

    def __eq__(self, o):
        return (self.offset, self.size) == (o.offset, o.size)

    def __repr__(self):
        return f"BlockHandle(offset={self.offset}, size={self.size})"

    def encode_to(self, dst: bytearray) -> None:
        buf = ctypes.create_string_buffer(BLOCK_HANDLE_MAX_ENCODED_LENGTH)
        n = _bind().lv_sst_block_handle_encode(self.offset, self.size, buf)
        dst += buf.raw[:n]

    @staticmethod
    def decode_from(src: bytes):
        """-> (BlockHandle, bytes consumed); Corruption("bad handle")."""
        L = _bind()
        o, s, n = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_size_t()
        b = bytes(src)
        _decode_check(L.lv_sst_block_handle_decode(b, len(b), ctypes.byref(o), ctypes.byref(s), ctypes.byref(n)), L)
        return BlockHandle(o.value, s.value), n.value


class Footer:  # format.rs:52-104
    def __init__(self, metaindex_handle: BlockHandle, index_handle: BlockHandle):
        self.metaindex_handle, self.index_handle = metaindex_handle, index_handle

    def __eq__(self, o):
        return (self.metaindex_handle, self.index_handle) == (o.metaindex_handle, o.index_handle)

    def encode(self) -> bytes:
        out = ctypes.create_string_buffer(FOOTER_ENCODED_LENGTH)
        m, i = self.metaindex_handle, self.index_handle
        _bind().lv_sst_footer_encode(m.offset, m.size, i.offset, i.size, out)
        return out.raw

    @staticmethod
    def decode_from(src: bytes) -> "Footer":
        L = _bind()
        h = (ctypes.c_uint64 * 4)()
        b = bytes(src)
        _decode_check(L.lv_sst_footer_decode(b, len(b), ctypes.byref(h)), L)
        return Footer(BlockHandle(h[0], h[1]), BlockHandle(h[2], h[3]))


def seal_blocks(file, handles, types=None, stream=None):
    """Write type + masked crc trailers after every handle's extent, in place.
    file: uint8 CUDA tensor; handles: int64 CUDA tensor of shape (n, 2)."""
    L = _bind()
    n = handles.numel() // 2
    _check(L.lv_sst_seal_blocks_device(_dev_ptr(file, "file"), file.numel(), _dev_ptr(handles, "handles"),
                                       _dev_ptr(types, "types"), n, _stream_ptr(stream)))
    return file


def verify_blocks(file, handles, out_crc=False, stream=None):
    """Per-block status (BLOCK_OK / BLOCK_CHECKSUM_MISMATCH / BLOCK_OUT_OF_RANGE)
    as an int32 CUDA tensor; with out_crc also crc32c(contents||type)."""
    torch = _torch()
    L = _bind()
    n = handles.numel() // 2
    st = torch.empty(n, dtype=torch.int32, device=file.device)
    crc = torch.empty(n, dtype=torch.int32, device=file.device) if out_crc else None
    _check(L.lv_sst_verify_blocks_device(_dev_ptr(file, "file"), file.numel(), _dev_ptr(handles, "handles"), n,
                                         _dev_ptr(st, "status"), _dev_ptr(crc, "crc"), _stream_ptr(stream)))
    return (st, crc) if out_crc else st


def verify_blocks_host(file: bytes, handles, device: int = 0) -> np.ndarray:
    L = _bind()
    h = np.ascontiguousarray(handles, dtype=np.uint64).reshape(-1, 2)
    st = np.zeros(h.shape[0], dtype=np.uint32)
    buf = ctypes.create_string_buffer(bytes(file), max(len(file), 1))
    _check(L.lv_sst_verify_blocks_host(buf, len(file), h.ctypes.data, h.shape[0], st.ctypes.data, device))
    return st


# ---- lv_sst_build_*: the sorted memtable to an SSTable image -----------------
BUILD_STATUS = {1: "NO_TABLE", 2: "HANDLE_OVER", 4: "FILE_OVER", 8: "BLOCK_LARGE"}  # LV_SST_BUILD_*
BUILD_TOTALS = ("entries", "data_blocks", "file_bytes", "metaindex_offset", "metaindex_size", "index_offset",
                "index_size", "status")
DEFAULT_BLOCK_SIZE, DEFAULT_RESTART_INTERVAL = 4096, 16
# csrc/lvk/knobs.h: LVK_SB_TILE (entries per scan tile of the size, layout and
# index scans) and LVK_SB_WAVE_COPY (a key suffix or value of at least this
# many bytes is copied by its wave, not its lane) and LVK_SB_COPY_LANES (the
# lanes that share one such copy).  The GPU tests sweep around the first two.
SB_TILE = 1024
SB_WAVE_COPY = 64
SB_COPY_LANES = 16


class BuildOptions(ctypes.Structure):
    """lv_sst_build_options."""
    _fields_ = [("block_size", ctypes.c_uint32), ("restart_interval", ctypes.c_uint32)]


class BuildTotals(ctypes.Structure):
    """lv_sst_build_totals."""
    _fields_ = [(n, ctypes.c_uint64) for n in BUILD_TOTALS]


_build_bound = False


def _bind_build():
    global _build_bound
    L = _bind()
    if not _build_bound:
        vp, sz, u64, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32
        L.lv_sst_build_workspace_bytes.restype = sz
        L.lv_sst_build_workspace_bytes.argtypes = [sz, sz]
        L.lv_sst_build_file_bound.restype = u64
        L.lv_sst_build_file_bound.argtypes = [u64, u64, vp]
        L.lv_sst_build_device.restype = ctypes.c_int
        L.lv_sst_build_device.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, u64, vp, sz, vp, u32, vp, sz, vp]
        L.lv_sst_build_host.restype = ctypes.c_int
        L.lv_sst_build_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, u64, vp, sz, vp]
        _build_bound = True
    return L


def _options(block_size, restart_interval):
    if block_size is None and restart_interval is None:
        return None  # a NULL opt: the defaults
    return BuildOptions(DEFAULT_BLOCK_SIZE if block_size is None else block_size,
                        DEFAULT_RESTART_INTERVAL if restart_interval is None else restart_interval)


def build_workspace_bytes(op_cap: int, block_cap: int) -> int:
    return int(_bind_build().lv_sst_build_workspace_bytes(op_cap, block_cap))


def file_bound(payload_bytes: int, op_cap: int, block_size=None, restart_interval=None) -> int:
    """lv_sst_build_file_bound: a file_cap that suffices for disjoint extents."""
    opt = _options(block_size, restart_interval)
    return int(_bind_build().lv_sst_build_file_bound(payload_bytes, op_cap, ctypes.byref(opt) if opt else None))


def build_host(payload, ops, order, mt_totals, block_size=None, restart_interval=None, *, file_cap=None,
               block_cap=None, sizing=False, payload_bytes=None):
    """lv_sst_build_host: (file bytes, handles [(offset, size)], totals dict).
    sizing: file == NULL and file_cap == 0 (and no handles unless block_cap is
    given).  file_cap / block_cap default to what a sizing pass reports.
    payload_bytes overrides len(payload) (a sizing pass reads key bytes only).
    With a status the file and the handles come back as the canaries they were
    filled with, for the caller to check."""
    from .write_batch import OP_DTYPE
    L = _bind_build()
    pb = bytes(payload)
    pbuf = ctypes.create_string_buffer(pb, max(len(pb), 1))
    pn = len(pb) if payload_bytes is None else payload_bytes
    arr = np.ascontiguousarray(ops, dtype=OP_DTYPE)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    mt = MtTotals(mt_totals["entries"], mt_totals["user_keys"], mt_totals["status"])
    opt = _options(block_size, restart_interval)
    optp = ctypes.byref(opt) if opt else None
    tot = BuildTotals()

    def call(file_p, fcap, handles_p, bcap):
        rc = L.lv_sst_build_host(pbuf, pn, arr.ctypes.data if arr.size else None,
                                 order.ctypes.data if order.size else None, ctypes.byref(mt), optp, file_p, fcap,
                                 handles_p, bcap, ctypes.byref(tot))
        if rc != 0:
            raise LvError(f"lv_sst_build_host: {rc}")
        return {n: int(getattr(tot, n)) for n in BUILD_TOTALS}

    if sizing or file_cap is None or block_cap is None:
        if sizing and block_cap:
            hs = np.full(2 * (block_cap + 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            return b"", hs, call(None, 0, hs.ctypes.data, block_cap)
        t = call(None, 0, None, 0)
        if sizing:
            return b"", [], t
        file_cap = t["file_bytes"] if file_cap is None else file_cap
        block_cap = t["data_blocks"] if block_cap is None else block_cap
    guard = 64
    fbuf = np.full(file_cap + guard, 0xA5, dtype=np.uint8)
    hs = np.full(2 * (block_cap + 2) + 8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    t = call(fbuf.ctypes.data if file_cap else None, file_cap, hs.ctypes.data, block_cap)
    if t["status"]:
        return fbuf.tobytes(), hs, t
    assert (fbuf[t["file_bytes"]:] == 0xA5).all(), "lv_sst_build_host wrote at or beyond file_bytes"
    nh = t["data_blocks"] + 2 if t["file_bytes"] else 0
    assert (hs[2 * nh:] == 0xA5A5A5A5A5A5A5A5).all(), "lv_sst_build_host wrote handles beyond its count"
    return fbuf[: t["file_bytes"]].tobytes(), [(int(hs[2 * i]), int(hs[2 * i + 1])) for i in range(nh)], t


class Built:
    """Outputs of build_device, CUDA tensors written asynchronously: file_t
    (uint8, file_cap bytes and the guard), handles_t (int64, block_cap + 2
    pairs and the guard) and totals (int64[8], BUILD_TOTALS)."""
    _extra = 2  # the handle pairs behind the data blocks'
    _name = "lv_sst_build_device"

    def __init__(self, file_t, file_cap, handles_t, block_cap, totals, keep):
        self.file_t, self.file_cap, self.handles_t, self.block_cap, self.totals = file_t, file_cap, handles_t, block_cap, totals
        self._keep = keep  # the workspace and the inputs, until the work has run
        self._tot = None

    def sync_totals(self, check: bool = True) -> dict:
        """Waits for the call; the totals as a dict.  Raises LvError naming the
        status bits if one is set (nothing was written) unless check is False."""
        if self._tot is None:
            torch = _torch()
            torch.cuda.synchronize(self.totals.device)
            t = [int(v) for v in self.totals.cpu().numpy().view(np.uint64)]
            self._tot = dict(zip(BUILD_TOTALS, t))
            self._keep = None
        st = self._tot["status"]
        if st and check:
            names = "|".join(n for b, n in BUILD_STATUS.items() if st & b)
            raise LvError(f"{self._name}: status {names} (totals {self._tot})")
        return self._tot

    def file(self) -> bytes:
        """d_file[0, file_bytes) (synchronises)."""
        n = self.sync_totals()["file_bytes"]
        return self.file_t[:n].cpu().numpy().tobytes()

    def handles(self) -> list:
        """The data_blocks + 2 handles as (offset, size) pairs (synchronises)."""
        t = self.sync_totals()
        n = t["data_blocks"] + self._extra if t["file_bytes"] else 0
        h = self.handles_t[: 2 * n].cpu().numpy().view(np.uint64)
        return [(int(h[2 * i]), int(h[2 * i + 1])) for i in range(n)]

    def handles_view(self):
        """The written handles as an (n, 2) int64 CUDA tensor for verify_blocks
        (synchronises for the count)."""
        t = self.sync_totals()
        n = t["data_blocks"] + self._extra if t["file_bytes"] else 0
        return self.handles_t[: 2 * n].view(n, 2)


def build_device(table, *, block_size=None, restart_interval=None, file_cap=None, block_cap=None, workspace=None,
                 stream=None, fill=None, guard: int = 0, flags: int = 0, bits_per_key=None, bloom_reserved: int = 0):
    """lv_sst_build_device (with bits_per_key, lv_sst_build_bloom_device: see
    build_bloom_device) over a lvgpu.memtable.Table (its payload, ops,
    order and totals, read on the device).  file_cap defaults to file_bound of
    the payload and op_cap, block_cap to op_cap (a block holds at least one
    entry).  fill, a byte value, initialises d_file and d_handles with it first
    and guard allocates that many more bytes behind each (canaries).  Returns a
    Built; asynchronous on `stream`."""
    torch = _torch()
    L = _bind_build()
    dev = table.payload.device
    op_cap = int(table.op_cap)
    bloom = bits_per_key is not None
    if bloom:
        L = _bind_bloom()
        bopt = BloomOptions(bits_per_key, bloom_reserved)
    if file_cap is None:
        file_cap = (bloom_file_bound(table.payload.numel(), op_cap, bits_per_key) if bloom
                    else file_bound(table.payload.numel(), op_cap, block_size, restart_interval))
    if block_cap is None:
        block_cap = op_cap
    if workspace is None:
        need = (L.lv_sst_build_bloom_workspace_bytes if bloom else L.lv_sst_build_workspace_bytes)(op_cap, block_cap)
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    fbytes = (max(file_cap, 16) + guard + 15) & ~15
    hbytes = (16 * (block_cap + (3 if bloom else 2)) + guard + 7) & ~7
    if fill is None:
        file_t = torch.empty(fbytes, dtype=torch.uint8, device=dev)
        handles_t = torch.empty(hbytes, dtype=torch.uint8, device=dev).view(torch.int64)
    else:
        file_t = torch.full((fbytes,), fill, dtype=torch.uint8, device=dev)
        handles_t = torch.full((hbytes,), fill, dtype=torch.uint8, device=dev).view(torch.int64)
    totals = torch.empty(len(BUILD_TOTALS), dtype=torch.int64, device=dev)
    opt = _options(block_size, restart_interval)
    if bloom:
        bloom_totals = torch.empty(len(BLOOM_TOTALS), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            rc = L.lv_sst_build_bloom_device(_dev_ptr(table.payload, "payload"), table.payload.numel(),
                                             _dev_ptr(table.ops_t, "ops"), _dev_ptr(table.order_t, "order"),
                                             _dev_ptr(table.totals, "mt_totals"), op_cap,
                                             ctypes.byref(opt) if opt else None, ctypes.byref(bopt),
                                             _dev_ptr(file_t, "file"), file_cap, _dev_ptr(handles_t, "handles"),
                                             block_cap, _dev_ptr(totals, "totals"),
                                             _dev_ptr(bloom_totals, "bloom_totals"), flags,
                                             _dev_ptr(workspace, "workspace"), workspace.numel(), _stream_ptr(stream))
        if rc != 0:
            raise LvError(f"lv_sst_build_bloom_device: {lib().lv_last_error().decode()}")
        return BuiltBloom(file_t, file_cap, handles_t, block_cap, totals, (table, workspace), bloom_totals)
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_sst_build_device(_dev_ptr(table.payload, "payload"), table.payload.numel(),
                                   _dev_ptr(table.ops_t, "ops"), _dev_ptr(table.order_t, "order"),
                                   _dev_ptr(table.totals, "mt_totals"), op_cap, ctypes.byref(opt) if opt else None,
                                   _dev_ptr(file_t, "file"), file_cap, _dev_ptr(handles_t, "handles"), block_cap,
                                   _dev_ptr(totals, "totals"), flags, _dev_ptr(workspace, "workspace"),
                                   workspace.numel(), _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_sst_build_device: {lib().lv_last_error().decode()}")
    return Built(file_t, file_cap, handles_t, block_cap, totals, (table, workspace))


# ---- lv_sst_open_* / lv_sst_get_*: Table::Open and Table::InternalGet ----------
OPEN_STATUS = {1: "UPSTREAM", 2: "NOT_A_TABLE", 4: "BAD_FOOTER", 8: "BAD_INDEX", 16: "INDEX_SHAPE",
               32: "HANDLE_OVER"}  # LV_SST_OPEN_*
OPEN_UPSTREAM, OPEN_NOT_A_TABLE, OPEN_BAD_FOOTER, OPEN_BAD_INDEX, OPEN_INDEX_SHAPE, OPEN_HANDLE_OVER = OPEN_STATUS
(GET_ABSENT, GET_FOUND, GET_DELETED, GET_BAD_SEQ, GET_NO_TABLE, GET_BAD_QUERY, GET_CORRUPT) = range(7)  # LV_SST_GET_*
TABLE_FIELDS = ("file_bytes", "metaindex_offset", "metaindex_size", "index_offset", "index_size", "data_blocks",
                "reserved", "status")
GET_DTYPE = np.dtype([("val_off", "<u8"), ("tag", "<u8"), ("val_len", "<u4"), ("block", "<u4"), ("status", "<u4"),
                      ("reserved", "<u4")])
assert GET_DTYPE.itemsize == 32
HANDLE_CANARY = 0xA5A5A5A5A5A5A5A5


class SstTable(ctypes.Structure):
    """lv_sst_table."""
    _fields_ = [(n, ctypes.c_uint64) for n in TABLE_FIELDS]


class SstGetResult(ctypes.Structure):
    """lv_sst_get_result."""
    _fields_ = [("val_off", ctypes.c_uint64), ("tag", ctypes.c_uint64), ("val_len", ctypes.c_uint32),
                ("block", ctypes.c_uint32), ("status", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


_get_bound = False


def _bind_get():
    global _get_bound
    L = _bind()
    if not _get_bound:
        vp, sz, u64, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32
        L.lv_sst_open_host.restype = ctypes.c_int
        L.lv_sst_open_host.argtypes = [vp, u64, vp, sz, vp]
        L.lv_sst_get_host.restype = ctypes.c_int
        L.lv_sst_get_host.argtypes = [vp, vp, vp, sz, u64, vp]
        L.lv_sst_open_device.restype = ctypes.c_int
        L.lv_sst_open_device.argtypes = [vp, u64, vp, vp, vp, sz, vp, u32, vp]
        L.lv_sst_get_device.restype = ctypes.c_int
        L.lv_sst_get_device.argtypes = [vp, u64, vp, vp, sz, vp, vp, vp, sz, vp, u32, vp]
        _get_bound = True
    return L


def _status_names(st):
    return "|".join(n for b, n in OPEN_STATUS.items() if st & b)


def open_host(file, *, block_cap=None, handles=True):
    """lv_sst_open_host over the bytes `file`: (table dict, handles).  With
    status 0 the handles are the data_blocks + 2 (offset, size) pairs; with a
    status they are the canary-filled uint64 array the call was given, for the
    caller to check.  block_cap defaults to the table's data_blocks (a first
    call without handles reads it); handles=False passes NULL and block_cap 0."""
    L = _bind_get()
    fb = bytes(file)
    t = SstTable()

    def call(hp, bc):
        rc = L.lv_sst_open_host(fb, len(fb), hp, bc, ctypes.byref(t))
        if rc != 0:
            raise LvError(f"lv_sst_open_host: {rc}")
        return {n: int(getattr(t, n)) for n in TABLE_FIELDS}

    if not handles:
        return call(None, 0), []
    if block_cap is None:
        block_cap = call(None, 0)["data_blocks"]
    hs = np.full(2 * (block_cap + 2) + 8, HANDLE_CANARY, dtype=np.uint64)
    tab = call(hs.ctypes.data, block_cap)
    if tab["status"]:
        return tab, hs
    nh = tab["data_blocks"] + 2 if tab["file_bytes"] else 0
    assert (hs[2 * nh:] == HANDLE_CANARY).all(), "lv_sst_open_host wrote handles beyond its count"
    return tab, [(int(hs[2 * i]), int(hs[2 * i + 1])) for i in range(nh)]


def get_host(file, table, key, seq) -> dict:
    """lv_sst_get_host for one query over the bytes `file` and the table dict
    of open_host: a dict of the result's fields."""
    L = _bind_get()
    t = SstTable(*[int(table[n]) for n in TABLE_FIELDS])
    r = SstGetResult()
    kb = bytes(key)
    rc = L.lv_sst_get_host(file if isinstance(file, bytes) else bytes(file), ctypes.byref(t), kb, len(kb), seq,
                           ctypes.byref(r))
    if rc != 0:
        raise LvError(f"lv_sst_get_host: {rc}")
    return {n: int(getattr(r, n)) for n, _ in SstGetResult._fields_}


class Opened:
    """Outputs of open_device, CUDA tensors written asynchronously: table
    (int64[8], TABLE_FIELDS) and handles_t (int64, block_cap + 2 pairs and the
    guard, or None), with the image a get needs."""

    def __init__(self, file_t, file_cap, table, handles_t, block_cap, keep):
        self.file_t, self.file_cap, self.table, self.handles_t, self.block_cap = file_t, file_cap, table, handles_t, block_cap
        self._keep = keep
        self._tab = None

    def sync(self, check: bool = True) -> dict:
        """Waits for the call; the table as a dict.  Raises LvError naming the
        status bits if one is set unless check is False."""
        if self._tab is None:
            _torch().cuda.synchronize(self.table.device)
            self._tab = dict(zip(TABLE_FIELDS, (int(v) for v in self.table.cpu().numpy().view(np.uint64))))
            self._keep = None
        st = self._tab["status"]
        if st and check:
            raise LvError(f"lv_sst_open_device: status {_status_names(st)} (table {self._tab})")
        return self._tab

    def handles(self) -> list:
        """The data_blocks + 2 handles as (offset, size) pairs (synchronises)."""
        t = self.sync()
        n = t["data_blocks"] + 2 if t["file_bytes"] else 0
        h = self.handles_t[: 2 * n].cpu().numpy().view(np.uint64)
        return [(int(h[2 * i]), int(h[2 * i + 1])) for i in range(n)]

    def handles_view(self):
        """The written handles as an (n, 2) int64 CUDA tensor for verify_blocks
        (synchronises for the count)."""
        t = self.sync()
        n = t["data_blocks"] + 2 if t["file_bytes"] else 0
        return self.handles_t[: 2 * n].view(n, 2)


def open_device(file_t, file_bytes, upstream_status=None, *, file_cap=None, block_cap=0, handles=True, table=None,
                handles_t=None, stream=None, fill=None, guard: int = 0, flags: int = 0):
    """lv_sst_open_device.  file_t is a uint8 CUDA tensor (any byte alignment:
    a slice will do) that holds the image; file_bytes and upstream_status are
    int64 CUDA tensors whose first element is read on the device (e.g.
    Built.totals[2:3] and Built.totals[7:8]).  file_cap defaults to
    file_t.numel().  handles=False passes a NULL d_handles.  table / handles_t
    reuse the outputs of an earlier call (graph replays).  fill / guard as in
    build_device.  Returns an Opened; asynchronous on `stream`."""
    torch = _torch()
    L = _bind_get()
    dev = file_t.device
    if file_t.dtype != torch.uint8:
        raise LvError("file_t must be a uint8 tensor")
    for name, t in (("file_bytes", file_bytes), ("upstream_status", upstream_status)):
        if t is None and name == "upstream_status":
            continue
        if t is None or t.dtype != torch.int64 or t.device != dev or t.numel() < 1:
            raise LvError(f"{name} must be an int64 tensor on the file's device")
    file_cap = file_t.numel() if file_cap is None else int(file_cap)
    if handles and handles_t is None:
        hbytes = (16 * (block_cap + 2) + guard + 7) & ~7
        if fill is None:
            handles_t = torch.empty(hbytes, dtype=torch.uint8, device=dev).view(torch.int64)
        else:
            handles_t = torch.full((hbytes,), fill, dtype=torch.uint8, device=dev).view(torch.int64)
    if not handles:
        handles_t = None
    if table is None:
        table = torch.empty(len(TABLE_FIELDS), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_sst_open_device(_dev_ptr(file_t, "file") if file_cap else None, file_cap,
                                  _dev_ptr(file_bytes, "file_bytes"), _dev_ptr(upstream_status, "upstream_status"),
                                  _dev_ptr(handles_t, "handles"), block_cap, _dev_ptr(table, "table"), flags,
                                  _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_sst_open_device: {lib().lv_last_error().decode()}")
    return Opened(file_t, file_cap, table, handles_t, block_cap, (file_bytes, upstream_status))


class Gets:
    """Output of get_device: res, a uint8 CUDA tensor of nq lv_sst_get_result
    (and the guard), written asynchronously."""

    def __init__(self, res, nq, keep):
        self.res, self.nq = res, nq
        self._keep = keep  # the query arrays, until the work has run
        self._out = None

    def sync(self):
        """Waits for the call; the results as a structured array (GET_DTYPE)."""
        if self._out is None:
            _torch().cuda.synchronize(self.res.device)
            self._out = self.res[: self.nq * 32].cpu().numpy().view(GET_DTYPE).copy()
            self._keep = None
        return self._out


def get_device(opened, qkeys, q_off, q_len, q_seq, *, nq=None, res=None, stream=None, fill=None, guard: int = 0,
               flags: int = 0):
    """lv_sst_get_device over an Opened (its image and its table, read on the
    device).  qkeys is a uint8 CUDA tensor, q_off / q_seq int64 and q_len int32
    CUDA tensors of nq entries.  res reuses an earlier call's tensor.  Returns
    a Gets; asynchronous on `stream`."""
    torch = _torch()
    L = _bind_get()
    dev = opened.file_t.device
    if qkeys.dtype != torch.uint8 or q_off.dtype != torch.int64 or q_seq.dtype != torch.int64 or \
            q_len.dtype != torch.int32:
        raise LvError("qkeys must be uint8, q_off and q_seq int64, q_len int32")
    nq = int(min(q_off.numel(), q_len.numel(), q_seq.numel())) if nq is None else int(nq)
    if min(q_off.numel(), q_len.numel(), q_seq.numel()) < nq:
        raise LvError("the query arrays must hold nq entries")
    if res is None:
        nbytes = (max(nq * 32, 16) + guard + 7) & ~7
        if fill is None:
            res = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        else:
            res = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.lv_sst_get_device(_dev_ptr(opened.file_t, "file") if opened.file_cap else None, opened.file_cap,
                                 _dev_ptr(opened.table, "table"), _dev_ptr(qkeys, "qkeys") if qkeys.numel() else None,
                                 qkeys.numel(), _dev_ptr(q_off, "q_off"), _dev_ptr(q_len, "q_len"),
                                 _dev_ptr(q_seq, "q_seq"), nq, _dev_ptr(res, "results"), flags, _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_sst_get_device: {lib().lv_last_error().decode()}")
    return Gets(res, nq, (opened, qkeys, q_off, q_len, q_seq))


# ---- lv_sst_scan_*: a table image back to a sorted op table --------------------
SCAN_STATUS = {1: "UPSTREAM", 2: "NO_TABLE", 4: "CORRUPT", 8: "BLOCK_OVER", 16: "OP_OVER",
               32: "ARENA_OVER"}  # LV_SST_SCAN_*
SCAN_UPSTREAM, SCAN_NO_TABLE, SCAN_CORRUPT, SCAN_BLOCK_OVER, SCAN_OP_OVER, SCAN_ARENA_OVER = SCAN_STATUS
SCAN_MT_UNORDERED = 8  # a bit of the memtable totals' status only
SCAN_TOTALS = ("entries", "arena_bytes", "table_entries", "table_bytes", "data_blocks", "runs", "reserved", "status")
# csrc/lvk/knobs.h: LVK_SS_TILE (blocks, and restart runs, per scan tile) and
# LVK_SS_WAVE_COPY (a key prefix, key suffix or value of at least this many
# bytes is copied by its wave, not its lane).  The GPU tests sweep around both.
SS_TILE = 1024
SS_WAVE_COPY = 64


class ScanTotals(ctypes.Structure):
    """lv_sst_scan_totals."""
    _fields_ = [(n, ctypes.c_uint64) for n in SCAN_TOTALS]


_scan_bound = False


def _bind_scan():
    global _scan_bound
    L = _bind_get()
    if not _scan_bound:
        vp, sz, u64, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32
        L.lv_sst_scan_workspace_bytes.restype = sz
        L.lv_sst_scan_workspace_bytes.argtypes = [sz, sz]
        L.lv_sst_scan_device.restype = ctypes.c_int
        L.lv_sst_scan_device.argtypes = [vp, u64, vp, vp, vp, u64, vp, sz, sz, vp, vp, vp, u32, vp, sz, vp]
        L.lv_sst_scan_host.restype = ctypes.c_int
        L.lv_sst_scan_host.argtypes = [vp, vp, vp, vp, u64, vp, sz, vp, vp, vp]
        _scan_bound = True
    return L


def scan_workspace_bytes(op_cap: int, block_cap: int) -> int:
    return int(_bind_scan().lv_sst_scan_workspace_bytes(op_cap, block_cap))


def scan_host(file, table, prev=None, *, arena=None, ops=None, arena_cap=None, op_cap=None, order=False, fill=0xA5):
    """lv_sst_scan_host over the bytes `file` and the table dict of open_host:
    (totals dict, ops array, arena bytes, mt_totals dict or None).  prev is the
    totals dict of the scan to append to, with `arena` (a uint8 array) and
    `ops` that scan returned whole (see below).  arena_cap / op_cap default to
    what a sizing call reports.  The arena and the ops come back whole, all
    arena_cap bytes and op_cap ops, the part no entry was written to still
    holding `fill`, for the caller to check or to append to; with order=True
    the fourth value carries the order array under "order"."""
    from .write_batch import OP_DTYPE
    L = _bind_scan()
    fb = bytes(file)
    t = SstTable(*[int(table[n]) for n in TABLE_FIELDS])
    pv = None if prev is None else ScanTotals(*[int(prev[n]) for n in SCAN_TOTALS])
    tot = ScanTotals()

    def call(ap, acap, opp, ocap, orp, mtp):
        rc = L.lv_sst_scan_host(fb, ctypes.byref(t), ctypes.byref(pv) if pv else None, ap, acap, opp, ocap, orp, mtp,
                                ctypes.byref(tot))
        if rc != 0:
            raise LvError(f"lv_sst_scan_host: {rc}")
        return {n: int(getattr(tot, n)) for n in SCAN_TOTALS}

    if arena_cap is None or op_cap is None:
        sized = call(None, 0, None, 0, None, None)
        arena_cap = sized["arena_bytes"] if arena_cap is None else arena_cap
        op_cap = sized["entries"] if op_cap is None else op_cap
    abuf = np.full(arena_cap, fill, dtype=np.uint8)
    obuf = np.frombuffer(bytes([fill]) * (32 * op_cap), dtype=OP_DTYPE).copy()
    if arena is not None:
        n = min(len(arena), arena_cap)
        abuf[:n] = np.frombuffer(bytes(arena), dtype=np.uint8)[:n]
    if ops is not None:
        n = min(len(ops), op_cap)
        obuf[:n] = ops[:n]
    orr = np.full(max(op_cap, 1), 0xA5A5A5A5, dtype=np.uint32) if order else None
    mt = MtTotals() if order else None
    tt = call(abuf.ctypes.data if arena_cap else None, arena_cap, obuf.ctypes.data if op_cap else None, op_cap,
              orr.ctypes.data if order else None, ctypes.byref(mt) if order else None)
    mtd = None
    if order:
        mtd = dict(entries=int(mt.entries), user_keys=int(mt.user_keys), status=int(mt.status), order=orr[:op_cap])
    return tt, obuf, abuf, mtd


class Scanned:
    """Outputs of scan_device, CUDA tensors written asynchronously: arena_t
    (uint8; the arena is arena_t[arena_shift:]), ops_t (uint8, 32 bytes per
    lv_wb_op), totals (int64[8], SCAN_TOTALS) and, with order=True, order_t
    (int32) and mt_totals (int64[3])."""

    def __init__(self, arena_t, arena_cap, ops_t, op_cap, block_cap, totals, order_t, mt_totals, keep):
        self.arena_t, self.arena_cap, self.ops_t, self.op_cap, self.block_cap = arena_t, arena_cap, ops_t, op_cap, block_cap
        self.totals, self.order_t, self.mt_totals = totals, order_t, mt_totals
        self._keep = keep
        self._tot = None

    def sync(self, check: bool = True) -> dict:
        """Waits for the call; the totals as a dict.  Raises LvError naming the
        status bits if one is set (nothing was written) unless check is False."""
        if self._tot is None:
            _torch().cuda.synchronize(self.totals.device)
            self._tot = dict(zip(SCAN_TOTALS, (int(v) for v in self.totals.cpu().numpy().view(np.uint64))))
            self._keep = None
        st = self._tot["status"]
        if st and check:
            names = "|".join(n for b, n in SCAN_STATUS.items() if st & b)
            raise LvError(f"lv_sst_scan_device: status {names} (totals {self._tot})")
        return self._tot

    def ops(self):
        """d_ops[0, entries) as a structured array (synchronises)."""
        from .write_batch import OP_DTYPE
        n = self.sync()["entries"]
        return self.ops_t[: 32 * n].cpu().numpy().view(OP_DTYPE).copy()

    def arena(self) -> bytes:
        """d_arena[0, arena_bytes) (synchronises)."""
        n = self.sync()["arena_bytes"]
        return self.arena_t[:n].cpu().numpy().tobytes()

    def mt(self) -> dict:
        """*d_mt_totals as a dict (synchronises)."""
        self.sync(check=False)
        return dict(zip(("entries", "user_keys", "status"), (int(v) for v in self.mt_totals.cpu().numpy().view(np.uint64))))

    def memtable(self):
        """The quadruple as a lvgpu.memtable.Table: what build_device here and
        lvgpu.memtable.get_device take where they take a memtable build's
        result.  Needs order=True; does not synchronise."""
        from .memtable import Table
        if self.order_t is None:
            raise LvError("scan_device was called without order=True")
        return Table(self.arena_t[: max(self.arena_cap, 0)], self.ops_t, self.op_cap, self.order_t, self.mt_totals, self)


def scan_device(opened, prev=None, *, arena_cap=None, op_cap=None, block_cap=None, order=False, arena_t=None,
                ops_t=None, order_t=None, mt_totals=None, totals=None, workspace=None, stream=None, fill=None,
                guard: int = 0, flags: int = 0):
    """lv_sst_scan_device over an Opened (its image and its table, read on the
    device).  prev is the Scanned to append to: its arena and ops are reused
    (with its caps) and its totals are d_prev.  arena_cap defaults to the
    image's capacity (a table's keys and values are no longer than its file
    only when keys share nothing; size by a retry on ARENA_OVER), op_cap to
    file_cap // 11 + 1 (an entry with a tag takes at least 11 bytes), block_cap
    to the Opened's, or file_cap // 13 + 1.  arena_t may be any uint8 CUDA
    tensor (a slice: any alignment).  order=True also writes d_order and
    d_mt_totals.  fill / guard as in build_device.  Returns a Scanned;
    asynchronous on `stream`."""
    torch = _torch()
    L = _bind_scan()
    dev = opened.file_t.device
    if prev is not None:
        arena_t, arena_cap, ops_t, op_cap = prev.arena_t, prev.arena_cap, prev.ops_t, prev.op_cap
    if arena_cap is None:
        arena_cap = int(opened.file_cap) if arena_t is None else arena_t.numel()
    if op_cap is None:
        op_cap = opened.file_cap // 11 + 1
    if block_cap is None:
        block_cap = opened.block_cap or opened.file_cap // 13 + 1

    def alloc(nbytes, dtype=None):
        nbytes = (max(nbytes, 16) + guard + 15) & ~15
        t = (torch.empty(nbytes, dtype=torch.uint8, device=dev) if fill is None
             else torch.full((nbytes,), fill, dtype=torch.uint8, device=dev))
        return t if dtype is None else t.view(dtype)
    if arena_t is None:
        arena_t = alloc(arena_cap)
    if ops_t is None:
        ops_t = alloc(32 * op_cap)
    if order and order_t is None:
        order_t = alloc(4 * op_cap, torch.int32)
    if order and mt_totals is None:
        mt_totals = torch.empty(3, dtype=torch.int64, device=dev)
    if totals is None:
        totals = torch.empty(len(SCAN_TOTALS), dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(L.lv_sst_scan_workspace_bytes(op_cap, block_cap), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.lv_sst_scan_device(_dev_ptr(opened.file_t, "file") if opened.file_cap else None, opened.file_cap,
                                  _dev_ptr(opened.table, "table"), _dev_ptr(prev.totals, "prev") if prev else None,
                                  _dev_ptr(arena_t, "arena") if arena_cap else None, arena_cap,
                                  _dev_ptr(ops_t, "ops") if op_cap else None, op_cap, block_cap,
                                  _dev_ptr(order_t, "order") if order else None,
                                  _dev_ptr(mt_totals, "mt_totals") if order else None, _dev_ptr(totals, "totals"),
                                  flags, _dev_ptr(workspace, "workspace"), workspace.numel(), _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_sst_scan_device: {lib().lv_last_error().decode()}")
    return Scanned(arena_t, arena_cap, ops_t, op_cap, block_cap, totals, order_t if order else None,
                   mt_totals if order else None, (opened, prev, workspace))


# ---- Bloom filter blocks: lv_bloom_*, lv_sst_build_bloom_*, lv_sst_bloom_open_*, lv_sst_get_bloom_* ----
BLOOM_NAME = b"filter.leveldb.BuiltinBloomFilter2"  # LV_SST_BLOOM_NAME
FILTER_BASE_LG = 11                                  # LV_SST_FILTER_BASE_LG
GET_FILTERED = 1                                     # lv_sst_get_result.reserved of a query the filter rejected
BLOOM_TOTALS = ("filter_offset", "filter_size", "filters", "filter_keys")
BLOOM_FIELDS = ("filter_offset", "filter_size", "array_offset", "num", "base_lg", "present", "why", "reserved")
BLOOM_WHY = {0: "", 1: "TABLE", 2: "EMPTY", 3: "BAD_METAINDEX", 4: "NO_ENTRY", 5: "BAD_HANDLE", 6: "BAD_TYPE",
             7: "SHORT", 8: "BAD_ARRAY"}  # LV_SST_BLOOM_*
SB_BLOOM_LDS = 2048  # csrc/sst_build.hip kSbBloomLds: filter bytes a wave holds in LDS; larger ones take the atomic path


class BloomOptions(ctypes.Structure):
    """lv_sst_bloom_options."""
    _fields_ = [("bits_per_key", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class BloomTotals(ctypes.Structure):
    """lv_sst_bloom_totals."""
    _fields_ = [(n, ctypes.c_uint64) for n in BLOOM_TOTALS]


class SstBloom(ctypes.Structure):
    """lv_sst_bloom."""
    _fields_ = [(n, ctypes.c_uint64) for n in BLOOM_FIELDS]


_bloom_bound = False


def _bind_bloom():
    global _bloom_bound
    L = _bind_get()
    _bind_build()
    if not _bloom_bound:
        vp, sz, u64, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32
        L.lv_bloom_hash.restype = u32
        L.lv_bloom_hash.argtypes = [vp, sz]
        L.lv_bloom_filter_bytes.restype = sz
        L.lv_bloom_filter_bytes.argtypes = [sz, u32]
        L.lv_bloom_create_filter.restype = ctypes.c_int
        L.lv_bloom_create_filter.argtypes = [vp, vp, vp, sz, u32, vp]
        L.lv_bloom_key_may_match.restype = ctypes.c_int
        L.lv_bloom_key_may_match.argtypes = [vp, sz, vp, sz]
        L.lv_sst_build_bloom_workspace_bytes.restype = sz
        L.lv_sst_build_bloom_workspace_bytes.argtypes = [sz, sz]
        L.lv_sst_build_bloom_file_bound.restype = u64
        L.lv_sst_build_bloom_file_bound.argtypes = [u64, u64, vp, vp]
        L.lv_sst_build_bloom_device.restype = ctypes.c_int
        L.lv_sst_build_bloom_device.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, vp, u64, vp, sz, vp, vp, u32, vp, sz, vp]
        L.lv_sst_build_bloom_host.restype = ctypes.c_int
        L.lv_sst_build_bloom_host.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, u64, vp, sz, vp, vp]
        L.lv_sst_bloom_open_device.restype = ctypes.c_int
        L.lv_sst_bloom_open_device.argtypes = [vp, u64, vp, vp, u32, vp]
        L.lv_sst_bloom_open_host.restype = ctypes.c_int
        L.lv_sst_bloom_open_host.argtypes = [vp, vp, vp]
        L.lv_sst_get_bloom_device.restype = ctypes.c_int
        L.lv_sst_get_bloom_device.argtypes = [vp, u64, vp, vp, vp, sz, vp, vp, vp, sz, vp, u32, vp]
        L.lv_sst_get_bloom_host.restype = ctypes.c_int
        L.lv_sst_get_bloom_host.argtypes = [vp, vp, vp, vp, sz, u64, vp]
        _bloom_bound = True
    return L


def bloom_hash(key) -> int:
    """lv_bloom_hash: lv_hash(key, 0xbc9f1d34)."""
    kb = bytes(key)
    return int(_bind_bloom().lv_bloom_hash(kb, len(kb)))


def bloom_filter_bytes(n: int, bits_per_key: int) -> int:
    return int(_bind_bloom().lv_bloom_filter_bytes(n, bits_per_key))


def bloom_create_filter(keys, bits_per_key: int) -> bytes:
    """lv_bloom_create_filter over a list of keys (packed with one gap byte
    between them, so that they sit at every alignment)."""
    L = _bind_bloom()
    blob, off, ln = bytearray(), [], []
    for k in keys:
        blob += b"\xee"
        off.append(len(blob))
        ln.append(len(k))
        blob += bytes(k)
    off = np.array(off, dtype=np.uint64)
    ln = np.array(ln, dtype=np.uint32)
    out = ctypes.create_string_buffer(L.lv_bloom_filter_bytes(len(keys), bits_per_key) + 8)
    out.raw = b"\xa5" * len(out)
    rc = L.lv_bloom_create_filter(bytes(blob), off.ctypes.data if len(keys) else None,
                                  ln.ctypes.data if len(keys) else None, len(keys), bits_per_key, out)
    if rc != 0:
        raise LvError(f"lv_bloom_create_filter: {rc}")
    assert out.raw[-8:] == b"\xa5" * 8, "lv_bloom_create_filter wrote beyond lv_bloom_filter_bytes"
    return out.raw[:-8]


def bloom_key_may_match(key, filt) -> bool:
    kb, fb = bytes(key), bytes(filt)
    return bool(_bind_bloom().lv_bloom_key_may_match(kb, len(kb), fb, len(fb)))


def build_bloom_workspace_bytes(op_cap: int, block_cap: int) -> int:
    return int(_bind_bloom().lv_sst_build_bloom_workspace_bytes(op_cap, block_cap))


def bloom_file_bound(payload_bytes: int, op_cap: int, bits_per_key: int) -> int:
    """lv_sst_build_bloom_file_bound."""
    b = BloomOptions(bits_per_key, 0)
    return int(_bind_bloom().lv_sst_build_bloom_file_bound(payload_bytes, op_cap, None, ctypes.byref(b)))


def build_bloom_host(payload, ops, order, mt_totals, bits_per_key=10, block_size=None, restart_interval=None, *,
                     file_cap=None, block_cap=None, sizing=False, reserved=0):
    """lv_sst_build_bloom_host: (file bytes, handles, totals dict, bloom totals
    dict), as build_host; data_blocks + 3 handles."""
    from .write_batch import OP_DTYPE
    L = _bind_bloom()
    pb = bytes(payload)
    pbuf = ctypes.create_string_buffer(pb, max(len(pb), 1))
    arr = np.ascontiguousarray(ops, dtype=OP_DTYPE)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    mt = MtTotals(mt_totals["entries"], mt_totals["user_keys"], mt_totals["status"])
    opt = _options(block_size, restart_interval)
    bopt = BloomOptions(bits_per_key, reserved)
    tot, btot = BuildTotals(), BloomTotals()

    def call(file_p, fcap, handles_p, bcap):
        rc = L.lv_sst_build_bloom_host(pbuf, len(pb), arr.ctypes.data if arr.size else None,
                                       order.ctypes.data if order.size else None, ctypes.byref(mt),
                                       ctypes.byref(opt) if opt else None, ctypes.byref(bopt), file_p, fcap, handles_p,
                                       bcap, ctypes.byref(tot), ctypes.byref(btot))
        if rc != 0:
            raise LvError(f"lv_sst_build_bloom_host: {rc}")
        return ({n: int(getattr(tot, n)) for n in BUILD_TOTALS}, {n: int(getattr(btot, n)) for n in BLOOM_TOTALS})

    if sizing or file_cap is None or block_cap is None:
        t, bt = call(None, 0, None, 0)
        if sizing:
            return b"", [], t, bt
        file_cap = t["file_bytes"] if file_cap is None else file_cap
        block_cap = t["data_blocks"] if block_cap is None else block_cap
    fbuf = np.full(file_cap + 64, 0xA5, dtype=np.uint8)
    hs = np.full(2 * (block_cap + 3) + 8, HANDLE_CANARY, dtype=np.uint64)
    t, bt = call(fbuf.ctypes.data if file_cap else None, file_cap, hs.ctypes.data, block_cap)
    if t["status"]:
        return fbuf.tobytes(), hs, t, bt
    assert (fbuf[t["file_bytes"]:] == 0xA5).all(), "lv_sst_build_bloom_host wrote at or beyond file_bytes"
    nh = t["data_blocks"] + 3 if t["file_bytes"] else 0
    assert (hs[2 * nh:] == HANDLE_CANARY).all(), "lv_sst_build_bloom_host wrote handles beyond its count"
    return fbuf[: t["file_bytes"]].tobytes(), [(int(hs[2 * i]), int(hs[2 * i + 1])) for i in range(nh)], t, bt


class BuiltBloom(Built):
    """Outputs of build_bloom_device: a Built with data_blocks + 3 handles and
    bloom_totals (int64[4], BLOOM_TOTALS)."""
    _extra = 3
    _name = "lv_sst_build_bloom_device"

    def __init__(self, file_t, file_cap, handles_t, block_cap, totals, keep, bloom_totals):
        super().__init__(file_t, file_cap, handles_t, block_cap, totals, keep)
        self.bloom_totals = bloom_totals

    def sync_bloom_totals(self) -> dict:
        self.sync_totals(check=False)
        return dict(zip(BLOOM_TOTALS, (int(v) for v in self.bloom_totals.cpu().numpy().view(np.uint64))))


def build_bloom_device(table, bits_per_key=10, **kw):
    """lv_sst_build_bloom_device over a lvgpu.memtable.Table: build_device's
    keywords; file_cap defaults to bloom_file_bound.  Returns a BuiltBloom."""
    return build_device(table, bits_per_key=bits_per_key, **kw)


def bloom_open_host(file, table) -> dict:
    """lv_sst_bloom_open_host over the bytes `file` and the table dict of
    open_host: the lv_sst_bloom as a dict."""
    L = _bind_bloom()
    t = SstTable(*[int(table[n]) for n in TABLE_FIELDS])
    b = SstBloom()
    fb = bytes(file)
    rc = L.lv_sst_bloom_open_host(fb, ctypes.byref(t), ctypes.byref(b))
    if rc != 0:
        raise LvError(f"lv_sst_bloom_open_host: {rc}")
    return {n: int(getattr(b, n)) for n in BLOOM_FIELDS}


def get_bloom_host(file, table, bloom, key, seq) -> dict:
    """lv_sst_get_bloom_host for one query: a dict of the result's fields."""
    L = _bind_bloom()
    t = SstTable(*[int(table[n]) for n in TABLE_FIELDS])
    b = SstBloom(*[int(bloom[n]) for n in BLOOM_FIELDS])
    r = SstGetResult()
    kb = bytes(key)
    rc = L.lv_sst_get_bloom_host(file if isinstance(file, bytes) else bytes(file), ctypes.byref(t), ctypes.byref(b), kb,
                                 len(kb), seq, ctypes.byref(r))
    if rc != 0:
        raise LvError(f"lv_sst_get_bloom_host: {rc}")
    return {n: int(getattr(r, n)) for n, _ in SstGetResult._fields_}


def bloom_open_device(opened, *, bloom=None, stream=None, flags: int = 0):
    """lv_sst_bloom_open_device over an Opened: the lv_sst_bloom as an int64[8]
    CUDA tensor (BLOOM_FIELDS), written asynchronously on `stream`.  bloom
    reuses an earlier call's tensor."""
    torch = _torch()
    L = _bind_bloom()
    dev = opened.file_t.device
    if bloom is None:
        bloom = torch.empty(len(BLOOM_FIELDS), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = L.lv_sst_bloom_open_device(_dev_ptr(opened.file_t, "file") if opened.file_cap else None, opened.file_cap,
                                        _dev_ptr(opened.table, "table"), _dev_ptr(bloom, "bloom"), flags,
                                        _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_sst_bloom_open_device: {lib().lv_last_error().decode()}")
    return bloom


def bloom_dict(bloom_t) -> dict:
    """An lv_sst_bloom tensor as a dict (synchronises)."""
    _torch().cuda.synchronize(bloom_t.device)
    return dict(zip(BLOOM_FIELDS, (int(v) for v in bloom_t.cpu().numpy().view(np.uint64))))


def get_bloom_device(opened, bloom, qkeys, q_off, q_len, q_seq, *, nq=None, res=None, stream=None, fill=None,
                     guard: int = 0, flags: int = 0):
    """lv_sst_get_bloom_device: get_device with the lv_sst_bloom tensor of
    bloom_open_device, read on the device.  Returns a Gets."""
    torch = _torch()
    L = _bind_bloom()
    dev = opened.file_t.device
    if qkeys.dtype != torch.uint8 or q_off.dtype != torch.int64 or q_seq.dtype != torch.int64 or \
            q_len.dtype != torch.int32:
        raise LvError("qkeys must be uint8, q_off and q_seq int64, q_len int32")
    nq = int(min(q_off.numel(), q_len.numel(), q_seq.numel())) if nq is None else int(nq)
    if min(q_off.numel(), q_len.numel(), q_seq.numel()) < nq:
        raise LvError("the query arrays must hold nq entries")
    if res is None:
        nbytes = (max(nq * 32, 16) + guard + 7) & ~7
        res = (torch.empty(nbytes, dtype=torch.uint8, device=dev) if fill is None
               else torch.full((nbytes,), fill, dtype=torch.uint8, device=dev))
    with torch.cuda.device(dev):
        rc = L.lv_sst_get_bloom_device(_dev_ptr(opened.file_t, "file") if opened.file_cap else None, opened.file_cap,
                                       _dev_ptr(opened.table, "table"), _dev_ptr(bloom, "bloom"),
                                       _dev_ptr(qkeys, "qkeys") if qkeys.numel() else None, qkeys.numel(),
                                       _dev_ptr(q_off, "q_off"), _dev_ptr(q_len, "q_len"), _dev_ptr(q_seq, "q_seq"),
                                       nq, _dev_ptr(res, "results"), flags, _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_sst_get_bloom_device: {lib().lv_last_error().decode()}")
    return Gets(res, nq, (opened, bloom, qkeys, q_off, q_len, q_seq))
