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
    output_workspace_bytes(op_cap, block_cap, files_cap), output_arena_bound(...)
    output_host(payload, ops, order, mt_totals, max_file_bytes, ...)
                                      lv_compact_output_host: a HostOutput (the
                                      compaction's output as a run of tables)
    output_device(table, max_file_bytes, ...)
                                      lv_compact_output_device over a Table (a
                                      Filtered too): an Output, whose tables_t,
                                      blooms_t, version_files_t and bounds_t
                                      lvgpu.version.open_device takes
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


# ---- lv_compact_output_*: a compaction's output as a run of tables -------------
OUT_STATUS = {1: "NO_TABLE", 2: "HANDLE_OVER", 4: "ARENA_OVER", 8: "BLOCK_LARGE", 16: "FILES_OVER",
              32: "BOUND_OVER"}  # LV_COMPACT_OUT_*
OUT_NO_TABLE, OUT_HANDLE_OVER, OUT_ARENA_OVER, OUT_BLOCK_LARGE, OUT_FILES_OVER, OUT_BOUND_OVER = OUT_STATUS
OUT_TOTALS = ("entries", "files", "data_blocks", "arena_bytes", "handle_pairs", "bound_bytes", "reserved", "status")
OUT_FILE_FIELDS = ("first_entry", "entries", "file_off", "file_bytes", "data_blocks", "first_handle", "filter_keys",
                   "reserved")
OUT_FILE_DTYPE = np.dtype([(n, "<u8") for n in OUT_FILE_FIELDS])  # lv_compact_output_file
DEFAULT_MAX_FILE_BYTES = 2 << 20  # upstream's max_file_size


class OutputTotals(ctypes.Structure):
    """lv_compact_output_totals."""
    _fields_ = [(n, ctypes.c_uint64) for n in OUT_TOTALS]


_out_bound = False


def _bind_output():
    global _out_bound
    L = lib()
    if not _out_bound:
        vp, sz, u64, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32
        L.lv_compact_output_workspace_bytes.restype = sz
        L.lv_compact_output_workspace_bytes.argtypes = [sz, sz, sz]
        L.lv_compact_output_arena_bound.restype = u64
        L.lv_compact_output_arena_bound.argtypes = [u64, u64, vp, vp]
        head = [vp, sz, vp, vp, vp, sz, vp, vp, u64, u64, u32, u64, vp, u64, vp, sz, vp, vp, vp, vp, sz, vp, u64, vp, vp]
        L.lv_compact_output_host.restype = ctypes.c_int
        L.lv_compact_output_host.argtypes = head
        L.lv_compact_output_device.restype = ctypes.c_int
        L.lv_compact_output_device.argtypes = head + [u32, vp, sz, vp]
        _out_bound = True
    return L


def _out_options(block_size, restart_interval, bits_per_key, bloom_reserved=0):
    from .table import BloomOptions, _options
    opt = _options(block_size, restart_interval)
    bopt = None if bits_per_key is None else BloomOptions(bits_per_key, bloom_reserved)
    return opt, bopt


def output_workspace_bytes(op_cap: int, block_cap: int, files_cap: int) -> int:
    return int(_bind_output().lv_compact_output_workspace_bytes(op_cap, block_cap, files_cap))


def output_arena_bound(payload_bytes: int, op_cap: int, bits_per_key=None, block_size=None, restart_interval=None) -> int:
    """lv_compact_output_arena_bound: an arena_cap that suffices for disjoint extents."""
    opt, bopt = _out_options(block_size, restart_interval, bits_per_key)
    return int(_bind_output().lv_compact_output_arena_bound(payload_bytes, op_cap, ctypes.byref(opt) if opt else None,
                                                            ctypes.byref(bopt) if bopt else None))


class HostOutput:
    """Outputs of output_host: totals (dict) and the whole buffers the call was
    given, filled with `fill` first: arena (uint8, arena_cap and a guard),
    handles (uint64), files (OUT_FILE_DTYPE), tables / blooms (uint64 [n, 8]),
    version_files (lvgpu.version.FILE_DTYPE), bounds (uint8) and the cursor."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def image(self, k) -> bytes:
        f = self.files[k]
        return self.arena[int(f["file_off"]): int(f["file_off"] + f["file_bytes"])].tobytes()

    def file_handles(self, k, extra) -> list:
        f = self.files[k]
        at, n = int(f["first_handle"]), int(f["data_blocks"]) + extra
        return [(int(self.handles[2 * i]), int(self.handles[2 * i + 1])) for i in range(at, at + n)]


def output_host(payload, ops, order, mt_totals, max_file_bytes=DEFAULT_MAX_FILE_BYTES, *, bits_per_key=None,
                block_size=None, restart_interval=None, first_number=1, level=1, images_off=0, arena_cap=None,
                block_cap=None, files_cap=None, bound_cap=None, bound_used=0, sizing=False, blooms=True,
                version_files=True, op_cap=None, payload_bytes=None, bloom_reserved=0, fill=0xA5, guard=64):
    """lv_compact_output_host: a HostOutput.  The capacities default to what a
    sizing pass reports; sizing=True is that pass alone (arena == NULL,
    arena_cap == 0).  Raises LvError on LV_ERR_INVALID."""
    from .version import FILE_DTYPE
    L = _bind_output()
    pb = bytes(payload)
    pbuf = ctypes.create_string_buffer(pb, max(len(pb), 1))
    pn = len(pb) if payload_bytes is None else payload_bytes
    arr = np.ascontiguousarray(ops, dtype=OP_DTYPE)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    op_cap = arr.size if op_cap is None else int(op_cap)
    mt = MtTotals(mt_totals["entries"], mt_totals["user_keys"], mt_totals["status"])
    opt, bopt = _out_options(block_size, restart_interval, bits_per_key, bloom_reserved)
    tot = OutputTotals()

    def call(arena_p, acap, hp, bc, fp, tp, bp, vp_, fc, kp, kc, up):
        rc = L.lv_compact_output_host(pbuf if pn or pb else None, pn, arr.ctypes.data if arr.size else None,
                                      order.ctypes.data if order.size else None, ctypes.byref(mt), op_cap,
                                      ctypes.byref(opt) if opt else None, ctypes.byref(bopt) if bopt else None,
                                      max_file_bytes, first_number, level, images_off, arena_p, acap, hp, bc, fp, tp, bp,
                                      vp_, fc, kp, kc, up, ctypes.byref(tot))
        if rc != 0:
            raise LvError(f"lv_compact_output_host: {rc}")
        return {n: int(getattr(tot, n)) for n in OUT_TOTALS}

    if sizing or None in (arena_cap, block_cap, files_cap, bound_cap):
        vf = ctypes.create_string_buffer(64) if version_files else None  # (non-NULL: the bound bytes are counted)
        t = call(None, 0, None, 0, None, None, None, vf, 0, None, 0, None)
        if sizing:
            return HostOutput(totals=t)
        arena_cap = t["arena_bytes"] if arena_cap is None else arena_cap
        block_cap = t["data_blocks"] if block_cap is None else block_cap
        files_cap = t["files"] if files_cap is None else files_cap
        bound_cap = bound_used + t["bound_bytes"] if bound_cap is None else bound_cap
    extra = 3
    arena = np.full(arena_cap + guard, fill, dtype=np.uint8)
    hs = np.full(2 * (block_cap + extra * files_cap) + 8, fill * 0x0101010101010101, dtype=np.uint64)
    files = np.frombuffer(bytes([fill]) * (64 * (files_cap + 1)), dtype=OUT_FILE_DTYPE).copy()
    tables = np.full((files_cap + 1, 8), fill * 0x0101010101010101, dtype=np.uint64)
    blm = np.full((files_cap + 1, 8), fill * 0x0101010101010101, dtype=np.uint64)
    vfs = np.frombuffer(bytes([fill]) * (64 * (files_cap + 1)), dtype=FILE_DTYPE).copy()
    bounds = np.full(bound_cap + guard, fill, dtype=np.uint8)
    cur = ctypes.c_uint64(bound_used)
    t = call(arena.ctypes.data if arena_cap else None, arena_cap, hs.ctypes.data, block_cap, files.ctypes.data,
             tables.ctypes.data, blm.ctypes.data if blooms else None, vfs.ctypes.data if version_files else None,
             files_cap, bounds.ctypes.data, bound_cap, ctypes.byref(cur))
    return HostOutput(totals=t, arena=arena, arena_cap=arena_cap, handles=hs, block_cap=block_cap, files=files,
                      tables=tables, blooms=blm, version_files=vfs, files_cap=files_cap, bounds=bounds,
                      bound_cap=bound_cap, bound_used=int(cur.value))


class Output:
    """Outputs of output_device, CUDA tensors written asynchronously: arena_t
    (uint8, arena_cap bytes and the guard), handles_t (int64, block_cap + 3
    files_cap pairs and the guard), files_t / tables_t / blooms_t /
    version_files_t (uint8, 64 bytes per file and the guard; blooms_t and
    version_files_t may be None), bounds_t (uint8), used_t (int64[1], the
    cursor) and totals (int64[8], OUT_TOTALS).  tables_t, blooms_t,
    version_files_t and bounds_t are what lvgpu.version.open_device takes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._tot = None

    def sync(self, check: bool = True) -> dict:
        """Waits for the call; the totals as a dict.  Raises LvError naming the
        status bits if one is set (nothing was written) unless check is False."""
        if self._tot is None:
            import torch
            torch.cuda.synchronize(self.totals.device)
            self._tot = dict(zip(OUT_TOTALS, (int(v) for v in self.totals.cpu().numpy().view(np.uint64))))
            self._keep = None
        st = self._tot["status"]
        if st and check:
            names = "|".join(n for b, n in OUT_STATUS.items() if st & b)
            raise LvError(f"lv_compact_output_device: status {names} (totals {self._tot})")
        return self._tot

    def files(self):
        """d_files[0, files) as an OUT_FILE_DTYPE array (synchronises)."""
        n = self.sync()["files"]
        return self.files_t[: 64 * n].cpu().numpy().view(OUT_FILE_DTYPE).copy()

    def image(self, k) -> bytes:
        f = self.files()[k]
        return self.arena_t[int(f["file_off"]): int(f["file_off"] + f["file_bytes"])].cpu().numpy().tobytes()

    def file_handles_view(self, k):
        """File k's handle pairs as an (n, 2) int64 CUDA tensor for verify_blocks."""
        f = self.files()[k]
        at, n = int(f["first_handle"]), int(f["data_blocks"]) + self.extra
        return self.handles_t[2 * at: 2 * (at + n)].view(n, 2)


def output_device(table, max_file_bytes=DEFAULT_MAX_FILE_BYTES, *, bits_per_key=None, block_size=None,
                  restart_interval=None, first_number=1, level=1, images_off=0, arena_t=None, arena_cap=None,
                  block_cap=None, files_cap=None, bounds_t=None, bound_cap=None, used_t=None, blooms=True,
                  version_files=True, workspace=None, stream=None, fill=None, guard: int = 0, flags: int = 0,
                  bloom_reserved: int = 0):
    """lv_compact_output_device over a lvgpu.memtable.Table (a memtable build's,
    Scanned.memtable() or a Filtered): its payload, ops, order and totals, read
    on the device.  arena_cap defaults to output_arena_bound, block_cap and
    files_cap to op_cap, bound_cap to the payload's bytes + 16 op_cap.  arena_t
    (with images_off: where the run goes inside a caller's images buffer) /
    bounds_t / used_t continue a caller's buffers; fill, a byte value,
    initialises every output it allocates with it first and guard allocates that
    many more bytes behind each (canaries).  Returns an Output; asynchronous on
    `stream`."""
    import torch
    from . import _dev_ptr, _stream_ptr
    L = _bind_output()
    dev = table.payload.device
    op_cap = int(table.op_cap)
    opt, bopt = _out_options(block_size, restart_interval, bits_per_key, bloom_reserved)
    if arena_cap is None:
        arena_cap = output_arena_bound(table.payload.numel(), op_cap, bits_per_key)
    block_cap = op_cap if block_cap is None else block_cap
    files_cap = min(op_cap, 1 << 20) if files_cap is None else files_cap
    bound_cap = table.payload.numel() + 16 * op_cap if bound_cap is None else bound_cap
    if workspace is None:
        need = L.lv_compact_output_workspace_bytes(op_cap, block_cap, files_cap)
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

    def alloc(nbytes, dtype=torch.uint8):
        nbytes = (max(nbytes, 16) + guard + 15) & ~15
        t = (torch.empty(nbytes, dtype=torch.uint8, device=dev) if fill is None
             else torch.full((nbytes,), fill, dtype=torch.uint8, device=dev))
        return t.view(dtype)
    arena = alloc(arena_cap) if arena_t is None else arena_t[images_off:]
    handles_t = alloc(16 * (block_cap + 3 * files_cap), torch.int64)
    files_t, tables_t = alloc(64 * files_cap), alloc(64 * files_cap)
    blooms_t = alloc(64 * files_cap) if blooms else None
    vfiles_t = alloc(64 * files_cap) if version_files else None
    if bounds_t is None:
        bounds_t = alloc(bound_cap)
    if used_t is None:
        used_t = torch.zeros(1, dtype=torch.int64, device=dev)
    totals = torch.empty(len(OUT_TOTALS), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):  # the C call runs on the current device
        rc = L.lv_compact_output_device(_dev_ptr(table.payload, "payload") if table.payload.numel() else None,
                                        table.payload.numel(), _dev_ptr(table.ops_t, "ops") if op_cap else None,
                                        _dev_ptr(table.order_t, "order") if op_cap else None,
                                        _dev_ptr(table.totals, "mt_totals"), op_cap, ctypes.byref(opt) if opt else None,
                                        ctypes.byref(bopt) if bopt else None, max_file_bytes, first_number, level,
                                        images_off, _dev_ptr(arena, "arena") if arena_cap else None, arena_cap,
                                        _dev_ptr(handles_t, "handles"), block_cap, _dev_ptr(files_t, "files"),
                                        _dev_ptr(tables_t, "tables"), _dev_ptr(blooms_t, "blooms"),
                                        _dev_ptr(vfiles_t, "version_files"), files_cap, _dev_ptr(bounds_t, "bound_keys"),
                                        bound_cap, _dev_ptr(used_t, "bound_used"), _dev_ptr(totals, "totals"), flags,
                                        _dev_ptr(workspace, "workspace"), workspace.numel(), _stream_ptr(stream))
    if rc != 0:
        raise LvError(f"lv_compact_output_device: {lib().lv_last_error().decode()}")
    out = Output(arena_t=arena, arena_cap=arena_cap, handles_t=handles_t, block_cap=block_cap, files_t=files_t,
                 tables_t=tables_t, blooms_t=blooms_t, version_files_t=vfiles_t, files_cap=files_cap, bounds_t=bounds_t,
                 bound_cap=bound_cap, used_t=used_t, totals=totals, extra=3 if bits_per_key is not None else 2)
    out._keep = (table, workspace)
    return out
