"""lv_wal_decode_workspace_bytes and the argument checks of
lv_wal_decode_device: everything about the device WAL Reader that needs no GPU."""
import ctypes
import os
import re
import subprocess

import pytest

import lvgpu
import lvgpu.wal as LW

INVALID = -1  # LV_ERR_INVALID


def test_decode_symbols_exported():
    names = lvgpu.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", lvgpu.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in ("lv_wal_decode_workspace_bytes", "lv_wal_decode_device"):
        assert n in names and n in syms, n


def test_decode_workspace_bytes():
    L = LW._bind()
    prev = 0
    for cap in [0, 1, 2, 100, 1023, 1024, 1025, 4681, 65536, 1 << 20, (1 << 20) + 1]:
        w = L.lv_wal_decode_workspace_bytes(cap)
        assert w >= prev and w % 16 == 0, cap
        # an event word and an output position per entry, three words per block
        assert w >= 24 * cap
        prev = w
    assert LW.decode_workspace_bytes(1000) == L.lv_wal_decode_workspace_bytes(1000)


def test_decode_constants_match_header():
    """The Python mirror's reason strings and status names are the header's."""
    with open(lvgpu.HEADER_PATH.replace("crc32c.h", "wal.h")) as f:
        text = f.read()
    drops = re.findall(r'#define LV_WAL_DROP_\w+ (\d+)u\s+/\* "([^"]+)" \*/', text)
    assert {int(k): v for k, v in drops} == LW.DROP_REASONS and len(drops) == 9
    status = dict(re.findall(r"#define LV_WAL_DECODE_(\w+_OVER) (\d+)u", text))
    assert {int(v): k for k, v in status.items()} == LW.DECODE_STATUS
    assert "#define LV_WAL_DECODE_NO_CHECKSUM 0x1u" in text and LW.DECODE_NO_CHECKSUM == 1


def test_decode_tile_matches_kernels():
    """lvgpu.wal.DECODE_TILE (the GPU tests sweep around its multiples) is the
    scan tile of csrc/wal_decode.hip."""
    with open(os.path.join(CSRC, "wal_decode.hip")) as f:
        text = f.read()
    threads = int(re.search(r"kDecThreads = (\d+);", text).group(1))
    per = int(re.search(r"kDecPer = (\d+);", text).group(1))
    assert "kDecTile = kDecThreads * kDecPer;" in text and LW.DECODE_TILE == threads * per


def test_decode_device_argument_checks():
    """Every argument error of lv_wal_decode_device is found on the host,
    before any device call: LV_ERR_INVALID and a message, with pointers that
    are never dereferenced and no GPU in the machine."""
    L = LW._bind()
    vp = ctypes.c_void_p
    cap, nbytes = 100, 4096
    wsb = L.lv_wal_decode_workspace_bytes(cap)
    err = lambda: lvgpu.lib().lv_last_error()

    def out(**kw):
        o = LW.DecodeOut()
        o.d_payload, o.payload_cap = 0x900000, nbytes
        o.d_rec_off, o.d_rec_len, o.d_rec_log_off, o.rec_cap = 0xA00000, 0xA10000, 0xA20000, cap
        o.d_rep_bytes, o.d_rep_log_off, o.d_rep_reason, o.rep_cap = 0xB00000, 0xB10000, 0xB20000, 2 * cap
        o.d_totals = 0xC00000
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(log=vp(0x100000), n=nbytes, hdr=vp(0x200000), crc=vp(0x300000), info=vp(0x400000), count=vp(0x500000),
             c=cap, o="default", flags=0, w=vp(0x4000000), wb=wsb):
        o = out() if o == "default" else o
        return L.lv_wal_decode_device(log, n, hdr, crc, info, count, c, ctypes.byref(o) if o is not None else None,
                                      flags, w, wb, None)

    # NULL pointers
    assert call(log=None) == INVALID and b"null" in err()
    assert call(hdr=None) == INVALID and b"null" in err()
    assert call(info=None) == INVALID and b"null" in err()
    assert call(crc=None) == INVALID and b"null" in err()
    assert call(count=None) == INVALID and b"null" in err()
    assert call(o=None) == INVALID and b"null" in err()
    assert call(w=None) == INVALID and b"workspace" in err()
    for field in ("d_payload", "d_rec_off", "d_rec_len", "d_rec_log_off", "d_totals"):
        assert call(o=out(**{field: None})) == INVALID and b"null" in err(), field
    # report arrays: all three or none, and none only with rep_cap == 0
    for field in ("d_rep_bytes", "d_rep_log_off", "d_rep_reason"):
        assert call(o=out(**{field: None})) == INVALID and b"report" in err(), field
    assert call(o=out(d_rep_bytes=None, d_rep_log_off=None, d_rep_reason=None)) == INVALID and b"rep_cap" in err()
    # workspace one byte short; misaligned
    assert call(wb=wsb - 1) == INVALID and b"workspace too small" in err()
    assert call(w=vp(0x4000008)) == INVALID and b"aligned" in err()
    # the log: 8-byte aligned
    assert call(log=vp(0x100004)) == INVALID and b"8-byte" in err()
    # d_payload inside / straddling the log, at either end
    assert call(o=out(d_payload=0x100000 + nbytes - 1)) == INVALID and b"overlap" in err()
    assert call(o=out(d_payload=0x100000 - nbytes + 1)) == INVALID and b"overlap" in err()
    assert call(o=out(d_payload=0x100000 + 8, payload_cap=16)) == INVALID and b"overlap" in err()
    # unknown flag bits
    assert call(flags=2) == INVALID and b"flag" in err()
    assert call(flags=0x80000001) == INVALID and b"flag" in err()
    # d_totals: 8-byte aligned
    assert call(o=out(d_totals=0xC00004)) == INVALID and b"d_totals" in err()
    # What passes the checks goes on to the device: with no GPU that is an
    # error of another kind, never LV_ERR_INVALID.  (NO_CHECKSUM with a NULL
    # d_crc; NULL report arrays with rep_cap == 0; a payload that ends where
    # the log starts.)
    import torch
    if not torch.cuda.is_available():
        assert call(crc=None, flags=LW.DECODE_NO_CHECKSUM) not in (0, INVALID)
        assert call(o=out(d_rep_bytes=None, d_rep_log_off=None, d_rep_reason=None, rep_cap=0)) not in (0, INVALID)
        assert call(o=out(d_payload=0x100000 - nbytes)) not in (0, INVALID)


CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "leveldb-rs_amd", "csrc")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_decode_kernels_do_not_spill():
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-munsafe-fp-atomics", "--cuda-device-only", "-c", "-o", os.devnull,
                        os.path.join(CSRC, "wal_decode.hip"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    spills, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name:
            spills[name] = int(m.group(1))
    for k in ("wal_dec_classify", "wal_dec_reduce", "wal_dec_tiles", "wal_dec_apply", "wal_unframe_kernel"):
        hits = {n: v for n, v in spills.items() if k in n}
        assert hits and all(v == 0 for v in hits.values()), (k, hits)
