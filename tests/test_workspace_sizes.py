"""The workspace sizes of the pipeline stages that take one, pinned.

A caller sizes its buffer with lv_*_workspace_bytes and the device entry point
cuts the same buffer into regions, so the numbers are part of what a caller
sees: a region that moves or grows changes them.  The expected values are
literals.  They were taken from the library as it was before each stage's
workspace came to be described once (one function that carves the regions,
run without a buffer to measure): that commit was built and these functions
called on it; they need no GPU.  Capacities lie either side of each stage's
tile (256 records, 512 and 1,024 entries, 1,024 blocks), and one lies beyond
each documented limit.

The three WAL stages (scan, decode, encode) came to it later, the same way:
their literals are from a build of the commit before their workspaces were
carved.  The scan's log sizes lie either side of one 32 KiB block and of one
workgroup's 64 blocks; decode and encode go on to the largest capacity one
call takes (entry and fragment indices are 32-bit) and, for decode, one past
it.

The WriteBatch encode and the two VersionEdit stages were pinned when their
device helpers moved into the shared headers: their literals are from a build
of the commit before that.  The VersionEdit encode takes four capacities; its
tile is 1,024 slots of capacity + 1 per table, so each capacity is also taken
alone either side of 1,023."""
import pytest

import lvgpu.memtable as MT
import lvgpu.table as T
import lvgpu.version_edit as VE
import lvgpu.wal as LW
import lvgpu.write_batch as WB

CAPS = (0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 100000)
BLOCK_CAPS = (0, 1, 1024, 1025)
MAX_CAP = 2**32 - 2        # op_cap / rec_cap of one call
MAX_BLOCK_CAP = 2**32 - 4  # block_cap of one call
MAX_ENCODE_ROWS = 2**30    # op_cap of a WriteBatch encode, a row capacity of a VersionEdit encode

WB_DECODE = (64, 112, 3152, 3152, 3184, 6224, 6224, 6272, 12384, 12384, 12432, 1203200)
MT_BUILD = (16, 80, 16336, 16400, 16464, 32720, 32784, 32848, 65488, 65552, 65616, 6400016)
# rows: op_cap in CAPS; columns: block_cap in BLOCK_CAPS
SST_BUILD = (
    (2100480, 2100512, 2120960, 2120992),
    (2108896, 2108928, 2129376, 2129408),
    (2124352, 2124384, 2144832, 2144864),
    (2124352, 2124384, 2144832, 2144864),
    (2124512, 2124544, 2144992, 2145024),
    (2139968, 2140000, 2160448, 2160480),
    (2139968, 2140000, 2160448, 2160480),
    (2140128, 2140160, 2160608, 2160640),
    (2171200, 2171232, 2191680, 2191712),
    (2171200, 2171232, 2191680, 2191712),
    (2179552, 2179584, 2200032, 2200064),
    (9006432, 9006464, 9026912, 9026944),
)
SST_SCAN = (
    (112, 240, 41120, 41200),
    (112, 240, 41152, 41200),
    (112, 4304, 45216, 45264),
    (112, 4336, 45216, 45296),
    (112, 4336, 45248, 45296),
    (112, 8400, 49312, 49360),
    (112, 8432, 49312, 49392),
    (112, 8432, 49344, 49392),
    (112, 16592, 57504, 57552),
    (112, 16624, 57504, 57616),
    (112, 16624, 57568, 57616),
    (112, 1601776, 1642688, 1642768),
)
WAL_LOG_BYTES = (0, 1, 32768, 32769, 64 * 32768, 64 * 32768 + 1)
# rows: log bytes in WAL_LOG_BYTES; columns: cap in CAPS
WAL_SCAN = (
    (3152, 3200, 9280, 9296, 9344, 15424, 15440, 15488, 27712, 27728, 27776, 2403152),
    (3680, 3728, 9808, 9824, 9872, 15952, 15968, 16016, 28240, 28256, 28304, 2403680),
    (3680, 3728, 9808, 9824, 9872, 15952, 15968, 16016, 28240, 28256, 28304, 2403680),
    (4192, 4240, 10320, 10336, 10384, 16464, 16480, 16528, 28752, 28768, 28816, 2404192),
    (36176, 36224, 42304, 42320, 42368, 48448, 48464, 48512, 60736, 60752, 60800, 2436176),
    (37728, 37776, 43856, 43872, 43920, 50000, 50016, 50064, 62288, 62304, 62352, 2437728),
)
WAL_DECODE = (32, 240, 6320, 6336, 6384, 12464, 12480, 12528, 24752, 24768, 24944, 2414144)
WAL_ENCODE = (2100320, 2100464, 2377792, 2378832, 2132336, 2163008, 2163024, 2164208, 2226752, 2226768, 2227952,
              8200416)
WB_ENCODE = (64, 128, 2160, 2160, 2176, 4208, 4208, 4224, 8304, 8304, 8320, 802416)
VE_DECODE = (32, 208, 22560, 22640, 22800, 45152, 45232, 45408, 90352, 90432, 90608, 8828192)
# rec_cap, file_cap, deleted_cap, pointer_cap = CAPS[i], CAPS[i + 1], CAPS[i + 2], CAPS[i + 3] (cyclic)
VE_ENCODE = (32896, 32896, 32896, 32896, 32896, 32896, 41120, 49312, 845504, 845504, 837280, 829088)


def test_write_batch_decode_workspace_bytes():
    assert tuple(WB.decode_workspace_bytes(c) for c in CAPS) == WB_DECODE
    # the size function knows no limit (lv_write_batch_decode_device refuses rec_cap > 2^32 - 2)
    assert WB.decode_workspace_bytes(MAX_CAP) == 51673825328
    assert WB.decode_workspace_bytes(MAX_CAP + 1) == 51673825344


def test_memtable_build_workspace_bytes():
    assert tuple(MT.build_workspace_bytes(c) for c in CAPS) == MT_BUILD
    assert MT.build_workspace_bytes(MAX_CAP) == 274877906832
    assert MT.build_workspace_bytes(MAX_CAP + 1) == 0


@pytest.mark.parametrize("fn, want, at_limit", [(T.build_workspace_bytes, SST_BUILD, 382388407376),
                                                 (T.scan_workspace_bytes, SST_SCAN, 240685940656)],
                         ids=["sst_build", "sst_scan"])
def test_sst_workspace_bytes(fn, want, at_limit):
    assert tuple(tuple(fn(c, b) for b in BLOCK_CAPS) for c in CAPS) == want
    assert fn(MAX_CAP, MAX_BLOCK_CAP) == at_limit
    assert fn(MAX_CAP + 1, 0) == 0
    assert fn(0, MAX_BLOCK_CAP + 1) == 0
    assert fn(MAX_CAP + 1, MAX_BLOCK_CAP + 1) == 0


def test_wal_scan_workspace_bytes():
    assert tuple(tuple(LW.scan_workspace_bytes(b, c) for c in CAPS) for b in WAL_LOG_BYTES) == WAL_SCAN


def test_wal_decode_workspace_bytes():
    assert tuple(LW.decode_workspace_bytes(c) for c in CAPS) == WAL_DECODE
    # the size function knows no limit (lv_wal_decode_device refuses scan_cap > 2^32 - 2)
    assert LW.decode_workspace_bytes(MAX_CAP) == 103683194880
    assert LW.decode_workspace_bytes(MAX_CAP + 1) == 103683194896


def test_wal_encode_workspace_bytes():
    assert tuple(LW.encode_workspace_bytes(f) for f in CAPS) == WAL_ENCODE
    assert LW.encode_workspace_bytes(2**32 - 1) == 257701193792  # the most fragments of one call


def test_write_batch_encode_workspace_bytes():
    assert tuple(WB.encode_workspace_bytes(c, c) for c in CAPS) == WB_ENCODE
    assert WB.encode_workspace_bytes(MAX_CAP, 0) == 64  # rec_cap takes no region
    assert WB.encode_workspace_bytes(0, MAX_ENCODE_ROWS) == WB.encode_workspace_bytes(MAX_CAP, MAX_ENCODE_ROWS) == 8615100480
    assert WB.encode_workspace_bytes(MAX_CAP + 1, 0) == 0
    assert WB.encode_workspace_bytes(0, MAX_ENCODE_ROWS + 1) == 0


def test_version_edit_decode_workspace_bytes():
    assert tuple(VE.decode_workspace_bytes(c) for c in CAPS) == VE_DECODE
    # the size function knows no limit (lv_version_edit_decode_device refuses rec_cap > 2^32 - 2)
    assert VE.decode_workspace_bytes(MAX_CAP) == 379165081456
    assert VE.decode_workspace_bytes(MAX_CAP + 1) == 379165081552


def test_version_edit_encode_workspace_bytes():
    n = len(CAPS)
    assert tuple(VE.encode_workspace_bytes(*(CAPS[(i + j) % n] for j in range(4))) for i in range(n)) == VE_ENCODE
    for k in range(4):  # each capacity alone: 1,023 + 1 slots fill its tile, 1,024 + 1 take a second
        assert [VE.encode_workspace_bytes(*(c if j == k else 0 for j in range(4))) for c in (1023, 1024)] == [32896, 41120]
    limits = (MAX_CAP, MAX_ENCODE_ROWS, MAX_ENCODE_ROWS, MAX_ENCODE_ROWS)
    assert VE.encode_workspace_bytes(*limits) == 60247007360
    for k in range(4):
        assert VE.encode_workspace_bytes(*(v + (j == k) for j, v in enumerate(limits))) == 0
