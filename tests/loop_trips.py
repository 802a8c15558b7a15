"""How often the workgroups of a capped-grid kernel go round their grid-stride
loop, from the library's own launch arithmetic (lv_debug_launch_grid: the
functions the launchers call).  A kernel with `units` of work runs on
`grid` workgroups, each taking `per` units a trip, so workgroup w takes the
chunks w, w + grid, ... of ceil(units / per); the busiest one (workgroup 0)
makes ceil(chunks / grid) trips.  For the one-workgroup round loops (wb_tiles,
wal_dec_tiles) a trip is a round.  The units of each kernel are listed at
lv_debug_launch_grid in include/lvgpu/crc32c.h.

The GPU tests size their inputs with size_for() and assert trips() for the
device they run on, so a change of a launcher's cap fails them instead of
leaving them running one trip."""
import lvgpu


def grid_of(kernel, units, cus):
    """(grid, units per workgroup trip); raises for a name the library does not know."""
    g, per = lvgpu.launch_grid(kernel, units, cus)
    if units and not (g and per):
        raise KeyError(f"lv_debug_launch_grid does not know {kernel!r}")
    return g, per


def trips(kernel, units, cus):
    """The largest number of trips any workgroup (or wave) of `kernel` makes
    over `units` of work on `cus` compute units."""
    if units == 0:
        return 0
    g, per = grid_of(kernel, units, cus)
    chunks = -(-units // per)
    return -(-chunks // g)


def size_for(kernel, want_trips, cus, extra=0):
    """The smallest work size at which some workgroup makes `want_trips`
    trips, plus a ragged `extra` (which never takes trips away: the trip
    count does not fall as the work grows)."""
    lo, hi = 1, 1
    while trips(kernel, hi, cus) < want_trips:
        hi *= 2
        if hi > 1 << 48:
            raise ValueError(f"{kernel}: no size reaches {want_trips} trips")
    while lo < hi:  # trips() is monotone in units
        mid = (lo + hi) // 2
        if trips(kernel, mid, cus) >= want_trips:
            hi = mid
        else:
            lo = mid + 1
    return lo + extra


def device_cus(gpu):
    import torch
    return torch.cuda.get_device_properties(gpu).multi_processor_count


# The sizes tests/test_gpu_loop_trips.py (and the two resized
# test_more_blocks_than_compute_units) use: kernel -> (the kernel the input is
# sized for, the trips asked of that one, the ragged extra, the trips this
# kernel must make at that size).  tests/test_loop_trips.py holds every row to
# its trips at 256 compute units; the GPU tests assert them for their device.
# A kernel whose test adds to its size in its own way (ss_count: a full tile
# and a ragged one; hint_len_kernel: three strides) or rides on another
# module's input (sb_bloom_offsets: the table of test_gpu_positions64.py) has
# the smallest size of its trips here (the loop-trip audit).
PLAN = {
    "hash_kernel": ("hash_kernel", 3, 64 * 5 + 17, 3),
    "wb_emit": ("wb_emit", 3, 300, 3),
    "wb_count": ("wb_emit", 3, 300, 3),
    "wb_tiles": ("wb_emit", 3, 300, 8),
    "wal_frame_kernel": ("wal_frame_kernel", 3, 5, 3),
    "wal_unframe_kernel": ("wal_frame_kernel", 3, 5, 3),
    "wal_dec_reduce": ("wal_dec_reduce", 2, 1025, 2),
    "wal_dec_apply": ("wal_dec_reduce", 2, 1025, 2),
    "wal_dec_classify": ("wal_dec_reduce", 2, 1025, 2),
    "wal_dec_tiles": ("wal_dec_reduce", 2, 1025, 2),
    "sb_bloom_emit": ("sb_bloom_emit", 3, 7, 3),
    "sb_bloom_big": ("sb_bloom_emit", 3, 7, 3),
    "so_validate": ("so_validate", 2, 11, 2),
    "so_emit": ("so_validate", 2, 11 + 2, 2),  # its units are the handles: the blocks + 2
    "wal_unsort": ("wal_unsort", 2, 0, 2),
    "sb_bloom_offsets": ("sb_bloom_offsets", 2, 0, 2),
    "ss_count": ("ss_count", 2, 0, 2),
    "sst_blocks_kernel": ("sst_blocks_kernel", 2, 0, 2),
    "sb_carry": ("sb_carry", 2, 2517, 2),
    "ss_carry": ("sb_carry", 2, 2517, 2),
    "cf_carry": ("sb_carry", 2, 2517, 2),
    "combine_pieces_kernel": ("combine_pieces_kernel", 2, 903, 2),
    "hint_len_kernel": ("hint_len_kernel", 3, 300, 3),  # (the GPU test adds three strides: hint_len_shape)
}


def planned_size(kernel, cus):
    by, want, extra, _ = PLAN[kernel]
    return size_for(by, want, cus, extra)


# hint_len_kernel's loop has two levels: thread t of the grid's `stride`
# threads reads len[t + q * stride], four values of q in flight in a pass of
# the unrolled loop for as long as all four lie below n, the rest one at a time
# in the tail loop.
def hint_len_shape(cus, ragged=300):
    """(n, stride): two full trips of the unrolled loop, then three strides and
    `ragged` lengths more, so thread t makes two unrolled passes and three
    tail iterations, and the threads t < ragged a third unrolled pass and no
    tail."""
    n = size_for("hint_len_kernel", 3, cus) - 1  # two full trips of every workgroup
    grid, per = grid_of("hint_len_kernel", n, cus)
    stride = grid * per // 4
    assert n == 8 * stride and 0 < ragged < stride
    n += 3 * stride + ragged
    assert grid_of("hint_len_kernel", n, cus) == (grid, per)
    return n, stride


def hint_len_place(i, n, stride):
    """Where the loop reads len[i]: ("unrolled", pass, slot) or ("tail",
    iteration, 0), with the passes the reading thread makes."""
    t, q = i % stride, i // stride
    passes = max(0, -(-(n - t - 3 * stride) // (4 * stride)))
    return ("unrolled", q // 4, q % 4) if q // 4 < passes else ("tail", q - 4 * passes, 0)
