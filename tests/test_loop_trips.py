"""tests/loop_trips.py against a brute-force walk of the grid-stride loop, and
the sizes the loop-trip GPU tests use against the launchers' caps: needs no
GPU (lv_debug_launch_grid is host arithmetic)."""
import pytest

import lvgpu
import loop_trips as LT

CUS = [1, 64, 256, 304]


def _brute_trips(units, grid, per):
    """for (u = wg; u < total; u += grid) over every workgroup: the most trips."""
    total = -(-units // per)
    most = 0
    for wg in range(grid):
        n, u = 0, wg
        while u < total:
            n += 1
            u += grid
        most = max(most, n)
        if wg > 2 and n < most:  # workgroups past the ragged end only make fewer
            break
    return most


def test_query_knows_its_names_and_no_others():
    names = lvgpu.launch_grid_names()
    assert len(names) == len(set(names)) >= 18
    for k in names:
        g, per = lvgpu.launch_grid(k, 1000, 256)
        assert g >= 1 and per >= 1, k
        assert lvgpu.launch_grid(k, 1000, 0) == (0, 0), k
    assert lvgpu.launch_grid("no_such_kernel", 1000, 256) == (0, 0)
    assert lvgpu.lib().lv_debug_launch_grid(None, 1000, 256, None) == 0
    assert lvgpu.lib().lv_debug_launch_grid(b"hash_kernel", 1000, 256, None) == 4  # NULL per-trip pointer
    with pytest.raises(KeyError):
        LT.trips("no_such_kernel", 5, 256)
    assert set(LT.PLAN) == set(names)


@pytest.mark.parametrize("cus", CUS)
def test_helpers_match_a_walk_of_the_loop(cus):
    for k in lvgpu.launch_grid_names():
        assert LT.trips(k, 0, cus) == 0
        for want in (1, 2, 3):
            s = LT.size_for(k, want, cus)
            assert LT.trips(k, s, cus) == want, (k, want)
            if s > 1:
                assert LT.trips(k, s - 1, cus) == want - 1 or (want == 1 and s == 1), (k, want)
            for units in {s, s + 1, s + 777, max(1, s - 1), 2 * s + 13}:
                g, per = LT.grid_of(k, units, cus)
                assert LT.trips(k, units, cus) == _brute_trips(units, g, per), (k, units)
            assert LT.size_for(k, want, cus, 41) == s + 41
            assert LT.trips(k, s + 41, cus) >= want


def test_the_known_caps_at_256_compute_units():
    """The thresholds the audit table in DESIGN.md states."""
    second = {"hash_kernel": 8 * 256 * 256, "wb_count": 16 * 256 * 256, "wb_emit": 16 * 256 * 256,
              "wb_tiles": 1024 * 256, "wal_frame_kernel": 8 * 256, "wal_unframe_kernel": 8 * 256,
              "wal_dec_classify": 16 * 256 * 256, "wal_dec_reduce": 8 * 256 * 1024, "wal_dec_apply": 8 * 256 * 1024,
              "wal_dec_tiles": 256 * 1024, "wal_unsort": 256 * 1024, "sb_bloom_emit": 4096, "sb_bloom_big": 4096,
              "sb_bloom_offsets": 1024 * 256, "so_validate": 2048 * 256, "so_emit": 2048 * 256,  # (so_emit: 524,286 blocks + 2)
              "ss_count": 4096 * 1024, "sst_blocks_kernel": 256 * 16, "sb_carry": 65536, "ss_carry": 65536,
              "cf_carry": 65536, "combine_pieces_kernel": 4096,
              "hint_len_kernel": 4 * 256 * 1024}  # (a thread's second length: above 4 * 256 * 256)
    assert set(second) == set(lvgpu.launch_grid_names())
    for k, last_single in second.items():
        assert LT.size_for(k, 2, 256) == last_single + 1, k


def _walk_hint_len(n, grid):
    """hint_len_kernel's two loops as written (csrc/classes.hip), for every
    thread of the grid: {index: place}, and the most passes (unrolled ones,
    and one more where a tail follows) any thread makes."""
    stride, seen, most = grid * 256, {}, 0
    for t in range(stride):
        i, u = t, 0
        while i + 3 * stride < n:
            for slot in range(4):
                assert i + slot * stride not in seen
                seen[i + slot * stride] = ("unrolled", u, slot)
            i, u = i + 4 * stride, u + 1
        k = 0
        while i < n:
            assert i not in seen
            seen[i] = ("tail", k, 0)
            i, k = i + stride, k + 1
        most = max(most, u + (k > 0))
    return seen, most


@pytest.mark.parametrize("cus", [1, 2])
def test_hint_len_grid_against_a_walk_of_its_loops(cus):
    """The grid query, trips() and hint_len_place() against the kernel's own
    two-level loop, at the shape the GPU test uses and around its edges."""
    n0, stride = LT.hint_len_shape(cus, ragged=300)
    assert stride == 4 * cus * 256 and n0 == 11 * stride + 300
    for n in (1, 255, 1024, 1025, 3 * stride, 3 * stride + 1, 4 * stride, 4 * stride + 1, 8 * stride, n0, n0 + 4 * stride):
        grid, per = LT.grid_of("hint_len_kernel", n, cus)
        assert per == 1024 and grid == min(4 * cus, -(-n // 1024))
        seen, most = _walk_hint_len(n, grid)
        assert sorted(seen) == list(range(n))  # every length read, and once
        assert LT.trips("hint_len_kernel", n, cus) == most, n
        if grid * 256 == stride:
            for i in set(range(0, n, 97)) | {n - 1}:
                assert LT.hint_len_place(i, n, stride) == seen[i], (n, i)
    seen, _ = _walk_hint_len(n0, 4 * cus)
    at = lambda t: [seen[t + q * stride] for q in range(12) if t + q * stride < n0]
    two_and_three = [("unrolled", u, s) for u in (0, 1) for s in range(4)] + [("tail", k, 0) for k in range(3)]
    assert at(300) == at(stride - 1) == two_and_three
    assert at(0) == at(299) == [("unrolled", u, s) for u in (0, 1, 2) for s in range(4)]


@pytest.mark.parametrize("kernel", sorted(LT.PLAN))
def test_planned_sizes_take_their_trips(kernel):
    by, want, _, need = LT.PLAN[kernel]
    n = LT.planned_size(kernel, 256)
    assert LT.trips(kernel, n, 256) >= need, (kernel, n)
    for cus in CUS:  # the kernel an input is sized for takes its trips on any device
        assert LT.trips(by, LT.planned_size(kernel, cus), cus) >= want, (kernel, cus)
