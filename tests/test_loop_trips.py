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
              "cf_carry": 65536, "combine_pieces_kernel": 4096}
    assert set(second) == set(lvgpu.launch_grid_names())
    for k, last_single in second.items():
        assert LT.size_for(k, 2, 256) == last_single + 1, k


@pytest.mark.parametrize("kernel", sorted(LT.PLAN))
def test_planned_sizes_take_their_trips(kernel):
    by, want, _, need = LT.PLAN[kernel]
    n = LT.planned_size(kernel, 256)
    assert LT.trips(kernel, n, 256) >= need, (kernel, n)
    for cus in CUS:  # the kernel an input is sized for takes its trips on any device
        assert LT.trips(by, LT.planned_size(kernel, cus), cus) >= want, (kernel, cus)
