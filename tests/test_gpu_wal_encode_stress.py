"""Seeded stress of lv_wal_encode_device against oracle/wal_oracle.py's Writer:
300 small batches with record lengths aimed at the block edges, random
dest_length and random alignments of both buffers."""
import numpy as np
import pytest

from wal_encode_cases import B, H, encode_checked, first_diff, oracle_encode

pytestmark = pytest.mark.gpu

TRIALS = 300


def _trial_records(rng):
    n = int(rng.integers(1, 65))
    lens = []
    for _ in range(n):
        if rng.random() < 0.5:  # skewed: mostly short
            lens.append(int(rng.integers(0, 1 << int(rng.integers(0, 13)))))
        else:  # a fragment's worth, or a multiple of it, give or take 3
            lens.append(max(0, int(rng.integers(1, 3)) * (B - H) + int(rng.integers(-3, 4))))
    # at most ~6 long records per trial keeps a trial's log near 200 KiB
    long_idx = [i for i, x in enumerate(lens) if x > 4096]
    for i in long_idx[6:]:
        lens[i] = lens[i] % 19
    return lens


def test_seeded_trials(gpu):
    import torch
    # one arena of random bytes; records are slices of it at random offsets
    arena = np.random.default_rng(99).integers(0, 256, size=4 * B, dtype=np.uint8).tobytes()
    for seed in range(TRIALS):
        rng = np.random.default_rng(seed)
        ln = np.array(_trial_records(rng), dtype=np.uint64)
        off = np.array([int(rng.integers(0, len(arena) - int(x) + 1)) for x in ln], dtype=np.uint64)
        dest_length = int(rng.integers(0, 2 * B))
        recs = [arena[int(o):int(o + x)] for o, x in zip(off, ln)]
        got, guards_ok = encode_checked(torch, gpu, arena, off, ln, dest_length, out_shift=int(rng.integers(0, 16)),
                                        pay_shift=int(rng.integers(0, 16)))
        diff = first_diff(got, oracle_encode(recs, dest_length))
        assert diff is None, f"seed {seed}: {diff}"
        assert guards_ok, f"seed {seed}: bytes outside d_out[0, out_len) were written"
