"""Seeded stress of lv_write_batch_decode_device against the Python model
(tests/write_batch_cases.py): STRESS_TRIALS payloads of 1-3,000 records with 0,
1, a few or hundreds of ops, key and value lengths of 0, 1-30, around WB_WINDOW
and up to 64 KiB, about 5 % of the records corrupted (truncation, a flipped
byte, a wrong count), packed or gapped, at every payload alignment, over a
dirty workspace.  Every output is compared with the model."""
import pytest

import lvgpu.write_batch as WB
from write_batch_cases import STRESS_TRIALS, check, stress_trial

CHUNK = 25


def test_trials_are_not_hollow():
    """(No GPU.)  At least one trial in ten holds a wave-class record and one
    in ten a bad record."""
    flags = [stress_trial(seed, WB.WB_SMALL, WB.WB_WINDOW)[3:] for seed in range(STRESS_TRIALS)]
    assert sum(w for w, _ in flags) * 10 >= STRESS_TRIALS
    assert sum(b for _, b in flags) * 10 >= STRESS_TRIALS


@pytest.mark.gpu
@pytest.mark.parametrize("first", range(0, STRESS_TRIALS, CHUNK))
def test_seeded_trials(gpu, first):
    import torch
    for seed in range(first, first + CHUNK):
        payload, off, ln, _, _ = stress_trial(seed, WB.WB_SMALL, WB.WB_WINDOW)
        try:
            check(torch, gpu, payload, off, ln, shift=seed % 16, tag=f"seed {seed}")
        except AssertionError:
            print(f"stress trial failed: seed {seed}, {len(off)} records, {len(payload)} payload bytes")
            raise
