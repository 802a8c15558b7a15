"""Seeded stress of lv_write_batch_encode_device against the Python model
(tests/write_batch_encode_cases.py): STRESS_TRIALS op tables of 1-3,000 records
with 0, 1, a few or hundreds of ops, key and value lengths of 0, 1-30, around
WE_WAVE_COPY and up to 64 KiB as windows of one pool (they overlap and repeat),
d_rec_op[0] of 0-3, sequences that wrap, every shift of source and
destination, over a dirty workspace.  Every fifth trial holds an empty record,
a long copy and a record above one tile (test_write_batch_encode.py checks
that without a GPU).  Every output byte and canary is compared."""
import pytest

import lvgpu.write_batch as WB
from write_batch_encode_cases import STRESS_TRIALS, check, stress_trial

CHUNK = 10


@pytest.mark.gpu
@pytest.mark.parametrize("first", range(0, STRESS_TRIALS, CHUNK))
def test_seeded_trials(gpu, first):
    import torch
    for seed in range(first, first + CHUNK):
        src, ops, rec_op, seq, lead, _ = stress_trial(seed, WB.WE_TILE, WB.WE_WAVE_COPY)
        try:
            r = check(torch, gpu, src, ops, rec_op, first_sequence=seq, out_shift=seed % 16,
                      src_shift=(3 * seed + 5) % 16, tag=f"seed {seed}")
            assert r.want[4]["status"] == 0
        except AssertionError:
            print(f"stress trial failed: seed {seed}, {len(rec_op) - 1} records, {len(ops) - lead} ops")
            raise
