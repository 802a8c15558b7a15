"""Seeded stress of lv_compact_filter_device against the Python model
(tests/compact_cases.py): STRESS_TRIALS sorted tables of 0-4,000 entries from
random_items over few keys and sequences, so that groups are long, now and then
with an unparsed type byte, a random snapshot, with and without
LV_COMPACT_BASE_LEVEL and a few ranges cut from the keys, packed or gapped, at
every payload alignment, over a dirty workspace.  d_order_out, both totals and
every canary are compared with the model.  (tests/test_compact.py checks that
the trials are not hollow.)"""
import pytest

from compact_cases import STRESS_TRIALS, check_device, stress_trial

CHUNK = 25


@pytest.mark.gpu
@pytest.mark.parametrize("first", range(0, STRESS_TRIALS, CHUNK))
def test_seeded_trials(gpu, first):
    import torch
    for seed in range(first, first + CHUNK):
        payload, ops, order, mt, S, ranges, flags = stress_trial(seed)
        try:
            cap = None if seed % 3 else 2 * len(ops) + 5
            check_device(torch, gpu, payload, ops, order, mt, S, ranges, flags, shift=seed % 16, op_cap=cap,
                         tag_=f"seed {seed}")
        except AssertionError:
            print(f"stress trial failed: seed {seed}, {len(ops)} ops, S {S}, flags {flags}, ranges {ranges}")
            raise
