"""Seeded stress of lv_memtable_build_device and lv_memtable_get_device against
the Python model (tests/memtable_cases.py): STRESS_TRIALS op tables of 0-6,000
ops with key lengths of 0-12, 13-64 and now and then up to 2,000 bytes, over
alphabets of 2, 16 and 256 symbols so that ties are frequent, random sequences
with repeats, packed or gapped, at every payload alignment, over a dirty
workspace.  d_order, the totals and a sample of lookups are compared with the
model."""
import pytest

import lvgpu.memtable as MT
from memtable_cases import MAX_SEQUENCE, STRESS_TRIALS, check, check_get, key_of, stress_trial

CHUNK = 25


def test_trials_are_not_hollow():
    """(No GPU.)  The trials hold tables of more than two tiles, keys beyond
    the sort prefix that tie in it, and repeated user keys."""
    big = ties = repeats = 0
    for seed in range(STRESS_TRIALS):
        payload, ops = stress_trial(seed)
        keys = [key_of(payload, o) for o in ops[:400]]
        big += len(ops) > 2 * MT.MT_TILE
        heads = [k[:MT.MT_PREFIX] for k in keys if len(k) > MT.MT_PREFIX]
        ties += len(set(heads)) < len(heads)
        repeats += len(set(keys)) < len(keys)
    assert big * 10 >= STRESS_TRIALS and ties * 4 >= STRESS_TRIALS and repeats * 4 >= STRESS_TRIALS


@pytest.mark.gpu
@pytest.mark.parametrize("first", range(0, STRESS_TRIALS, CHUNK))
def test_seeded_trials(gpu, first):
    import torch
    for seed in range(first, first + CHUNK):
        payload, ops = stress_trial(seed)
        try:
            cap = None if seed % 3 else 2 * len(ops) + 5
            table, order = check(torch, gpu, payload, ops, shift=seed % 16, op_cap=cap, tag_=f"seed {seed}")
            step = max(len(ops) // 40, 1)
            queries = []
            for o in ops[::step]:
                key, seq = key_of(payload, o), min(int(o["tag"]) >> 8, MAX_SEQUENCE)
                queries += [(key, seq), (key, max(seq - 1, 0)), (key + b"\x00", seq)]
            check_get(torch, gpu, table, payload, ops, order, queries, f"seed {seed}")
        except AssertionError:
            print(f"stress trial failed: seed {seed}, {len(ops)} ops, {len(payload)} payload bytes")
            raise
