"""Seeded random tables through lv_memtable_build_device and
lv_sst_build_device against the Python model, byte for byte: the memtable
stress generator's op tables (0-6,000 ops, key lengths 0-2,000 over alphabets
of 2, 16 and 256 symbols, repeated sequences, exact duplicates, packed or
gapped payloads) under block sizes from one entry per block to one block per
table and restart intervals from 1 to the largest."""
import random

import pytest

import memtable_cases as M
import sst_build_cases as C

pytestmark = pytest.mark.gpu

TRIALS = 30


def test_random_tables(gpu):
    import torch
    blocks = 0
    for seed in range(TRIALS):
        rng = random.Random(500 + seed)
        payload, ops = M.stress_trial(seed)
        bs = rng.choice([1, 32, 64, 300, 4096, 1 << 20])
        ri = rng.choice([1, 2, 3, 16, 100, 1024])
        built = C.run_device(torch, gpu, payload, ops, bs, ri, shift=seed % 16)
        C.compare_device(built, payload, ops, bs, ri, f"seed {seed}: {len(ops)} ops, block_size {bs}, interval {ri}")
        blocks += built.sync_totals()["data_blocks"]
    assert blocks > 1000  # not hollow
