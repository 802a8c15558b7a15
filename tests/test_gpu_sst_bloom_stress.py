"""Seeded random small tables through lv_memtable_build_device and
lv_sst_build_bloom_device against the host twin, byte for byte, and for every
fifth one the filter's open and the filtered gets against the host twins:
0-80 entries over small alphabets, block sizes from one entry per block to one
block per table, every restart interval class and bits per key from 1 to 64."""
import random

import numpy as np
import pytest

import lvgpu.memtable as MT
import lvgpu.table as T
import memtable_cases as M
import sst_bloom_cases as B
import sst_get_cases as G
from memtable_cases import MAX_SEQUENCE, make_table

pytestmark = pytest.mark.gpu

TRIALS = 300


def test_random_tables(gpu):
    import torch
    filters = filtered = 0
    for seed in range(TRIALS):
        rng = random.Random(900 + seed)
        nrng = np.random.default_rng(900 + seed)
        items = M.random_items(nrng, rng.randrange(0, 81), alphabet=rng.choice([2, 4, 26]), maxlen=rng.choice([4, 12, 40]),
                               seqs=rng.choice([3, 50]))
        items = [(k, t, v * rng.choice([1, 1, 30])) for k, t, v in items]
        bs = rng.choice([1, 32, 64, 300, 2048, 4096, 1 << 20])
        ri = rng.choice([1, 2, 3, 16, 1024])
        bpk = rng.choice([1, 5, 10, 10, 17, 64])
        payload, ops = make_table(items, [rng.randrange(0, 4) for _ in items])
        order, mt = MT.build_host(payload, ops)
        want = T.build_bloom_host(payload, ops, order, mt, bpk, bs, ri)
        what = f"seed {seed}: {len(ops)} ops, block_size {bs}, interval {ri}, bits_per_key {bpk}"
        built = B.run_device(torch, gpu, payload, ops, bpk, bs, ri, shift=seed % 16, want=want)
        B.compare_device(built, want, what)
        filters += want[3]["filters"]
        if seed % 5 or not items:
            continue
        image = want[0]
        keys = sorted({k for k, _, _ in items})
        queries = [(k, MAX_SEQUENCE) for k in keys] + [(k + b"?", MAX_SEQUENCE) for k in keys] + [(k[:-1], 7) for k in keys]
        table, bloom, wants = B.host_answers(image, queries)
        op, bloom_t, owner = B.open_both(torch, gpu, image, shift=seed % 7)
        qk, off, ln, sq, _ = G.pack_queries(queries, bad_query=False)
        got = B.run_get(torch, gpu, op, bloom_t, qk, off, ln, sq)
        assert T.bloom_dict(bloom_t) == bloom and bloom["present"] == 1, what
        assert B.result_dicts(got) == wants, what
        filtered += sum(w["reserved"] for w in wants)
    assert filters > TRIALS and filtered > 1000  # not hollow: more than a filter a table, rejected queries
