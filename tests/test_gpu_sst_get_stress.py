"""lv_sst_open_device / lv_sst_get_device against the Python model over a few
hundred seeded random tables: keys over small alphabets behind shared stems,
random block sizes and restart intervals, the image at a random alignment."""
import numpy as np
import pytest

import memtable_cases as M
import sst_build_cases as S
import sst_get_cases as G
from memtable_cases import make_table

pytestmark = pytest.mark.gpu

TRIALS, PER_TEST = 300, 30


@pytest.mark.parametrize("first", range(0, TRIALS, PER_TEST))
def test_random_tables(gpu, first):
    import torch
    for trial in range(first, first + PER_TEST):
        rng = np.random.default_rng(4000 + trial)
        n = int(rng.choice([1, 2, 17, 60, 150]))
        items = M.random_items(rng, n, alphabet=int(rng.integers(2, 5)), maxlen=int(rng.choice([3, 12, 40])),
                               seqs=int(rng.choice([2, 6, 50])))
        bs, ri = int(rng.choice([1, 7, 64, 300, 4096])), int(rng.choice([1, 2, 16, 1024]))
        payload, ops = make_table(items)
        image, _, _ = S.model_build(payload, ops, bs, ri)
        qs = G.queries_for(image, payload, ops)
        qs = qs[:: max(len(qs) // 150, 1)]
        G.check_image(torch, gpu, image, qs, shifts=(int(rng.integers(0, 16)),), tag_=f"trial {trial} bs={bs} ri={ri}")
