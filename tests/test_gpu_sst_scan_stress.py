"""lv_sst_scan_device against the Python model over 200 seeded random tables:
alphabets of 2, 16 and 256 symbols, 0 to 3,000 entries, random block sizes and
restart intervals, the image and the arena at random alignments, exact and
generous capacities; every third trial appends a second table to the first."""
import numpy as np
import pytest

import memtable_cases as M
import sst_build_cases as S
import sst_scan_cases as C
from memtable_cases import make_table

pytestmark = pytest.mark.gpu

TRIALS, PER_TEST = 200, 20


def random_items(rng, n, alphabet, maxlen, seqs):
    """M.random_items; with 256 symbols (its symbols start at 97, so it stops
    at 159) the same shape over every byte value."""
    if alphabet <= 159:
        return M.random_items(rng, n, alphabet=alphabet, maxlen=maxlen, seqs=seqs)
    draw = lambda ln: bytes(rng.integers(0, 256, size=ln, dtype=np.uint16).astype(np.uint8))
    prefixes = [draw(int(rng.integers(9, 31))) for _ in range(4)]
    items = []
    for i in range(n):
        key = (prefixes[int(rng.integers(4))] if rng.random() < 0.6 else b"") + draw(int(rng.integers(0, maxlen)))
        typ = 0 if rng.random() < 0.25 else 1
        items.append((key, M.tag(int(rng.integers(1, seqs)), typ), b"" if typ == 0 else b"val%d" % (i % 7)))
    return items


def random_image(rng):
    n = int(rng.choice([0, 1, 17, 150, 600, 3000], p=[0.05, 0.1, 0.3, 0.35, 0.15, 0.05]))
    items = random_items(rng, n, int(rng.choice([2, 16, 256])), int(rng.choice([3, 12, 40])), int(rng.choice([2, 6, 50])))
    bs, ri = int(rng.choice([1, 7, 64, 300, 4096])), int(rng.choice([1, 2, 16, 1024]))
    payload, ops = make_table(items)
    return S.model_build(payload, ops, bs, ri)[0], (n, bs, ri)


@pytest.mark.parametrize("first", range(0, TRIALS, PER_TEST))
def test_random_tables(gpu, first):
    import torch
    for trial in range(first, first + PER_TEST):
        rng = np.random.default_rng(7000 + trial)
        images = [random_image(rng) for _ in range(2 if trial % 3 == 0 else 1)]
        shift, ashift, slack = int(rng.integers(0, 16)), int(rng.integers(0, 16)), int(rng.choice([1, 1, 3]))
        tag_ = f"trial {trial} {[i[1] for i in images]}"
        if len(images) == 1:
            C.check_image(torch, gpu, images[0][0], shift=shift, arena_shift=ashift, slack=slack, tag_=tag_)
            continue
        tabs = [C.open_table(img) for img, _ in images]
        fulls = [C.model_scan(img, t)[0] for (img, _), t in zip(images, tabs)]
        acap = sum(f["table_bytes"] for f in fulls) * slack
        ocap = sum(f["table_entries"] for f in fulls) * slack
        bcap = max(max(t["data_blocks"] for t in tabs), 1)
        op0, own0 = C.open_on(torch, gpu, images[0][0], shift)
        w0 = C.model_scan(images[0][0], tabs[0], arena_cap=acap, op_cap=ocap, block_cap=bcap)
        s0 = C.run_scan(torch, gpu, op0, arena_cap=acap, op_cap=ocap, block_cap=bcap, arena_shift=ashift)
        op1, own1 = C.open_on(torch, gpu, images[1][0], ashift)
        w1 = C.model_scan(images[1][0], tabs[1], w0[0], arena_cap=acap, op_cap=ocap, block_cap=bcap)
        s1 = C.run_scan(torch, gpu, op1, s0, arena_cap=acap, op_cap=ocap, block_cap=bcap)
        assert s0.sync(check=False) == w0[0], tag_
        C.check_scan(s1, w1, prev_want=(w0[1], w0[2]), tag_=tag_)
