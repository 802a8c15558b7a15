"""GPU parity of the uniform-block kernel's positioned last batch and XOR join
(crc32c_blocks_kernel: lvk::carry_finish<true>, lvk::join_group).  On a
block's last batch the fourth slice step reads region B of the blocks image,
whose eight copies hold different shifts, so the lanes of a sub-group end at
one point and join by XOR; the few partials left are shifted from the image's
combine slots.  Everything is bit-exact against the CPU oracle: every group
size, first batch = last batch, masked groups of a partial wave, the round
wrap, the 16-round flush of the result staging, seeds and masking, padded
strides, the long-block split's paths and the gathered walk."""
import numpy as np
import pytest

import lvgpu
import wal_oracle as W

pytestmark = pytest.mark.gpu

GROUPS = [1, 4, 16, 64]
NBS = [1, 2, 3, 5]  # batches per block; 1: the first batch is the last
NS = [1, 2, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, gpu


@pytest.fixture(scope="module")
def arena(torch_dev):
    """One payload for the small cases: (device tensor, host bytes)."""
    torch, dev = torch_dev
    t = torch.empty(max(NS) * (64 * max(GROUPS) * max(NBS) + 64) + 64, dtype=torch.uint8, device=dev)
    lvgpu.fill_splitmix(t, 0, 0x10E5)
    torch.cuda.synchronize()
    return t, t.cpu().numpy().tobytes()


def oracle_batch(arena: bytes, off, ln, seed, masked):
    a = np.frombuffer(arena, dtype=np.uint8)
    o = np.ascontiguousarray(off, dtype=np.uint64)
    n = np.ascontiguousarray(ln, dtype=np.uint32)
    s = None if seed is None else np.ascontiguousarray(seed, dtype=np.uint32)
    out = np.zeros(o.size, dtype=np.uint32)
    W.lib().oracle_batch(a.ctypes.data, o.ctypes.data, n.ctypes.data, None if s is None else s.ctypes.data,
                         out.ctypes.data, o.size, 1 if masked else 0)
    return out


def _seeds(torch, dev, rng, n, seeded):
    if not seeded:
        return None, None
    seeds = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    return seeds, torch.from_numpy(seeds.view(np.int32)).to(dev)


def _check_strided(torch, dev, t, host, n, blen, stride, seeded, group):
    """n blocks of blen bytes at `stride` in t (host: its bytes) through
    lv_crc32c_batch_strided, seeded calls masked, against the oracle.
    Returns the kernel the call launched."""
    seeds, sd = _seeds(torch, dev, np.random.default_rng(n * 31 + blen), n, seeded)
    out = lvgpu.batch_strided(t, stride, blen, n, seed=sd, masked=seeded, group=group)
    kern = lvgpu.last_kernel()
    torch.cuda.synchronize()
    want = oracle_batch(host, np.arange(n, dtype=np.uint64) * stride, np.full(n, blen, np.uint32), seeds, seeded)
    got = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want), (n, blen, stride, seeded, group, kern, np.flatnonzero(got != want)[:8])
    return kern


def _fresh(torch, dev, nbytes, fill):
    t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lvgpu.fill_splitmix(t, 0, fill)
    torch.cuda.synchronize()
    return t, t.cpu().numpy().tobytes()


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("group", GROUPS)
def test_forced_groups(torch_dev, arena, group, seeded):
    """Blocks of 64 G nb bytes, contiguous and at a stride 64 bytes wider:
    partial sub-groups of a wave are masked, whole waves and workgroups are
    not, 257 blocks span several workgroups."""
    torch, dev = torch_dev
    t, host = arena
    for nb in NBS:
        blen = 64 * group * nb
        for n in NS:
            for stride in (blen, blen + 64):
                kern = _check_strided(torch, dev, t, host, n, blen, stride, seeded, group)
                assert kern == "crc32c_blocks_kernel<%d>" % group


@pytest.mark.parametrize("group", GROUPS)
def test_round_wrap(torch_dev, group):
    """Five groups more than one pass of the grid holds: a few waves walk a
    second round, whose join must see only its own block.  Two batches per
    block, seeded and masked."""
    torch, dev = torch_dev
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    n = cus * 16 * (64 // group) + 5
    blen = 64 * group * 2
    t, host = _fresh(torch, dev, n * blen + 64, 0x10E6 + group)
    assert _check_strided(torch, dev, t, host, n, blen, blen, True, group) == "crc32c_blocks_kernel<%d>" % group


def test_sixteen_round_flush(torch_dev):
    """1 KiB blocks (first batch = last batch) on the G = 16 kernel, a few
    more than 16 rounds of the grid: every wave fills its 64 result slots,
    stores them, and some start a 17th round."""
    torch, dev = torch_dev
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    n = 16 * cus * 64 + 5
    t, host = _fresh(torch, dev, n * 1024 + 64, 0x10E7)
    assert _check_strided(torch, dev, t, host, n, 1024, 1024, True, 16) == "crc32c_blocks_kernel<16>"


def _split_kernel(n, blen, cus):
    """The kernel of lvh::uniform_plan's long-block split (the rule
    tests/test_abi.py::_uniform_plan restates)."""
    want, ps = 4 * cus * 16, 0
    while (n << ps) < want and ps < 12:
        s2 = 2 << ps
        if blen % s2 or (blen // s2) % 1024 or blen // s2 < 4096:
            break
        ps += 1
    assert ps > 0
    if (1 << ps) <= 16 and (n << ps) <= 64 * cus:
        return "crc32c_blocks_kernel<16,pieces,fused>"
    return "crc32c_blocks_kernel<16,pieces>+combine_pieces_" + ("wg_kernel" if ps >= 11 else "kernel")


# 8 x 64 KiB: 16 pieces per block, one round, joined in the walk.  300 x 64 KiB:
# 4,800 pieces -- joined in the walk where they fit one round of the grid
# (64 pieces per CU), by a second launch on a smaller device.  1 x 1 MiB: 256
# pieces, a second launch.  100 x 160 KiB: 32 pieces of five batches, the
# batch loop and a second launch.
SPLIT_CASES = [(8, 64 << 10), (300, 64 << 10), (1, 1 << 20), (100, 160 << 10)]


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("n,blen", SPLIT_CASES)
def test_long_block_split(torch_dev, n, blen, seeded):
    torch, dev = torch_dev
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    want_kern = _split_kernel(n, blen, cus)
    if (n, blen) == (8, 64 << 10):
        assert want_kern == "crc32c_blocks_kernel<16,pieces,fused>"
    if n in (1, 100):
        assert want_kern == "crc32c_blocks_kernel<16,pieces>+combine_pieces_kernel"
    t, host = _fresh(torch, dev, n * blen + 64, 0x10E8 + n)
    assert _check_strided(torch, dev, t, host, n, blen, blen, seeded, None) == want_kern


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("n,blen,kern", [(64, 4096, "crc32c_blocks_kernel<64,gather>"),
                                         (8, 64 << 10, "crc32c_blocks_kernel<16,pieces,fused,gather>")])
def test_gathered_walk(torch_dev, n, blen, kern, seeded):
    """lv_crc32c_batch_device_hint with HINT_UNIFORM | HINT_ALIGNED16:
    shuffled 16-B aligned starts with gaps."""
    torch, dev = torch_dev
    rng = np.random.default_rng(blen + seeded)
    gaps = rng.integers(0, 4, n) * 16
    starts = np.cumsum(gaps + blen) - blen
    offs = rng.permutation(starts).astype(np.uint64)
    lens = np.full(n, blen, dtype=np.uint32)
    a, host = _fresh(torch, dev, int(starts[-1]) + blen + 64, 0x10E9 + blen)
    seeds, sd = _seeds(torch, dev, rng, n, seeded)
    hint = lvgpu.hint_for(lens, offs)
    assert hint.uniform == lvgpu.HINT_UNIFORM | lvgpu.HINT_ALIGNED16
    out = lvgpu.batch_hint(a, torch.from_numpy(offs.astype(np.int64)).to(dev),
                           torch.from_numpy(lens.view(np.int32)).to(dev), hint, seed=sd, masked=seeded)
    got_kern = lvgpu.last_kernel()
    torch.cuda.synchronize()
    assert got_kern == kern
    want = oracle_batch(host, offs, lens, seeds, seeded)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
