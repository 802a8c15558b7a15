"""GPU parity of the uniform-block kernel's carried fold (crc32c_blocks_kernel,
lvk::fold_batch_carry): a row's register is carried from batch to batch
through the jump table J = Shift_{16GU-12} and only a block's last batch reads
T.  Bit-exact against the CPU oracle at the smallest shapes where the chain
can go wrong: every batch count that puts the last batch in either ping-pong
slot, partial waves and workgroups, every group size, more than one round per
wave (a block's chain must end with the block), the long-block split's
one-round, fused and two-launch paths, and the gathered walk."""
import numpy as np
import pytest

import lvgpu
import wal_oracle as W

pytestmark = pytest.mark.gpu

NS = [1, 3, 5, 64, 65]  # partial waves (4 blocks per G = 16 wave) and a partial workgroup (64)


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, gpu


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


def _check_strided(torch, dev, n, blen, pad, seeded, group, fill):
    """n blocks of blen bytes at stride blen + pad (distinct splitmix
    payloads): lv_crc32c_batch_strided, seeded calls masked, vs the oracle.
    Returns the kernel the call launched."""
    stride = blen + pad
    t = torch.empty(stride * n + 64, dtype=torch.uint8, device=dev)
    lvgpu.fill_splitmix(t, 0, fill)
    seeds, sd = _seeds(torch, dev, np.random.default_rng(fill), n, seeded)
    out = lvgpu.batch_strided(t, stride, blen, n, seed=sd, masked=seeded, group=group)
    kern = lvgpu.last_kernel()
    torch.cuda.synchronize()
    want = oracle_batch(t.cpu().numpy().tobytes(), np.arange(n, dtype=np.uint64) * stride,
                        np.full(n, blen, np.uint32), seeds, seeded)
    got = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want), (n, blen, pad, seeded, group, kern, np.flatnonzero(got != want)[:8])
    return kern


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("nb", [1, 2, 3, 4, 5, 7])
def test_g16_batch_counts(torch_dev, nb, seeded):
    """nb KiB blocks on the G = 16 kernel: first = last, one jump, odd and
    even counts (the last batch in either slot), contiguous and at a stride
    with a 16-B-multiple gap."""
    torch, dev = torch_dev
    for n in NS:
        for pad in (0, 48):
            kern = _check_strided(torch, dev, n, 1024 * nb, pad, seeded, 16, 0xCA00 + 16 * nb + n)
            assert kern == "crc32c_blocks_kernel<16>"


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("group,batch", [(64, 4096), (4, 256), (1, 64)])
def test_forced_groups(torch_dev, group, batch, seeded):
    """One, two and three batches per block at the other group sizes (each has
    its own jump table)."""
    torch, dev = torch_dev
    for nb in (1, 2, 3):
        for n in NS:
            kern = _check_strided(torch, dev, n, batch * nb, 0, seeded, group, 0xF0 + group + nb + n)
            assert kern == "crc32c_blocks_kernel<%d>" % group


def test_chain_ends_with_its_block(torch_dev):
    """More blocks than one pass of the grid holds: a few waves walk a second
    round, whose blocks must start from a zero carry.  2 KiB blocks, seeded,
    every payload distinct."""
    torch, dev = torch_dev
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    kern = _check_strided(torch, dev, 64 * cus + 5, 2048, 0, True, None, 0x2B10C)
    assert kern == "crc32c_blocks_kernel<16>"


def _split_kernel(n, blen, cus):
    """The kernel of lvh::uniform_plan's long-block split (the rule
    tests/test_abi.py::_uniform_plan restates), and its piece length."""
    want, ps = 4 * cus * 16, 0
    while (n << ps) < want and ps < 12:
        s2 = 2 << ps
        if blen % s2 or (blen // s2) % 1024 or blen // s2 < 4096:
            break
        ps += 1
    assert ps > 0
    if (1 << ps) <= 16 and (n << ps) <= 64 * cus:
        return "crc32c_blocks_kernel<16,pieces,fused>", blen >> ps
    return "crc32c_blocks_kernel<16,pieces>+combine_pieces_" + ("wg_kernel" if ps >= 11 else "kernel"), blen >> ps


# n, block length, bytes per piece, joined in the walk
SPLIT_CASES = [(2, 8 << 10, 4096, True), (1, 16 << 10, 4096, True), (3, 32 << 10, 4096, True),
               (5, 64 << 10, 4096, True),  # the one-round walk, 4 batches per piece, fused join
               (1, 256 << 10, 4096, False),  # 64 pieces: the one-round walk, then combine_pieces_kernel
               (600, 40 << 10, 5120, True),  # 5 batches per piece: the batch loop, fused join
               (100, 160 << 10, 5120, False)]  # 32 pieces of 5 batches: the batch loop, two launches


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("n,blen,plen,fused", SPLIT_CASES)
def test_long_block_split(torch_dev, n, blen, plen, fused, seeded):
    torch, dev = torch_dev
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    want_kern, want_plen = _split_kernel(n, blen, cus)
    assert (want_plen, "fused" in want_kern) == (plen, fused), "the case no longer takes the path it was chosen for"
    kern = _check_strided(torch, dev, n, blen, 4096 if n % 2 == 0 else 0, seeded, None, 0x5B11 + n)
    assert kern == want_kern


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("blen,rounds", [(4096, 1), (2048, 2)])
def test_gathered_walk(torch_dev, blen, rounds, seeded):
    """The same kernel through lv_crc32c_batch_device_hint with HINT_UNIFORM |
    HINT_ALIGNED16: shuffled 16-B aligned starts with gaps; 4 KiB x 65, and
    2 KiB blocks five past one pass of the grid."""
    torch, dev = torch_dev
    n = 65 if rounds == 1 else 64 * torch.cuda.get_device_properties(dev).multi_processor_count + 5
    rng = np.random.default_rng(blen + seeded)
    gaps = rng.integers(0, 4, n) * 16
    starts = np.cumsum(gaps + blen) - blen
    offs = rng.permutation(starts).astype(np.uint64)
    lens = np.full(n, blen, dtype=np.uint32)
    a = torch.empty(int(starts[-1]) + blen + 64, dtype=torch.uint8, device=dev)
    lvgpu.fill_splitmix(a, 0, 0x6A7 + blen)
    seeds, sd = _seeds(torch, dev, rng, n, seeded)
    hint = lvgpu.hint_for(lens, offs)
    assert hint.uniform == lvgpu.HINT_UNIFORM | lvgpu.HINT_ALIGNED16
    out = lvgpu.batch_hint(a, torch.from_numpy(offs.astype(np.int64)).to(dev),
                           torch.from_numpy(lens.view(np.int32)).to(dev), hint, seed=sd, masked=seeded)
    kern = lvgpu.last_kernel()
    torch.cuda.synchronize()
    assert kern == ("crc32c_blocks_kernel<64,gather>" if blen == 4096 else "crc32c_blocks_kernel<16,gather>")
    want = oracle_batch(a.cpu().numpy().tobytes(), offs, lens, seeds, seeded)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
