"""The carried fold of the uniform-block kernel (lvk::fold_batch_carry),
restated without a device.

Row i, lane l of a group is one CRC stream over its granules of successive
batches, 16*G*U bytes apart.  A granule is four slice steps s <- T(s) ^ next
word with T = Shift_4; the carried register enters the granule's first word.
On every batch but the block's last the fourth step reads J = Shift_{16GU-12}
instead of T, which leaves the register just before the stream's next
granule; the last batch reads T and leaves R at the end of its granule.
Shifting every stream to the block's end and xoring them must give
R(~seed, block), i.e. the oracle's value / extend."""
import random
import struct

import pytest

import wal_oracle as W

POLY = 0x82F63B78
U = 4


def _zero_byte(s):
    for _ in range(8):
        s = (s >> 1) ^ POLY if s & 1 else s >> 1
    return s


def _apply(m, v):
    r = 0
    for j in range(32):
        if v >> j & 1:
            r ^= m[j]
    return r


def _shift_matrix(nbytes):
    """Shift_n as 32 column images, by square-and-multiply over bit-serial
    single-byte steps."""
    one = [_zero_byte(1 << j) for j in range(32)]
    acc = [1 << j for j in range(32)]
    while nbytes:
        if nbytes & 1:
            acc = [_apply(one, c) for c in acc]
        one = [_apply(one, c) for c in one]
        nbytes >>= 1
    return acc


def _carried_register(block, seed, G, nb):
    """R(~seed, block) by the kernel's carried streams."""
    assert len(block) == 16 * G * U * nb
    T = _shift_matrix(4)
    J = _shift_matrix(16 * G * U - 12)
    S16 = _shift_matrix(16)
    words = list(struct.unpack("<%dI" % (len(block) // 4), block))
    words[0] ^= ~seed & 0xFFFFFFFF  # the seed enters lane 0's first word of batch 0
    X = 0
    for i in range(U):
        for l in range(G):
            a = 0
            for b in range(nb):
                w = 4 * ((b * U + i) * G + l)
                s = words[w] ^ a
                s = _apply(T, s) ^ words[w + 1]
                s = _apply(T, s) ^ words[w + 2]
                s = _apply(T, s) ^ words[w + 3]
                a = _apply(T if b == nb - 1 else J, s)
            # the streams end 16 bytes apart in (row, lane) order, the last at
            # the block's end: Horner with Shift_16 shifts each to that end
            X = _apply(S16, X) ^ a
    return X


@pytest.mark.parametrize("G,nb", [(16, 4), (16, 1), (16, 7), (64, 2), (4, 3), (1, 5)])
def test_carried_streams_reproduce_the_crc(G, nb):
    rng = random.Random(1000 * G + nb)
    block = bytes(rng.randrange(256) for _ in range(16 * G * U * nb))
    assert _carried_register(block, 0, G, nb) ^ 0xFFFFFFFF == W.value(block)
    seed = rng.randrange(1 << 32)
    assert _carried_register(block, seed, G, nb) ^ 0xFFFFFFFF == W.extend(seed, block)


def test_jump_is_the_row_shift_after_the_last_slice_step():
    """J = Shift_{16GU-16} o Shift_4: what W4 did to the accumulator as a
    separate lookup, moved behind the granule's last slice step."""
    for G in (1, 4, 16, 64):
        n = 16 * G * U
        J, T, gap = _shift_matrix(n - 12), _shift_matrix(4), _shift_matrix(n - 16)
        rng = random.Random(G)
        for _ in range(8):
            s = rng.randrange(1 << 32)
            assert _apply(J, s) == _apply(gap, _apply(T, s))
