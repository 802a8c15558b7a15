"""The positioned last batch and the XOR join of the uniform-block kernel
(lvk::fold_batch_carry on `last`, lvk::join_group), restated without a device.

Row i, lane l = w*m + c of a group (w = min(G, 8) lanes per sub-group,
M = G / w sub-groups) is one CRC stream, as in test_blocks_carry_algebra.py.
On the block's last batch the fourth slice step of rows 0-1 reads
E1_c = Shift_{4 + 32G + 16(w-1-c)} and that of rows 2-3 reads
E0_c = Shift_{4 + 16(w-1-c)} in place of T = Shift_4: every stream of a
sub-group leaves its register at the end of the sub-group's last granule, rows
0 and 2 in row 2, rows 1 and 3 in row 3.  The registers of a sub-group then
join by plain XOR (y_m from rows 0 and 2, z_m from rows 1 and 3) and only the
M pairs (y_m, z_m) are shifted to the block's end, grouped as the kernel
groups them.  The result must be R(~seed, block): the oracle's value / extend."""
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


_CACHE = {}


def _shift_matrix(nbytes):
    """Shift_n as 32 column images, by square-and-multiply over bit-serial
    single-byte steps."""
    if nbytes not in _CACHE:
        n = nbytes
        one = [_zero_byte(1 << j) for j in range(32)]
        acc = [1 << j for j in range(32)]
        while n:
            if n & 1:
                acc = [_apply(one, c) for c in acc]
            one = [_apply(one, c) for c in one]
            n >>= 1
        _CACHE[nbytes] = acc
    return _CACHE[nbytes]


def _shift(nbytes, v):
    return _apply(_shift_matrix(nbytes), v)


def _e0(G, c):
    return _shift_matrix(4 + 16 * (min(G, 8) - 1 - c))


def _e1(G, c):
    return _shift_matrix(4 + 32 * G + 16 * (min(G, 8) - 1 - c))


def _subgroup_sums(block, seed, G, nb):
    """(y_m, z_m), m < M: the XOR over a sub-group's lanes of rows 0 ^ 2 and
    of rows 1 ^ 3 after the positioned last batch."""
    assert len(block) == 16 * G * U * nb
    w = min(G, 8)
    T = _shift_matrix(4)
    J = _shift_matrix(16 * G * U - 12)
    words = list(struct.unpack("<%dI" % (len(block) // 4), block))
    words[0] ^= ~seed & 0xFFFFFFFF  # the seed enters lane 0's first word of batch 0
    y = [0] * (G // w)
    z = [0] * (G // w)
    for i in range(U):
        for l in range(G):
            m, c = divmod(l, w)
            a = 0
            for b in range(nb):
                k = 4 * ((b * U + i) * G + l)
                s = words[k] ^ a
                s = _apply(T, s) ^ words[k + 1]
                s = _apply(T, s) ^ words[k + 2]
                s = _apply(T, s) ^ words[k + 3]
                if b < nb - 1:
                    a = _apply(J, s)
                else:  # the table by (row pair, l mod w)
                    a = _apply(_e1(G, c) if i < 2 else _e0(G, c), s)
            if i % 2 == 0:
                y[m] ^= a
            else:
                z[m] ^= a
    return y, z


def _joined_register(block, seed, G, nb):
    """R(~seed, block) with the final shifts grouped as join_group groups them."""
    y, z = _subgroup_sums(block, seed, G, nb)
    if G <= 4:  # one sub-group: Shift_16G(y) ^ z
        return _shift(16 * G, y[0]) ^ z[0]
    if G == 16:  # four partials, one table each, and an XOR
        return _shift(384, y[0]) ^ _shift(128, z[0]) ^ _shift(256, y[1]) ^ z[1]
    assert G == 64  # v_m at the end of octet m's row 3, then a tree over the octets
    v = [_shift(1024, y[m]) ^ z[m] for m in range(8)]
    for k in range(3):
        for m in range(0, 8, 2 << k):
            v[m] = _shift(128 << k, v[m]) ^ v[m + (1 << k)]
    return v[0]


def _general_register(block, seed, G, nb):
    """The issue's closed form: X = XOR_m Shift_{16w(M-1-m)}(Shift_16G(y_m) ^ z_m)."""
    y, z = _subgroup_sums(block, seed, G, nb)
    w = min(G, 8)
    M = G // w
    X = 0
    for m in range(M):
        X ^= _shift(16 * w * (M - 1 - m), _shift(16 * G, y[m]) ^ z[m])
    return X


CASES = [(16, 4), (16, 1), (16, 7), (64, 2), (64, 1), (4, 3), (1, 5)]


@pytest.mark.parametrize("G,nb", CASES)
def test_positioned_streams_join_to_the_crc(G, nb):
    rng = random.Random(7000 * G + nb)
    block = bytes(rng.randrange(256) for _ in range(16 * G * U * nb))
    assert _joined_register(block, 0, G, nb) ^ 0xFFFFFFFF == W.value(block)
    assert _general_register(block, 0, G, nb) ^ 0xFFFFFFFF == W.value(block)
    seed = rng.randrange(1 << 32)
    assert _joined_register(block, seed, G, nb) ^ 0xFFFFFFFF == W.extend(seed, block)
    assert _general_register(block, seed, G, nb) ^ 0xFFFFFFFF == W.extend(seed, block)


@pytest.mark.parametrize("G", [1, 4, 16, 64])
def test_last_batch_tables(G):
    """E1_c = Shift_32G o E0_c (rows 0-1 sit two rows before rows 2-3), and
    the sub-group's last lane needs no extra shift: E0_{w-1} = T = Shift_4."""
    w = min(G, 8)
    assert _e0(G, w - 1) == _shift_matrix(4)
    rng = random.Random(G)
    for c in range(w):
        for _ in range(4):
            s = rng.randrange(1 << 32)
            assert _apply(_e1(G, c), s) == _shift(32 * G, _apply(_e0(G, c), s))
            # ... and E0_c is the slice step followed by the lanes still to come
            assert _apply(_e0(G, c), s) == _shift(16 * (w - 1 - c), _shift(4, s))
