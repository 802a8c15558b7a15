"""Seeded stress of lv_wal_decode_device against oracle/wal_oracle.py's Reader
and the host Reader: 300 logs of at most 2 MiB from random_records, each with 0
to 3 random corruptions (a byte flip, a type edit with the checksum fixed, a
length edit, a truncation), at random payload alignments.  A trial is left out
only if the oracle Reader itself raises on its log; for these seeds it never
does (checked without a GPU below), and at most 2 % may be."""
import pytest

from wal_decode_cases import STRESS_TRIALS, check, oracle_read, stress_log

CHUNK = 50


def _oracle_ok(log):
    try:
        oracle_read(log)
        return True
    except Exception:
        return False


def test_oracle_accepts_the_seeds():
    """(No GPU.)  The oracle Reader raises on at most 2 % of the trials' logs,
    and no log is over 2 MiB."""
    logs = [stress_log(seed) for seed in range(STRESS_TRIALS)]
    assert max(len(l) for l in logs) <= 2 << 20
    left_out = [seed for seed, l in enumerate(logs) if not _oracle_ok(l)]
    assert len(left_out) <= STRESS_TRIALS // 50, left_out
    # the corruptions bite: a good share of the logs make reports
    assert sum(1 for l in logs if _oracle_ok(l) and oracle_read(l)[2]) >= STRESS_TRIALS // 5


@pytest.mark.gpu
@pytest.mark.parametrize("first", range(0, STRESS_TRIALS, CHUNK))
def test_seeded_trials(gpu, first):
    import torch
    left_out = 0
    for seed in range(first, first + CHUNK):
        log = stress_log(seed)
        if not _oracle_ok(log):
            left_out += 1
            continue
        try:
            check(torch, gpu, log, pay_shift=seed % 16, tag=f"seed {seed}")
        except AssertionError:
            print(f"stress trial failed: seed {seed}, {len(log)} log bytes")
            raise
    assert left_out <= CHUNK // 50
