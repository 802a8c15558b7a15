"""lv_version_open_device / lv_version_get_device over random consistent
versions (tests/version_cases.py: a simulated op stream with flushes and
whole-level compactions), a few hundred trials: the GPU against the serial
model, field for field, and against the union rule (every answer is
lv_memtable_get_host's over the union of all files' entries)."""
import pytest

import sst_get_cases as G
import version_cases as C

pytestmark = pytest.mark.gpu

TRIALS = 240
CHUNK = 40


@pytest.mark.parametrize("chunk", range(TRIALS // CHUNK))
def test_random_consistent_versions(gpu, chunk):
    import torch
    seen, levels, reads = set(), set(), 0
    for seed in range(1000 + chunk * CHUNK, 1000 + (chunk + 1) * CHUNK):
        bloom = seed % 3 != 0
        ver = C.random_version(seed, bpk=None if seed % 5 == 0 else 10, shift=(0, 1, 5, 8)[seed % 4])
        queries = C.queries_for(ver)
        if len(queries) > 300:
            queries = queries[::len(queries) // 300 + 1]
        s, _, wants = C.check_device(torch, gpu, ver, queries, bloom=bloom, tag_=f"seed {seed}")
        C.check_union(ver, queries, wants[: len(queries)])
        seen |= s
        levels |= {f["level"] for f in ver.files}
        reads = max(reads, max(w["files_read"] for w in wants))
    assert {G.ABSENT, G.FOUND, G.DELETED, G.BAD_SEQ, G.BAD_QUERY} <= seen
    assert len(levels) >= 4 and reads >= 4, (levels, reads)
