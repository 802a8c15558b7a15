"""The whole pipeline over the host twins against a plain model of the store's
history (tests/store_cases.py): after writes, flushes, compactions and a
reopen, what does the store answer to a Get or a range read at a snapshot?
No GPU: the driver runs over the *_host entry points; test_gpu_store.py runs
the same driver over the device's."""
import pytest

import store_cases as SC
from store_cases import ABSENT, DELETED, DELETION, FOUND, MAX, VALUE, Store, StoreModel

SEEDS = (1, 2, 3)


def host_store(fault=None):
    return Store(SC.HostBackend(), fault)


def test_model_against_the_reference_rules():
    """Six ops in three batches, the answers written out by hand: a batch's
    ops take sequence, sequence + 1, ... (write_batch.rs); Get returns the
    newest entry at or below the snapshot and a deletion hides (memtable.rs)."""
    m = StoreModel()
    m.apply([(VALUE, b"a", b"a1"), (VALUE, b"b", b"b2")])            # sequences 1, 2
    m.apply([(DELETION, b"a", b""), (VALUE, b"c", b"")])             # 3, 4: the empty value is a value
    m.apply([(VALUE, b"a", b"a5"), (DELETION, b"b", b"")])           # 5, 6: a is put again
    assert m.last_sequence == 6
    assert m.history[b"a"] == [(1, VALUE, b"a1"), (3, DELETION, b""), (5, VALUE, b"a5")]
    want = {
        (b"a", 0): (ABSENT, None), (b"a", 1): (FOUND, b"a1"), (b"a", 2): (FOUND, b"a1"),
        (b"a", 3): (DELETED, None),                      # the deletion exactly at the snapshot
        (b"a", 4): (DELETED, None), (b"a", 5): (FOUND, b"a5"), (b"a", MAX): (FOUND, b"a5"),
        (b"b", 1): (ABSENT, None), (b"b", 2): (FOUND, b"b2"), (b"b", 5): (FOUND, b"b2"), (b"b", 6): (DELETED, None),
        (b"c", 3): (ABSENT, None), (b"c", 4): (FOUND, b""), (b"c", MAX): (FOUND, b""),
        (b"", MAX): (ABSENT, None), (b"a\0", MAX): (ABSENT, None), (b"d", MAX): (ABSENT, None),
    }
    for (key, snap), answer in want.items():
        assert m.get(key, snap) == answer, (key, snap)
    assert m.range(b"", None, MAX, 1000) == [(b"a", b"a5"), (b"c", b"")]
    assert m.range(b"", None, 4, 1000) == [(b"b", b"b2"), (b"c", b"")]
    assert m.range(b"", None, 2, 1000) == [(b"a", b"a1"), (b"b", b"b2")]
    assert m.range(b"a", b"b", 2, 1000) == [(b"a", b"a1")]           # hi is exclusive
    assert m.range(b"a\0", None, 2, 1000) == [(b"b", b"b2")]
    assert m.range(b"", None, 2, 1) == [(b"a", b"a1")]
    assert m.range(b"", None, 0, 1000) == []


def assert_life(total, store, model, asked=100000, ranges=3000):
    """No answer differs, and the check did not pass by asking little."""
    assert not total.mismatches, total.mismatches[:5]
    assert total.asked > asked and total.ranges > ranges
    for n in (total.found, total.deleted, total.absent):
        assert 10 * n >= total.asked, (total.asked, total.found, total.deleted, total.absent)
    assert {"mem", "level0 older", "deeper"} <= total.sources, total.sources
    c = store.compactions
    assert [x["level"] for x in c] == [0, 1, 0]
    assert len(c[0]["picked"]) == 2 and len(c[0]["outputs"]) > 8           # two level-0 files into a run
    assert c[1]["outputs"] and store.files[c[1]["outputs"][0]][0] == 2     # a level-1 file went down to level 2
    assert c[2]["below"] and c[2]["untouched"] and c[2]["ranges"]          # level 0 + part of level 1, level 2 beneath
    assert sum(x["totals"]["dropped_deletions"] for x in c) > 0
    assert store.floor == model.last_sequence == store.last_sequence


@pytest.mark.parametrize("seed", SEEDS)
def test_life_of_a_store(seed):
    """Four generations of about 1,500 ops in about 300 batches over about 120
    user keys, checked after every group, flush, compaction and the reopen."""
    store, model = host_store(), StoreModel()
    total = SC.life(store, model, seed)
    assert_life(total, store, model)
    assert any(len(b) == 40 for g in SC.generation(SC.np.random.default_rng(seed), SC.universe(), 0, big=True)
               for b in g)
    assert b"" in model.history and any(v == b"" and t == VALUE for _, t, v in sum(model.history.values(), []))
    assert max(len(v) for _, _, v in sum(model.history.values(), [])) > 4096


def assert_tombstone_story(facts, total):
    assert facts["k lies on level 2"]
    assert facts["k's tombstone is kept"] and facts["get k"] == DELETED           # rule B must not fire: level 2 holds k
    assert facts["j's tombstone is dropped"] and facts["dropped_deletions"] == 1  # nothing beneath j
    assert facts["get j"] == ABSENT
    assert facts["levels after the last compaction"] == [2] and facts["no entry of k is left"]
    assert facts["get k at the end"] == ABSENT
    assert not total.mismatches, total.mismatches[:5]


def test_a_tombstone_above_a_deeper_value():
    facts, total = SC.tombstone_story(host_store(), StoreModel())
    assert_tombstone_story(facts, total)


@pytest.mark.parametrize("fault", SC.FAULTS)
def test_the_check_notices(fault):
    """The check can fail: each fault changes the driver only, and the check
    reports it."""
    store, model = host_store(fault), StoreModel()
    if fault == "ranges_omitted":
        facts, total = SC.tombstone_story(store, model)
        assert facts["get k"] == FOUND  # the level-2 value is back
        assert any(m[0] == "get" and m[1] == b"k" and m[3][0] == FOUND and m[4][0] == DELETED for m in total.mismatches)
        return
    total = SC.life(store, model, 5, per_group=fault in ("first_sequence_off_by_one", "dest_length_zero"),
                    stop_at_mismatch=True)
    kinds = {m[0] for m in total.mismatches}
    assert total.mismatches
    if fault == "first_sequence_off_by_one":
        assert "last_sequence" in kinds and "get" in kinds and store.groups_in_log == 2
    elif fault == "dest_length_zero":
        assert "the log lost records" in kinds and store.groups_in_log >= 2
    elif fault == "level0_oldest_first":
        assert store.unsorted_seen  # lv_version_open_* refuses the order as it is
        stale = [m for m in total.mismatches if m[0] == "get" and m[3][0] == FOUND and m[3][1] != m[4][1]]
        assert stale and len(store.level_files(0)) == 2  # renumbered, it opens and a stale value wins
    elif fault == "compaction_inputs_not_removed":
        assert "version open status" in kinds and store.ver.status & SC.V.OPEN_UNSORTED
    elif fault == "floor_ignored":
        assert kinds <= {"get", "range", "resume chain"} and "get" in kinds and store.compactions
        sound, m2 = host_store(), StoreModel()  # the same history asked at and above the floor only: nothing differs
        assert not SC.life(sound, m2, 5, per_group=False, generations=2).mismatches
