"""A serial Python model of lv_version_apply_* written from the contract in
include/lvgpu/version_set.h (not from the C code), the cases the CPU and GPU
tests share, and the dump tools/version_apply_hostcheck.cc replays.

An edit is version_edit_cases' dict (new_edit): scalars or None, pointers
[(level, key)], deleted [(level, number)], files [(level, number, file_size,
smallest, largest)] with internal keys as bytes.  A case is the tuple
version_edit_cases.tables_of makes of such edits -- (src, edits, files,
rec_file, deleted, rec_deleted, pointers, rec_pointer) -- plus a directory.
"""
import json
import os
import struct

import numpy as np

import version_edit_cases as EC
from version_edit_cases import internal_key, new_edit, tables_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "version_apply_example.json")

UPSTREAM, REC_OVER, BAD_BOUNDS, BAD_ROW, DUPLICATE, BAD_DIRECTORY, FILE_OVER = 1, 2, 4, 8, 16, 32, 64
KIND_POINTER, KIND_DELETED, KIND_FILE, KIND_DIRECTORY = 1, 2, 3, 4
NUM_LEVELS = 7
MAX_NUMBER = 1 << 56
NONE = (1 << 64) - 1
NO_DIR_INDEX = 0xFFFFFFFF
FILE_UNPLACED = 6
M64 = (1 << 64) - 1
VALUE = 1


def k(user, seq, vtype=VALUE):
    return internal_key(user if isinstance(user, bytes) else user.encode(), seq, vtype)


# ---- the model --------------------------------------------------------------------
def _refused(records, status, kind=NONE, row=NONE):
    t = dict(records=records, new_files=0, deleted=0, pointers=0, live=0, unplaced=0, level_files=[0] * 7,
             level_bytes=[0] * 7, compact_pointer=[0] * 7, log_number=0, prev_log_number=0, next_file_number=0,
             last_sequence=0, comparator_off=0, comparator_len=0, has=0, max_file_number=0, status=status, bad_kind=kind,
             bad_row=row)
    return [], [], t


def model(src, E, F, bf, D, bd, P, bp, directory=None, *, records=None, caps=None, files_cap=None, upstream=0,
          rec_cap=None, src_bytes=None):
    """(rows, dir_index, totals): rows are dicts with the fields of
    lv_version_file.  `records` is *d_records, rec_cap the capacity (default:
    no REC_OVER), directory [(number, file_off, file_cap)] or None."""
    n = len(E) if records is None else records
    nb = len(src) if src_bytes is None else src_bytes
    caps = (len(F), len(D), len(P)) if caps is None else caps
    if upstream:
        return _refused(0, UPSTREAM)
    if rec_cap is not None and n > rec_cap:
        return _refused(n, REC_OVER)
    bounds = {KIND_POINTER: (bp, caps[2]), KIND_DELETED: (bd, caps[1]), KIND_FILE: (bf, caps[0])}
    for r in range(n):
        for kind in (KIND_POINTER, KIND_DELETED, KIND_FILE):
            b, cap = bounds[kind]
            if not int(b[r]) <= int(b[r + 1]) <= cap:
                return _refused(n, BAD_BOUNDS, kind, r)
    lo = {kind: int(bounds[kind][0][0]) if n else 0 for kind in bounds}
    hi = {kind: int(bounds[kind][0][n]) if n else 0 for kind in bounds}

    def inside(off, ln):
        return int(off) <= nb and int(ln) <= nb - int(off)

    for i in range(lo[KIND_POINTER], hi[KIND_POINTER]):
        p = P[i]
        if p["level"] >= NUM_LEVELS or p["key_len"] < 8 or not inside(p["key_off"], p["key_len"]):
            return _refused(n, BAD_ROW, KIND_POINTER, i)
    for i in range(lo[KIND_DELETED], hi[KIND_DELETED]):
        if D[i]["level"] >= NUM_LEVELS or int(D[i]["number"]) >= MAX_NUMBER:
            return _refused(n, BAD_ROW, KIND_DELETED, i)
    for i in range(lo[KIND_FILE], hi[KIND_FILE]):
        f = F[i]
        if (f["level"] >= NUM_LEVELS or int(f["number"]) >= MAX_NUMBER or f["smallest_len"] < 8 or f["largest_len"] < 8
                or not inside(f["smallest_off"], f["smallest_len"]) or not inside(f["largest_off"], f["largest_len"])):
            return _refused(n, BAD_ROW, KIND_FILE, i)
    # per pair: the record and row of its NewFile row, the records of its deleted rows
    added, deletes = {}, {}
    for r in range(n):
        for i in range(int(bd[r]), int(bd[r + 1])):
            deletes.setdefault((int(D[i]["level"]), int(D[i]["number"])), []).append(r)
        for i in range(int(bf[r]), int(bf[r + 1])):
            pair = (int(F[i]["level"]), int(F[i]["number"]))
            if pair in added:
                return _refused(n, DUPLICATE, KIND_FILE, i)  # rows are met in ascending order: the lowest
            added[pair] = (r, i)
    directory = list(directory) if directory is not None else []
    for i in range(1, len(directory)):
        if directory[i - 1][0] >= directory[i][0]:
            return _refused(n, BAD_DIRECTORY, KIND_DIRECTORY, i)

    live = [(pair, i) for pair, (r, i) in added.items() if not any(x > r for x in deletes.get(pair, ()))]

    def order(item):
        (level, number), i = item
        if level == 0:
            return (0, -number)
        key = bytes(src[int(F[i]["smallest_off"]): int(F[i]["smallest_off"]) + int(F[i]["smallest_len"])])
        return (level, key[:-8], -int.from_bytes(key[-8:], "little"), number)

    live.sort(key=order)
    _, _, t = _refused(n, 0)
    t["new_files"], t["deleted"], t["pointers"] = (hi[kind] - lo[kind] for kind in (KIND_FILE, KIND_DELETED, KIND_POINTER))
    for i in range(lo[KIND_POINTER], hi[KIND_POINTER]):
        t["compact_pointer"][int(P[i]["level"])] = i + 1
    have = {}
    for r in range(n):
        e = E[r]
        for b, name in enumerate(("comparator", "log_number", "prev_log_number", "next_file_number", "last_sequence")):
            if int(e["has"]) >> b & 1:
                t["has"] |= 1 << b
                if b == 0:
                    t["comparator_off"], t["comparator_len"] = int(e["comparator_off"]), int(e["comparator_len"])
                else:
                    t[name] = int(e[name])
                have[name] = True
    for name in ("log_number", "prev_log_number"):  # MarkFileNumberUsed
        if name in have and t["next_file_number"] <= t[name]:
            t["next_file_number"] = (t[name] + 1) & M64
    where = {number: (idx, off, cap) for idx, (number, off, cap) in enumerate(directory)}
    rows, index = [], []
    for (level, number), i in live:
        f = F[i]
        size = int(f["file_size"])
        t["level_files"][level] += 1
        t["level_bytes"][level] += size
        t["max_file_number"] = max(t["max_file_number"], number)
        row = dict(number=number, file_off=0, file_cap=size, smallest_off=int(f["smallest_off"]),
                   largest_off=int(f["largest_off"]), smallest_len=int(f["smallest_len"]), largest_len=int(f["largest_len"]),
                   level=level, status=0, reserved=i)
        at = NO_DIR_INDEX
        if directory:
            if number in where and where[number][2] >= size:
                at, row["file_off"], row["file_cap"] = where[number]
            else:
                row["file_cap"], row["status"] = 0, FILE_UNPLACED
                t["unplaced"] += 1
        rows.append(row)
        index.append(at)
    t["live"] = len(rows)
    if files_cap is not None and len(rows) > files_cap:
        t["status"] = FILE_OVER
        return [], [], t
    return rows, index, t


def rows_as_dicts(rows):
    """An lvgpu.version.FILE_DTYPE array as the model's rows."""
    return [{n: int(r[n]) for n in rows.dtype.names} for r in rows]


# ---- the worked example -----------------------------------------------------------
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def example_edits(upto=None):
    g = golden()
    key = lambda j: k(j[0], j[1])
    edits = []
    for r in g["records"][: upto]:
        edits.append(new_edit(log_number=r.get("log_number"), next_file_number=r.get("next_file_number"),
                              last_sequence=r.get("last_sequence"),
                              pointers=[(lv, key(j)) for lv, j in r.get("pointers", [])],
                              deleted=[tuple(d) for d in r.get("deleted", [])],
                              files=[(lv, num, size, key(s), key(l)) for lv, num, size, s, l in r.get("files", [])]))
    return edits


# ---- histories --------------------------------------------------------------------
def user_key(rng, style):
    """User keys that stress the compare: empty (an 8-byte internal key), one
    byte, long ones with shared prefixes beyond 16 bytes, and ordinary ones."""
    x = int(rng.integers(0, 1 << 20))
    if style == 0:
        return b"" if x % 7 == 0 else bytes([x % 251])
    if style == 1:
        return b"P" * 16 + b"%05d" % (x % 40)                # equal 16-byte prefixes: the remainder decides
    if style == 2:
        return b"shared-prefix-of-more-than-sixteen-bytes/" * 5 + b"%07d" % (x % 3000)   # over 200 bytes
    if style == 3:
        return b"k%04d" % (x % 50)                            # few user keys: many differ in the tag only
    return b"key%08d" % x


def random_history(seed, records=40, *, per_flush=1, level0_share=0.5, styles=(0, 1, 2, 3, 4), directory_gaps=True,
                   compaction_width=4, compaction_share=0.3, compaction_out=None):
    """A legal history (no pair added twice) with what the contract calls not
    an error: flushes to level 0, compactions of several files into the level
    below, trivial moves, deletes of files nobody added, deletes in the record
    of the add and in a record before it, compact pointers.  Returns (edits,
    directory)."""
    rng = np.random.default_rng(seed)
    edits, nxt, seq = [], 2, 1
    live = {lv: [] for lv in range(NUM_LEVELS)}   # level -> numbers
    size_of = {}

    def new_file(level):
        nonlocal nxt, seq
        number = nxt
        nxt += 1
        style = int(styles[int(rng.integers(len(styles)))])
        a, b = sorted((user_key(rng, style), user_key(rng, style)))
        s = k(a, seq + int(rng.integers(0, 3)))
        l = k(b, seq) if a != b else s[:-8] + struct.pack("<Q", min(struct.unpack("<Q", s[-8:])[0], (seq << 8) | VALUE))
        seq += 3
        size_of[number] = int(rng.integers(100, 5000))
        live[level].append(number)
        return (level, number, size_of[number], s, l)

    for r in range(records):
        e = new_edit()
        roll = rng.random()
        if rng.random() < 0.8:
            e["next_file_number"], e["last_sequence"] = nxt + 5, seq
        if rng.random() < 0.4:
            e["log_number"] = nxt
            nxt += 1
        if r == 0:
            e["comparator"] = b"leveldb.BytewiseComparator"
            e["prev_log_number"] = 0
        if roll < level0_share or not any(live.values()):
            e["files"] = [new_file(0) for _ in range(per_flush)]
        elif roll < level0_share + compaction_share:         # a compaction
            src_level = int(rng.choice([lv for lv in range(NUM_LEVELS - 1) if live[lv]] or [0]))
            if live[src_level]:
                take = [live[src_level].pop(int(rng.integers(len(live[src_level]))))
                        for _ in range(min(len(live[src_level]), int(rng.integers(1, compaction_width + 1))))]
                below = [live[src_level + 1].pop() for _ in range(min(len(live[src_level + 1]), int(rng.integers(0, 3))))]
                e["deleted"] = sorted([(src_level, n) for n in take] + [(src_level + 1, n) for n in below])
                e["files"] = [new_file(src_level + 1) for _ in range(int(rng.integers(0, (compaction_out or compaction_width) + 1)))]
                e["pointers"] = [(src_level, k(b"ptr%d" % r, seq))]
        elif roll < level0_share + compaction_share + 0.1:   # a trivial move
            cands = [lv for lv in range(NUM_LEVELS - 1) if live[lv]]
            if cands:
                lv = int(rng.choice(cands))
                n = live[lv].pop(int(rng.integers(len(live[lv]))))
                e["deleted"] = [(lv, n)]
                live[lv + 1].append(n)
                number, nxt_keep = n, nxt
                f = new_file(lv + 1)                         # fresh bounds under the old number
                live[lv + 1].pop()
                nxt = nxt_keep
                e["files"] = [(lv + 1, number, size_of[number], f[3], f[4])]
        elif roll < level0_share + compaction_share + 0.15:  # deletes of files nobody added
            e["deleted"] = sorted({(int(rng.integers(NUM_LEVELS)), 1 << 40 | int(rng.integers(1000))) for _ in range(3)})
        else:                                                # a delete before, and one beside, the add
            lv = int(rng.integers(1, NUM_LEVELS))
            if edits:
                edits[-1]["deleted"] = sorted(set(edits[-1]["deleted"]) | {(lv, nxt)})
            f = new_file(lv)
            e["deleted"] = [(lv, f[1])]
            e["files"] = [f]
        edits.append(e)
    numbers = sorted(n for lv in live.values() for n in lv)
    directory, at = [], 16
    for i, n in enumerate(numbers):
        if directory_gaps and i % 9 == 4:
            continue                                         # a live file the directory does not know
        cap = size_of[n] + (i % 3) * 16 if not (directory_gaps and i % 11 == 7) else size_of[n] - 1   # too small
        directory.append((n, at, cap))
        at += (cap + 31) & ~15
    directory += [(1 << 50 | j, at + 64 * j, 64) for j in range(3)]   # entries nobody uses
    return edits, directory


def consistent_history(seed, live_files, level0=6):
    """A history whose version opens (lv_version_open_*: status 0): level-0
    files may overlap, deeper levels hold disjoint key ranges, added out of
    order and partly replaced by compactions under new numbers.  Exactly
    `live_files` files stay live and every one is placed.  Returns (edits,
    directory)."""
    rng = np.random.default_rng(seed)
    edits, nxt, size_of = [], 2, {}
    deep = live_files - level0
    slots = [(1 + j % 3, j) for j in range(deep)]             # (level, range index): ranges ascend within a level
    order = list(rng.permutation(deep))
    holder = {}

    def file_for(slot, seq):
        nonlocal nxt
        level, j = slot
        number = nxt
        nxt += 1
        size_of[number] = int(rng.integers(100, 5000))
        holder[slot] = number
        return (level, number, size_of[number], k(b"range-%02d-%06d-a" % (level, j), seq), k(b"range-%02d-%06d-z" % (level, j), 1))

    seq = 10
    for at in range(0, deep, 5):
        e = new_edit(log_number=nxt, next_file_number=nxt + 9, last_sequence=seq)
        e["files"] = [file_for(slots[j], seq) for j in order[at: at + 5]]
        seq += 7
        edits.append(e)
    for j in rng.permutation(deep)[: deep // 4]:              # a compaction rewrites the range under a new number
        slot = slots[int(j)]
        e = new_edit(next_file_number=nxt + 3, last_sequence=seq, deleted=[(slot[0], holder[slot])],
                     pointers=[(slot[0], k(b"range-%02d-%06d-z" % slot, 1))])
        size_of.pop(holder[slot])
        e["files"] = [file_for(slot, seq)]
        seq += 3
        edits.append(e)
    for _ in range(level0):
        number = nxt
        nxt += 1
        size_of[number] = int(rng.integers(100, 5000))
        a, b = sorted((user_key(rng, 4), user_key(rng, 4) + b"x"))
        edits.append(new_edit(log_number=nxt, next_file_number=nxt + 1, last_sequence=seq,
                              files=[(0, number, size_of[number], k(a, seq), k(b, seq - 1))]))
        seq += 5
    directory, at = [], 0
    for n in sorted(size_of):
        directory.append((n, at, size_of[n] + 16 * (n % 3)))
        at += (size_of[n] + 16 * (n % 3) + 15) & ~15
    return edits, directory


def case_of(edits, directory=None, lead=(0, 0, 0)):
    return tables_of(edits, lead) + (directory,)


# ---- damaged inputs ---------------------------------------------------------------
def damaged_cases():
    """[(name, case, kwargs of the call, (status, bad_kind, bad_row))]: each
    status bit that an input can raise on the host, and pairs of them where
    the earlier one wins."""
    edits, directory = random_history(11, 30)
    base = case_of(edits, directory)
    out = []

    def variant(name, want, mutate, **kw):
        src, E, F, bf, D, bd, P, bp, dr = base
        c = dict(src=src, E=E.copy(), F=F.copy(), bf=bf.copy(), D=D.copy(), bd=bd.copy(), P=P.copy(), bp=bp.copy(),
                 dr=list(dr))
        mutate(c)
        out.append((name, (c["src"], c["E"], c["F"], c["bf"], c["D"], c["bd"], c["P"], c["bp"], c["dr"]), kw, want))

    src, E, F, bf, D, bd, P, bp, dr = base
    nf, nd, np_ = len(F), len(D), len(P)
    assert nf > 20 and nd > 10 and np_ > 3 and len(dr) > 6

    def setf(table, i, field, v):
        def m(c):
            c[table][i][field] = v
        return m

    def both(*ms):
        def m(c):
            for x in ms:
                x(c)
        return m

    def bound(name, r, v):
        def m(c):
            c[name][r] = v
        return m

    def swap_dir(i):
        def m(c):
            c["dr"][i - 1], c["dr"][i] = c["dr"][i], c["dr"][i - 1]
        return m

    def dup_dir(i):
        def m(c):
            c["dr"][i] = (c["dr"][i - 1][0],) + c["dr"][i][1:]
        return m

    def dup_file(i, j):
        def m(c):
            c["F"][i]["level"], c["F"][i]["number"] = c["F"][j]["level"], c["F"][j]["number"]
        return m

    variant("bounds_order_file", (BAD_BOUNDS, KIND_FILE, 4), bound("bf", 5, int(bf[4]) - 1 if bf[4] else nf + 1))
    variant("bounds_over_deleted", (BAD_BOUNDS, KIND_DELETED, len(E) - 1), bound("bd", len(E), nd + 1))
    variant("bounds_pointer_and_file", (BAD_BOUNDS, KIND_POINTER, len(E) - 1),
            both(bound("bp", len(E), np_ + 7), bound("bf", len(E), nf + 7)))
    variant("bounds_two_records", (BAD_BOUNDS, KIND_DELETED, 2), both(bound("bd", 3, nd + 1), bound("bf", 9, nf + 3)))
    variant("pointer_level", (BAD_ROW, KIND_POINTER, 1), setf("P", 1, "level", 7))
    variant("pointer_extent", (BAD_ROW, KIND_POINTER, 2), setf("P", 2, "key_off", len(src) - 3))
    variant("pointer_short", (BAD_ROW, KIND_POINTER, 0), setf("P", 0, "key_len", 7))
    variant("deleted_level", (BAD_ROW, KIND_DELETED, 3), setf("D", 3, "level", 0x80000000))
    variant("deleted_number", (BAD_ROW, KIND_DELETED, 5), setf("D", 5, "number", MAX_NUMBER))
    variant("file_level", (BAD_ROW, KIND_FILE, 7), setf("F", 7, "level", 7))
    variant("file_number", (BAD_ROW, KIND_FILE, 2), setf("F", 2, "number", MAX_NUMBER + 5))
    variant("file_smallest_extent", (BAD_ROW, KIND_FILE, 9), setf("F", 9, "smallest_off", M64 - 3))
    variant("file_largest_extent", (BAD_ROW, KIND_FILE, nf - 1), setf("F", nf - 1, "largest_len", len(src) + 1))
    variant("file_smallest_short", (BAD_ROW, KIND_FILE, 4), setf("F", 4, "smallest_len", 3))
    variant("file_largest_short", (BAD_ROW, KIND_FILE, 0), setf("F", 0, "largest_len", 0))
    variant("lowest_kind_wins", (BAD_ROW, KIND_DELETED, 6), both(setf("F", 1, "level", 9), setf("D", 6, "level", 9)))
    variant("lowest_row_wins", (BAD_ROW, KIND_FILE, 3), both(setf("F", 12, "level", 9), setf("F", 3, "smallest_len", 1)))
    variant("duplicate", (DUPLICATE, KIND_FILE, 15), dup_file(15, 6))
    variant("duplicate_lowest", (DUPLICATE, KIND_FILE, 10), both(dup_file(18, 2), dup_file(10, 8)))
    variant("duplicate_thrice", (DUPLICATE, KIND_FILE, 11), both(dup_file(11, 5), dup_file(17, 5)))
    variant("directory_swapped", (BAD_DIRECTORY, KIND_DIRECTORY, 3), swap_dir(3))
    variant("directory_equal", (BAD_DIRECTORY, KIND_DIRECTORY, 5), both(dup_dir(5), swap_dir(len(dr) - 1)))
    variant("file_over", (FILE_OVER, NONE, NONE), lambda c: None, files_cap=3)
    variant("bounds_before_row", (BAD_BOUNDS, KIND_FILE, 0), both(bound("bf", 1, nf + 1), setf("P", 0, "level", 9)))
    variant("row_before_duplicate", (BAD_ROW, KIND_POINTER, 3), both(setf("P", 3, "key_len", 2), dup_file(15, 6)))
    variant("duplicate_before_directory", (DUPLICATE, KIND_FILE, 15), both(dup_file(15, 6), swap_dir(2)))
    variant("directory_before_file_over", (BAD_DIRECTORY, KIND_DIRECTORY, 2), swap_dir(2), files_cap=1)
    return out


# ---- the dump tools/version_apply_hostcheck.cc replays ------------------------------
def dump_cases():
    """[(name, case, kwargs, rows, index, totals)] by the model."""
    import lvgpu.version_set as VS
    out = []

    def add(name, case, **kw):
        rows, index, t = model(*case[:8], case[8], **kw)
        kw.setdefault("files_cap", len(case[2]))
        out.append((name, case, kw, rows, index, t))

    add("empty", case_of([], None))
    for upto in range(1, 7):
        add(f"example_{upto}", case_of(example_edits(upto)))
    for seed in range(6):
        edits, directory = random_history(100 + seed, 25 + 10 * seed)
        add(f"history_{seed}", case_of(edits, directory if seed % 2 == 0 else None, lead=(seed, 1, 2)))
    for name, case, kw, want in damaged_cases():
        add("damaged_" + name, case, **kw)
        assert (out[-1][5]["status"], out[-1][5]["bad_kind"], out[-1][5]["bad_row"]) == want, name
    assert VS.TOTALS_WORDS == 38
    return out


def totals_words(t):
    return ([t[n] for n in ("records", "new_files", "deleted", "pointers", "live", "unplaced")] + t["level_files"] +
            t["level_bytes"] + t["compact_pointer"] +
            [t[n] for n in ("log_number", "prev_log_number", "next_file_number", "last_sequence", "comparator_off",
                            "comparator_len", "has", "max_file_number", "status", "bad_kind", "bad_row")])


def dump(path):
    """Every case as: 8 u64 (src bytes, records, file / deleted / pointer rows,
    directory entries, files_cap, rows expected), then src, the edits, the
    three tables each followed by its bounds, the directory, the 38 expected
    totals, the expected rows (64 bytes each) and indices (u32).  Returns the
    number of cases."""
    import lvgpu.version as V
    import lvgpu.version_set as VS
    cases = dump_cases()
    with open(path, "wb") as f:
        for name, (src, E, F, bf, D, bd, P, bp, dr), kw, rows, index, t in cases:
            pl = VS.placements(dr or [])
            f.write(struct.pack("<8Q", len(src), len(E), len(F), len(D), len(P), len(pl), kw["files_cap"], len(rows)))
            f.write(src)
            for a in (E, F, bf, D, bd, P, bp, pl):
                f.write(np.ascontiguousarray(a).tobytes())
            f.write(np.array(totals_words(t), dtype=np.uint64).tobytes())
            out = np.zeros(len(rows), dtype=V.FILE_DTYPE)
            for o, r in zip(out, rows):
                for n_, v in r.items():
                    o[n_] = v
            f.write(out.tobytes())
            f.write(np.array(index, dtype=np.uint32).tobytes())
    return len(cases)
