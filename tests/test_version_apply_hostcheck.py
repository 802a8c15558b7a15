"""tools/version_apply_hostcheck.cc, the stand-alone check of the version
builder's host twin, built with AddressSanitizer and UBSan from the sources its
header comment lists and run over the dump tests/version_apply_cases.py writes:
the worked example and its prefixes, random histories and the damaged inputs
(bounds, extents, levels, numbers, duplicates, directories) with the model's
answers.  The program has its own main(); nothing Python loads is sanitized,
and the child runs in the environment of the test, unchanged.  Needs no GPU."""
import os
import re
import subprocess

import version_apply_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Iinclude"]
SOURCES = ["tools/version_apply_hostcheck.cc", "leveldb-rs_amd/csrc/version_set.cc"]


def test_hostcheck_under_sanitizers(tmp_path):
    with open(os.path.join(ROOT, SOURCES[0])) as f:
        head = []
        for line in f:
            if not line.startswith("//"):
                break
            head.append(line[2:])
    head = " ".join(head)
    # the header comment's recipe names exactly these sources and flags
    assert sorted(set(re.findall(r"(?<![\w/.])((?:tools|leveldb-rs_amd/csrc)/\w+\.cc)", head))) == sorted(SOURCES)
    for flag in FLAGS[:4]:
        assert flag in head, flag
    assert "tests/test_version_apply_hostcheck.py" in head
    exe = str(tmp_path / "version_apply_hostcheck")
    cmd = ["g++"] + FLAGS + SOURCES + ["-o", exe]
    b = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, " ".join(cmd) + "\n" + b.stdout
    # a build that dropped the flags must not pass: both runtimes are linked
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert libs.returncode == 0 and "libasan" in libs.stdout and "libubsan" in libs.stdout, libs.stdout
    dump = str(tmp_path / "version_apply_cases.bin")
    n = C.dump(dump)
    cases = C.dump_cases()
    names = [c[0] for c in cases]
    assert n == len(names) > 35 and os.path.getsize(dump) > 0
    assert {"empty", "example_1", "example_6", "history_0", "history_5", "damaged_bounds_order_file",
            "damaged_bounds_over_deleted", "damaged_pointer_extent", "damaged_file_smallest_extent",
            "damaged_file_largest_extent", "damaged_file_largest_short", "damaged_deleted_number", "damaged_duplicate",
            "damaged_directory_swapped", "damaged_directory_equal", "damaged_file_over"} <= set(names)
    r = subprocess.run([exe, dump], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace")
    said = f"exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, said
    assert r.returncode == 0, said
    m = re.search(r"^version_apply_hostcheck: (\d+) cases replayed, (\d+) refused, (\d+) retried one row short, "
                  r"(\d+) live rows, 0 failures$", r.stdout, re.M)
    assert m, said
    replayed, refused, overs, live = (int(x) for x in m.groups())
    assert replayed == n and refused == len(C.damaged_cases()) >= 25 and overs >= 10 and live > 100, said
