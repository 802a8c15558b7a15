"""tools/version_edit_hostcheck.cc, the stand-alone check of the VersionEdit host
twins, built with AddressSanitizer and UBSan from the sources its header
comment lists and run over the dump tests/version_edit_cases.py writes: records
with the model's answers (the example, its prefixes and flips, the quirks,
every status, random edits) and encode inputs with the model's verdicts, the
damaged ones among them.  The program has its own main(); nothing Python loads
is sanitized, and the child runs in the environment of the test, unchanged.
Needs no GPU."""
import os
import re
import subprocess

import lvgpu.version_edit as VE
import version_edit_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Iinclude"]
SOURCES = ["tools/version_edit_hostcheck.cc", "leveldb-rs_amd/csrc/version_edit.cc"]


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
    assert "tests/test_version_edit_hostcheck.py" in head
    exe = str(tmp_path / "version_edit_hostcheck")
    cmd = ["g++"] + FLAGS + SOURCES + ["-o", exe]
    b = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, " ".join(cmd) + "\n" + b.stdout
    # a build that dropped the flags must not pass: both runtimes are linked
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert libs.returncode == 0 and "libasan" in libs.stdout and "libubsan" in libs.stdout, libs.stdout
    dump = str(tmp_path / "version_edit_cases.bin")
    n = C.dump(dump)
    names = [c[0] for c in C.dump_cases()]
    assert n == len(names) > 300 and os.path.getsize(dump) > 0 and VE.EDIT_DTYPE.itemsize == 64
    assert {"prefix_0", "prefix_54", "flip_0_80", "flip_54_ff", "quirk_14", "status_6", "decode_model_5", "encode_example",
            "encode_empty", "encode_model_3", "damaged_bounds_order_file_0", "damaged_bounds_over_pointer_2",
            "damaged_pointer_extent_1", "damaged_file_extent_0", "damaged_comparator_extent_2", "damaged_has_0",
            "damaged_file_level_1", "damaged_deleted_order_2"} <= set(names)
    r = subprocess.run([exe, dump], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace")
    said = f"exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, said
    assert r.returncode == 0, said
    m = re.search(r"^version_edit_hostcheck: (\d+) cases replayed, (\d+) decodes, (\d+) encodes \((\d+) refused\), "
                  r"0 failures$", r.stdout, re.M)
    assert m, said
    cases, decodes, encodes, refused = (int(x) for x in m.groups())
    assert cases == n == decodes + encodes and decodes > 300 and refused == len(C.damaged_encode_inputs()) >= 30, said
