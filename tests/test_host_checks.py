"""The stand-alone host check programs (tools/*_host_check.cc and
tools/wal_layout_check.cc), built with AddressSanitizer and UBSan and run: the
serial cores a lane also executes (csrc/lvk/sst_read.h, version_read.h,
sst_scan.h) and the host twins the GPU tests use as references must stay
inside their buffers whatever the bytes say, and a read outside that changes
no answer shows nowhere else.  Each program is built from the sources its
header comment lists (PROGRAMS below mirrors the comments, and the test holds
the two together) and, where it replays a dump, gets the one its case module
writes: the inputs the GPU tests replay.  These are programs with their own
main(); nothing Python loads is sanitized, and a child runs in the
environment of the test, unchanged.  Needs no GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "leveldb-rs_amd/csrc/"
FLAGS = ["-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Iinclude"]

# program -> (the sources after tools/<program>.cc, the case module whose dump() it replays, its line of success)
_READER = ["sst_get.cc", "sst_build.cc", "sst_format.cc", "memtable.cc", "crc32c_scalar.cc"]
PROGRAMS = {
    "mt_host_check": (["memtable.cc"], None, r"^mt_host_check: ok$"),
    "wb_host_check": (["write_batch.cc"], None, r"^wb_host_check ok$"),
    "compact_host_check": (["compact.cc", "memtable.cc"], None, r"^\d+ calls; 0 failures$"),
    "sst_host_check": (["sst_build.cc", "sst_format.cc", "memtable.cc", "crc32c_scalar.cc"], None, r"^sst_host_check: ok$"),
    "sst_get_host_check": (_READER, "sst_get_cases", r"^sst_get_host_check: ok$"),
    "sst_scan_host_check": (["sst_scan.cc"] + _READER, "sst_scan_cases",
                            r"^\d+ scans: \d+ with status 0, \d+ CORRUPT; 0 failures$"),
    "sst_bloom_host_check": (_READER, "sst_bloom_cases", r"^sst_bloom_host_check: ok$"),
    "version_host_check": (["version.cc"], "version_cases",
                           r"^version_host_check: [1-9]\d* cases, [1-9]\d* queries replayed, 0 failures$"),
    "wal_layout_check": (["wal_layout.cc"], None, r"^wal_layout_check: [1-9]\d* layouts ok$"),
}
REPLAYED = {"sst_get_host_check": r"^sst_get_host_check: replayed [1-9]\d* cases, [1-9]\d* queries$",
            "sst_bloom_host_check": r"^sst_bloom_host_check: replayed [1-9]\d* cases, [1-9]\d* queries$"}


def _sources(name):
    return [f"tools/{name}.cc"] + [CSRC + s for s in PROGRAMS[name][0]]


@pytest.fixture(scope="session")
def builds(tmp_path_factory):
    """Every program's compile, started at once (each takes a few seconds on
    one core); a test waits for its own."""
    out = tmp_path_factory.mktemp("host_checks")
    jobs = {}
    for name in PROGRAMS:
        exe, log = str(out / name), open(out / (name + ".build.txt"), "w+")
        cmd = ["g++"] + FLAGS + _sources(name) + ["-o", exe]
        jobs[name] = (subprocess.Popen(cmd, cwd=ROOT, stdout=log, stderr=subprocess.STDOUT), log, exe, cmd)
    yield out, jobs
    for p, log, _, _ in jobs.values():
        p.wait()
        log.close()


def test_the_table_is_the_nine_programs():
    tools = os.listdir(os.path.join(ROOT, "tools"))
    assert sorted(PROGRAMS) == sorted(t[:-3] for t in tools if t.endswith(("_host_check.cc", "_layout_check.cc")))
    assert len(PROGRAMS) == 9


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_host_check_under_sanitizers(builds, name):
    out, jobs = builds
    _, cases, ok_line = PROGRAMS[name]
    # the header comment's recipe names exactly these sources and flags
    with open(os.path.join(ROOT, "tools", name + ".cc")) as f:
        head = []
        for line in f:
            if not line.startswith("//"):
                break
            head.append(line[2:])
    head = " ".join(head)
    assert sorted(set(re.findall(r"(?<![\w/.])((?:tools|leveldb-rs_amd/csrc)/\w+\.cc)", head))) == sorted(_sources(name)), name
    for flag in FLAGS[:4]:
        assert flag in head, (name, flag)
    assert "tests/test_host_checks.py" in head, name
    proc, log, exe, cmd = jobs[name]
    rc = proc.wait()
    log.seek(0)
    assert rc == 0, " ".join(cmd) + "\n" + log.read()
    # a build that dropped the flags must not pass: both runtimes are linked
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert libs.returncode == 0 and "libasan" in libs.stdout and "libubsan" in libs.stdout, libs.stdout
    args = [exe]
    if cases:
        dump = str(out / (cases + ".bin"))
        assert __import__(cases).dump(dump) > 0 and os.path.getsize(dump) > 0
        args.append(dump)
    r = subprocess.run(args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace")
    said = f"{name}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, said
    assert r.returncode == 0, said
    assert re.search(ok_line, r.stdout, re.M), said
    if name in REPLAYED:
        assert re.search(REPLAYED[name], r.stdout, re.M), said
