"""The SA ingest of bam_ingest.cpp under ASan+UBSan: tests/san/junction_san.cpp, a stand-alone program
linked with bam_ingest.cpp, reads every BAM of tests/test_junction_ingest.py -- the malformed ones included --
and must exit clean and print the table the uninstrumented library gives.  The program is compiled here and
run directly; nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import pytest

from svtrek_amd import build, host

import test_junction_ingest as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def driver():
    out_dir = os.path.join(ROOT, "build", "san")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "junction_asan")
    src = [os.path.join(ROOT, "tests", "san", "junction_san.cpp"), os.path.join(build.CSRC, "bam_ingest.cpp")]
    hdrs = [os.path.join(build.CSRC, "svtrek_host.h"), os.path.join(build.CSRC, "svt_bamrec.h"), os.path.join(build.INC, "svtrek_junction.h")]
    if build._stale(out, src + hdrs):
        build._run(["g++", "-O1", "-g", "-std=c++17", "-pthread", *build.SAN_FLAGS["asan"], "-I", build.INC, "-I", build.CSRC, "-o", out] +
                   src + ["-lz", "-ldl"])
    return out


def expected(path, region):
    pl, info, (read, off, seg) = host.read_bam(path, threads=3, junctions=True, region=region)
    lines = [f"reads {pl.n_reads} records {len(read)} malformed {info['sa_malformed']}"]
    for k in range(len(read)):
        for s in seg[int(off[k]):int(off[k + 1])]:
            lines.append(" ".join(str(int(v)) for v in (read[k], s["tid"], s["strand"], s["r_beg"], s["r_end"], s["q_beg"], s["q_end"])))
    return lines


@pytest.mark.parametrize("name", ["aux", "unsorted", "whole", "region", "malformed"])
def test_sa_ingest_under_asan_ubsan(tmp_path, driver, name):
    path, _, _, malformed, region = T.files(tmp_path)[name]
    args = [driver, path, "3"] + ([str(x) for x in region] if region else [])
    p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-4000:]
    got = p.stdout.decode().split("\n")[:-1]
    assert got == expected(path, region)
    assert got[0].endswith(f"malformed {malformed}")
