"""The load's host pass (svtrek_amd/csrc/svt_loadprep.h) under ASan+UBSan and under TSan: tests/san/loadprep_san.cpp,
a stand-alone program, runs both functions on a seeded pileup on 16 threads and must exit clean and print the
digests the uninstrumented shim gives for the same seed.  The program is compiled here and run directly; nothing is
loaded into Python under a sanitizer."""
import ctypes as C
import os
import subprocess

import pytest

from svtrek_amd import build

from test_loadprep_model import shim  # noqa: F401  (the uninstrumented build)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
SEED = 20240611


@pytest.fixture(scope="module", params=["asan", "tsan"])
def driver(request):
    out_dir = os.path.join(ROOT, "build", "san")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, f"loadprep_{request.param}")
    src = os.path.join(ROOT, "tests", "san", "loadprep_san.cpp")
    deps = [src, os.path.join(ROOT, "tests", "native", "loadprep_shim.cpp"), os.path.join(build.CSRC, "svt_loadprep.h")]
    if build._stale(out, deps):
        build._run(["g++", "-O1", "-g", "-std=c++17", "-pthread", *build.SAN_FLAGS[request.param], "-I", build.CSRC, "-o", out, src])
    return out


def test_host_pass_under_sanitizers(shim, driver):  # noqa: F811
    buf = C.create_string_buffer(8192)
    assert shim.lp_seeded_digest(SEED, 16, buf, len(buf)) > 0
    p = subprocess.run([driver, str(SEED), "16"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-4000:]
    assert p.stdout.decode() == buf.value.decode()
    assert p.stdout.count(b"\n") == 22
