"""The junction classifier (svtrek_amd/csrc/svt_jnclass.h) under ASan+UBSan: tests/san/jnclass_san.cpp, a stand-alone
program, classifies the seeded table and the extreme-value table of tests/native/jnclass_shim.cpp and must exit
clean and print the digests the uninstrumented shim gives.  The program is compiled here and run directly; nothing
is loaded into Python under a sanitizer."""
import ctypes as C
import os
import subprocess

import pytest

from svtrek_amd import build

from test_jnclass_model import LIM, RECORDS, SEED, shim  # noqa: F401  (the uninstrumented build)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def driver():
    out_dir = os.path.join(ROOT, "build", "san")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "jnclass_asan")
    src = os.path.join(ROOT, "tests", "san", "jnclass_san.cpp")
    deps = [src, os.path.join(ROOT, "tests", "native", "jnclass_shim.cpp"), os.path.join(build.CSRC, "svt_jnclass.h"),
            os.path.join(build.INC, "svtrek_junction.h")]
    if build._stale(out, deps):
        build._run(["g++", "-O1", "-g", "-std=c++17", *build.SAN_FLAGS["asan"], "-I", build.CSRC, "-o", out, src])
    return out


def test_classifier_under_sanitizers(shim, driver):  # noqa: F811
    buf = C.create_string_buffer(1024)
    assert shim.jc_digest(LIM.ctypes.data, SEED, RECORDS, buf, len(buf)) > 0
    p = subprocess.run([driver, str(SEED), str(RECORDS), *(str(int(v)) for v in LIM)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=ENV, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-4000:]
    assert p.stdout.decode() == buf.value.decode()
    assert p.stdout.count(b"\n") == 3 and p.stdout.startswith(b"seeded ")
