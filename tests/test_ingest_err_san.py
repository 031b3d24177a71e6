"""The error exits of bam_ingest.cpp under ASan+UBSan with the leak checker on: tests/san/ingest_err_san.cpp, a
stand-alone program linked with bam_ingest.cpp (svtrek_amd.build.build_sanitizers), calls svth_bam_read,
svth_bam_read_region, svth_bam_read_seq, svth_bam_read_sa and svth_bam_read_device on every crafted file of
tests/test_ingest_errors.py.  Each call must fail with the message named there and the run must end clean: no
leak of the pileup, the file, the batch buffers or the helper thread's batch on any exit.  The program is
compiled here and run directly; nothing is loaded into Python under a sanitizer."""
import subprocess

import pytest

from svtrek_amd import build

import test_ingest_errors as T
from test_sanitizers import ENV


@pytest.fixture(scope="module")
def driver():
    return build.build_sanitizers()["ingest_err_asan"]


@pytest.mark.parametrize("name", list(T.ROWS))
def test_error_exit_is_clean_under_asan_ubsan(tmp_path, driver, name):
    path, region = T.write_row(tmp_path, name)
    want_host, _, want_device = T.ROWS[name][3:]
    args = [driver, path, "4"] + ([str(x) for x in region] if region else [])
    p = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-4000:]
    got = dict(line.split(": ", 1) for line in p.stdout.decode().replace(path, "{path}").splitlines())
    want = {k: want_host for k in (("region", "seq", "sa") if region else ("read", "region", "seq", "sa"))}
    if not region:   # the program's sink takes every batch unread, so damage inside the records passes it
        want["device"] = "ok" if name in T.RECORD_ROWS else want_device
    assert got == want
