"""The host side of `svtrek call --rearrangements` without a GPU: the VCF writer (svth_format_calls_rearr through
host.format_calls) on hand-made records -- the <DUP> / <INV> lines, the per-type ranks, the header, and the text
for scans without rearrangements byte for byte what it was -- the same writer under ASan+UBSan in a stand-alone
program (tests/san/rearr_san.cpp; nothing is loaded into Python under a sanitizer), the public type parsers, and
the CLI on the CPU backend, which has no discovery."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from svtrek_amd import build, host
from svtrek_amd._lib import CALL_DTYPE, GT_DTYPE, SVT_DEL, SVT_DUP, SVT_INS, SVT_INV
from svtrek_amd.engine import call_type_bits, rearr_type_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_CLI = os.path.join(ROOT, "oracle", "_cpu", "svtrek_cpu")
ENV = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
TYPES = (SVT_DEL, SVT_INS, SVT_INV, SVT_DUP, 5)
MASKS = {(): 0, ("DUP",): 1 << SVT_DUP, ("INV",): 1 << SVT_INV, ("DUP", "INV"): (1 << SVT_DUP) | (1 << SVT_INV)}


def generated(n):
    """tests/san/rearr_san.cpp's records."""
    k = np.arange(n, dtype=np.int64)
    calls = np.zeros(n, dtype=CALL_DTYPE)
    calls["type"] = np.array(TYPES)[k % 5]
    calls["chrom"] = 1 + (k // 1000) % 4
    calls["pos"] = 100 + 7 * k
    calls["len"] = 50 + k % 977
    calls["end"] = calls["pos"] + calls["len"]
    calls["support"] = 3 + k % 5
    calls["depth"] = k % 60
    calls["len_lo"], calls["len_hi"] = calls["len"] - 1, calls["len"] + 2
    calls["x_lo"], calls["x_hi"] = calls["pos"] - 3, calls["pos"] + 4
    gts = np.zeros(n, dtype=GT_DTYPE)
    plain = (calls["type"] == SVT_DEL) | (calls["type"] == SVT_INS)
    gts["gt"] = np.where(plain, k % 3, -1)
    gts["alt"], gts["ref"], gts["gq"] = np.where(plain, k % 11, 0), np.where(plain, k % 7, 0), np.where(plain, k % 100, 0)
    gts["pl"][:, 0], gts["pl"][:, 2] = np.where(plain, k % 500, 0), np.where(plain, k % 300, 0)
    return calls, gts


def test_type_parsers():
    assert rearr_type_bits(()) == 0 and rearr_type_bits("") == 0
    assert rearr_type_bits("DUP") == 1 << SVT_DUP and rearr_type_bits(("inv", "DUP")) == MASKS[("DUP", "INV")]
    assert rearr_type_bits("DUP, INV") == MASKS[("DUP", "INV")]
    for bad in (("DEL",), "INS", ("DUP", "BND")):
        with pytest.raises(ValueError):
            rearr_type_bits(bad)
    with pytest.raises(ValueError):
        call_type_bits(("DUP",))                        # types keeps meaning DEL / INS only


def test_records_ranks_and_header():
    rows = [(SVT_INS, 1, 2000, 2001, 3, 9, 80, 80, 80, 2000, 2000, 0), (SVT_DEL, 1, 2000, 2301, 5, 9, 300, 300, 300, 2000, 2000, 0),
            (SVT_INV, 1, 2000, 2600, 3, 9, 600, 600, 600, 2000, 2000, 0), (SVT_DUP, 1, 2000, 2650, 6, 9, 650, 400, 900, 2000, 2000, 0),
            (SVT_DUP, 2, 800, 1200, 3, 4, 400, 400, 400, 800, 800, 0), (SVT_INV, 3, 7, 90, 3, 1, 83, 83, 83, 7, 7, 0)]
    calls = np.array(rows, dtype=CALL_DTYPE)
    names = ["chr1", "chr2"]
    text = host.format_calls(calls, names, rearrangements=("DUP", "INV"))
    head, body = text[:text.index("#CHROM")], text[text.index("#CHROM"):].split("\n")
    assert ('##ALT=<ID=DEL,Description="Deletion">\n##ALT=<ID=INS,Description="Insertion">\n'
            '##ALT=<ID=DUP,Description="Tandem duplication">\n##ALT=<ID=INV,Description="Inversion">\n##INFO=<ID=SVTYPE') in head
    assert body[1:] == [
        "chr1\t2000\tsvtrek.INS.1\tN\t<INS>\t.\tPASS\tSVTYPE=INS;END=2001;SVLEN=80;SUPPORT=3;DEPTH=9;XRANGE=2000,2000;LENRANGE=80,80",
        "chr1\t2000\tsvtrek.DEL.1\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=2301;SVLEN=-300;SUPPORT=5;DEPTH=9;XRANGE=2000,2000;LENRANGE=300,300",
        "chr1\t2000\tsvtrek.INV.1\tN\t<INV>\t.\tPASS\tSVTYPE=INV;END=2600;SVLEN=600;SUPPORT=3;DEPTH=9;XRANGE=2000,2000;LENRANGE=600,600",
        "chr1\t2000\tsvtrek.DUP.1\tN\t<DUP>\t.\tPASS\tSVTYPE=DUP;END=2650;SVLEN=650;SUPPORT=6;DEPTH=9;XRANGE=2000,2000;LENRANGE=400,900",
        "chr2\t800\tsvtrek.DUP.2\tN\t<DUP>\t.\tPASS\tSVTYPE=DUP;END=1200;SVLEN=400;SUPPORT=3;DEPTH=4;XRANGE=800,800;LENRANGE=400,400",
        "3\t7\tsvtrek.INV.2\tN\t<INV>\t.\tPASS\tSVTYPE=INV;END=90;SVLEN=83;SUPPORT=3;DEPTH=1;XRANGE=7,7;LENRANGE=83,83", ""]
    # the header names only what the scan asked for; the body does not depend on the header
    only = host.format_calls(calls, names, rearrangements=("INV",))
    assert "##ALT=<ID=INV" in only and "##ALT=<ID=DUP" not in only
    assert host.format_calls(calls, names, rearrangements="DUP,INV", header=False) == "\n".join(body[1:])
    # genotypes: the invalid record prints ./.
    gts = np.zeros(len(calls), dtype=GT_DTYPE)
    gts["gt"] = [1, 2, -1, -1, -1, -1]
    lines = host.format_calls(calls, names, genotypes=gts, sample="S", rearrangements=("DUP", "INV"), header=False).split("\n")
    assert lines[1].endswith("\tGT:GQ:DR:DV:PL\t1/1:0:0:0:0,0,0") and all(ln.endswith("\tGT:GQ:DR:DV:PL\t./.:0:0:0:0,0,0") for ln in lines[2:6])
    with pytest.raises(ValueError):
        host.format_calls(calls, names, rearrangements=("DUP",), consensus=(None, None))


def test_text_without_rearrangements_is_unchanged():
    """rearr == 0 is svth_format_calls_seq byte for byte, DEL / INS records do not depend on the mask, and the only
    difference the mask makes to a DEL / INS-only scan's text is the ##ALT lines it adds."""
    L = host.load_host()
    calls, gts = generated(3000)
    names = (C.c_char_p * 2)(b"chr1", b"chr2")
    for g in (None, gts.ctypes.data):
        n1, n2 = C.c_size_t(0), C.c_size_t(0)
        p1 = L.svth_format_calls_seq(calls.ctypes.data, g, None, None, 0, len(calls), names, 2, b"S1", 1, 3, C.byref(n1))
        p2 = L.svth_format_calls_rearr(calls.ctypes.data, g, None, None, 0, len(calls), names, 2, b"S1", 1, 3, 0, C.byref(n2))
        a, b = C.string_at(p1, n1.value), C.string_at(p2, n2.value)
        L.svth_free(p1)
        L.svth_free(p2)
        assert a == b and b"<DUP>" not in a and b"<INV>" not in a
    plain = calls[(calls["type"] == SVT_DEL) | (calls["type"] == SVT_INS)]
    old = host.format_calls(plain, ["chr1", "chr2"])
    assert old == host.format_calls(plain, ["chr1", "chr2"], rearrangements=())
    new = host.format_calls(plain, ["chr1", "chr2"], rearrangements=("DUP", "INV"))
    assert new.replace('##ALT=<ID=DUP,Description="Tandem duplication">\n##ALT=<ID=INV,Description="Inversion">\n', "") == old


@pytest.fixture(scope="module")
def driver():
    out_dir = os.path.join(ROOT, "build", "san")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "rearr_asan")
    src = [os.path.join(ROOT, "tests", "san", "rearr_san.cpp"), os.path.join(build.CSRC, "vcf_audit.cpp")]
    hdrs = [os.path.join(build.CSRC, "svtrek_host.h"), os.path.join(build.INC, "svtrek_call.h"), os.path.join(build.INC, "svtrek_rearr.h")]
    if build._stale(out, src + hdrs):
        build._run(["g++", "-O1", "-g", "-std=c++17", "-pthread", *build.SAN_FLAGS["asan"], "-I", build.INC, "-I", build.CSRC, "-o", out] +
                   src + ["-lz", "-ldl"])
    return out


@pytest.mark.parametrize("n, threads, gt", [(0, 1, 0), (7, 4, 1), (40000, 3, 0), (40000, 4, 1)])
@pytest.mark.parametrize("rearr", list(MASKS))
def test_writer_under_asan_ubsan(driver, rearr, n, threads, gt):
    """40 000 calls: three pieces formatted by three threads, the ranks carried from piece to piece."""
    p = subprocess.run([driver, str(n), str(MASKS[rearr]), str(threads), str(gt)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV,
                       timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-4000:]
    calls, gts = generated(n)
    want = host.format_calls(calls, ["chr1", "chr2"], genotypes=gts if gt else None, sample="S1", threads=threads, rearrangements=rearr)
    assert p.stdout.decode("latin-1") == want
    if n == 40000 and rearr == ("DUP", "INV"):
        assert f"svtrek.DUP.{n // 5}\t" in want and f"svtrek.INV.{n // 5}\t" in want and f"svtrek.INS.{2 * n // 5}\t" in want


def test_cli_on_the_cpu_backend_refuses(tmp_path):
    if not os.path.exists(CPU_CLI):
        pytest.fail(f"{CPU_CLI} not built (run __graft_entry__.build())")
    import test_junction_ingest as T
    bam = T.write(tmp_path / "x.bam", [T.rec(0, 1000, [(0, 100)])])
    p = subprocess.run([CPU_CLI, "call", "-b", bam, "--rearrangements", "DUP,INV"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode != 0 and "rearrangements: not supported by this backend" in p.stderr and p.stdout == ""
    p = subprocess.run([CPU_CLI, "call", "-b", bam, "--rearrangements", "DUP", "--ins-seq"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode != 0 and "--rearrangements cannot be combined with --ins-seq" in p.stderr
