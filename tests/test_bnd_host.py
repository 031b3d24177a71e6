"""The host side of `svtrek call --breakends` without a GPU: the VCF writer (svth_format_calls_bnd through
host.format_calls) on hand-made records -- the four ALT forms, the partner's name, the per-type ranks, the header,
and the text for scans without breakends byte for byte what it was -- the same writer under ASan+UBSan in a
stand-alone program (tests/san/bnd_san.cpp; nothing is loaded into Python under a sanitizer), the pad helper, and
the CLI on the CPU backend: `call --breakends` is refused there, and `audt` of a BND VCF treats its BND lines as
it treats any SVTYPE=BND line."""
import ctypes as C
import os
import subprocess

import numpy as np
import oracle_ffi as O
import pytest

from svtrek_amd import build, host
from svtrek_amd._lib import CALL_DTYPE, GT_DTYPE, SVT_BND, SVT_DEL, SVT_DUP, SVT_INS, SVT_INV, SVT_NA, bind_abi, call_mate, has_bnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libsvtrek_cpu.so")
CPU_CLI = os.path.join(ROOT, "oracle", "_cpu", "svtrek_cpu")
ENV = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
TYPES = (SVT_DEL, SVT_BND, SVT_INS, SVT_INV, SVT_DUP, 5)
BOTH = (1 << SVT_DUP) | (1 << SVT_INV)
NAMES5 = ["chr1", "chr2", "chr3", "chr4", "chr5"]
ROWS = [(SVT_INS, 1, 2000, 2001, 3, 9, 80, 80, 80, 2000, 2000, 0), (SVT_DEL, 1, 2000, 2301, 5, 9, 300, 300, 300, 2000, 2000, 0),
        (SVT_DUP, 1, 2000, 2650, 6, 9, 650, 400, 900, 2000, 2000, 0),
        (SVT_BND, 1, 2000, 7000, 3, 9, 0, 6999, 7002, 1998, 2003, 5 << 2 | 1), (SVT_BND, 1, 2000, 7000, 4, 9, 0, 7000, 7000, 2000, 2000, 2 << 2 | 0),
        (SVT_BND, 2, 10, 20, 3, 0, 0, 20, 20, 10, 10, 9 << 2 | 2), (SVT_BND, 7, 10, 20, 3, 0, 0, 20, 20, 10, 10, 4 << 2 | 3)]
BODY = [
    "chr1\t2000\tsvtrek.INS.1\tN\t<INS>\t.\tPASS\tSVTYPE=INS;END=2001;SVLEN=80;SUPPORT=3;DEPTH=9;XRANGE=2000,2000;LENRANGE=80,80",
    "chr1\t2000\tsvtrek.DEL.1\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=2301;SVLEN=-300;SUPPORT=5;DEPTH=9;XRANGE=2000,2000;LENRANGE=300,300",
    "chr1\t2000\tsvtrek.DUP.1\tN\t<DUP>\t.\tPASS\tSVTYPE=DUP;END=2650;SVLEN=650;SUPPORT=6;DEPTH=9;XRANGE=2000,2000;LENRANGE=400,900",
    "chr1\t2000\tsvtrek.BND.1\tN\tN[chr5:7000[\t.\tPASS\tSVTYPE=BND;CHR2=chr5;POS2=7000;SUPPORT=3;DEPTH=9;XRANGE=1998,2003;X2RANGE=6999,7002",
    "chr1\t2000\tsvtrek.BND.2\tN\tN]chr2:7000]\t.\tPASS\tSVTYPE=BND;CHR2=chr2;POS2=7000;SUPPORT=4;DEPTH=9;XRANGE=2000,2000;X2RANGE=7000,7000",
    "chr2\t10\tsvtrek.BND.3\tN\t]9:20]N\t.\tPASS\tSVTYPE=BND;CHR2=9;POS2=20;SUPPORT=3;DEPTH=0;XRANGE=10,10;X2RANGE=20,20",
    "7\t10\tsvtrek.BND.4\tN\t[chr4:20[N\t.\tPASS\tSVTYPE=BND;CHR2=chr4;POS2=20;SUPPORT=3;DEPTH=0;XRANGE=10,10;X2RANGE=20,20", ""]
BND_INFO = ('##INFO=<ID=CHR2,Number=1,Type=String,Description="BND: the partner breakend\'s contig">\n'
            '##INFO=<ID=POS2,Number=1,Type=Integer,Description="BND: rounded mean of the partner breakend\'s position">\n'
            '##INFO=<ID=X2RANGE,Number=2,Type=Integer,Description="BND: smallest and largest partner position of the supporting reads">\n')


def generated(n):
    """tests/san/bnd_san.cpp's records."""
    k = np.arange(n, dtype=np.int64)
    calls = np.zeros(n, dtype=CALL_DTYPE)
    calls["type"] = np.array(TYPES)[k % 6]
    bnd = calls["type"] == SVT_BND
    calls["chrom"] = 1 + (k // 1000) % 4
    calls["pos"] = 100 + 7 * k
    calls["len"] = np.where(bnd, 0, 50 + k % 977)
    calls["end"] = calls["pos"] + 50 + k % 977
    calls["support"] = 3 + k % 5
    calls["depth"] = k % 60
    calls["len_lo"], calls["len_hi"] = calls["end"] - 1, calls["end"] + 2
    calls["x_lo"], calls["x_hi"] = calls["pos"] - 3, calls["pos"] + 4
    calls["pad"] = np.where(bnd, (1 + (k // 7) % 5) << 2 | (k // 6) % 4, 0)
    gts = np.zeros(n, dtype=GT_DTYPE)
    plain = (calls["type"] == SVT_DEL) | (calls["type"] == SVT_INS)
    gts["gt"] = np.where(plain, k % 3, -1)
    gts["alt"], gts["ref"], gts["gq"] = np.where(plain, k % 11, 0), np.where(plain, k % 7, 0), np.where(plain, k % 100, 0)
    gts["pl"][:, 0], gts["pl"][:, 2] = np.where(plain, k % 500, 0), np.where(plain, k % 300, 0)
    return calls, gts


def test_pad_helper():
    calls = np.array(ROWS, dtype=CALL_DTYPE)
    mc, o = call_mate(calls[3:])
    assert mc.tolist() == [5, 2, 9, 4] and o.tolist() == [1, 0, 2, 3]


def test_records_ranks_and_header():
    calls = np.array(ROWS, dtype=CALL_DTYPE)
    text = host.format_calls(calls, NAMES5, rearrangements=("DUP",), breakends=True)
    head, body = text[:text.index("#CHROM")], text[text.index("#CHROM"):].split("\n")
    assert body[0] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" and body[1:] == BODY
    assert head.endswith('Description="Smallest and largest length of the supporting ops">\n' + BND_INFO)
    assert "##ALT=<ID=BND" not in head and '##ALT=<ID=DUP,Description="Tandem duplication">\n##INFO=<ID=SVTYPE' in head
    for line in BODY[3:7]:                                   # no END key, and no key that ends in END=
        assert "END=" not in line
    assert "END=" not in BND_INFO
    assert host.format_calls(calls, NAMES5, rearrangements="DUP", breakends=True, header=False) == "\n".join(BODY)
    # without rearrangements the DUP record is an INS record as ever, the BND records are unchanged
    lines = host.format_calls(calls, NAMES5, breakends=True, header=False).split("\n")
    assert lines[2].startswith("chr1\t2000\tsvtrek.INS.2\tN\t<INS>\t") and lines[3:] == BODY[3:]
    # genotypes: ./. whatever the record says
    gts = np.zeros(len(calls), dtype=GT_DTYPE)
    gts["gt"] = [1, 2, -1, -1, 1, -1, -1]
    lines = host.format_calls(calls, NAMES5, genotypes=gts, sample="S", rearrangements=("DUP",), breakends=True).split("\n")
    assert "##FORMAT=<ID=GT" in "\n".join(lines) and lines[-9] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"
    assert lines[-7].endswith("\tGT:GQ:DR:DV:PL\t1/1:0:0:0:0,0,0")
    assert all(ln == b + "\tGT:GQ:DR:DV:PL\t./.:0:0:0:0,0,0" for ln, b in zip(lines[-6:-1], BODY[2:7]))
    with pytest.raises(ValueError):
        host.format_calls(calls, NAMES5, breakends=True, consensus=(None, None))


def test_text_without_breakends_is_unchanged():
    """bnd == 0 is svth_format_calls_rearr byte for byte on a list of every type, for every mask; the only
    difference bnd makes to a scan's text without a BND call is the three ##INFO lines."""
    L = host.load_host()
    calls, gts = generated(3000)
    names = (C.c_char_p * 2)(b"chr1", b"chr2")
    for rearr in (0, 1 << SVT_DUP, BOTH):
        for g in (None, gts.ctypes.data):
            n1, n2 = C.c_size_t(0), C.c_size_t(0)
            p1 = L.svth_format_calls_rearr(calls.ctypes.data, g, None, None, 0, len(calls), names, 2, b"S1", 1, 3, rearr, C.byref(n1))
            p2 = L.svth_format_calls_bnd(calls.ctypes.data, g, None, None, 0, len(calls), names, 2, b"S1", 1, 3, rearr, 0, C.byref(n2))
            a, b = C.string_at(p1, n1.value), C.string_at(p2, n2.value)
            L.svth_free(p1)
            L.svth_free(p2)
            assert a == b and b"SVTYPE=BND" not in a and b"CHR2" not in a
    mixed = host.format_calls(calls, ["chr1", "chr2"], genotypes=gts, rearrangements=("DUP", "INV"))
    assert mixed == host.format_calls(calls, ["chr1", "chr2"], genotypes=gts, rearrangements=("DUP", "INV"), breakends=False)
    rest = calls[calls["type"] != SVT_BND]
    old = host.format_calls(rest, ["chr1", "chr2"], rearrangements=("DUP", "INV"))
    new = host.format_calls(rest, ["chr1", "chr2"], rearrangements=("DUP", "INV"), breakends=True)
    assert new != old and new.replace(BND_INFO, "") == old


@pytest.fixture(scope="module")
def driver():
    out_dir = os.path.join(ROOT, "build", "san")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "bnd_asan")
    src = [os.path.join(ROOT, "tests", "san", "bnd_san.cpp"), os.path.join(build.CSRC, "vcf_audit.cpp")]
    hdrs = [os.path.join(build.CSRC, "svtrek_host.h"), os.path.join(build.INC, "svtrek_call.h"), os.path.join(build.INC, "svtrek_bnd.h")]
    if build._stale(out, src + hdrs):
        build._run(["g++", "-O1", "-g", "-std=c++17", "-pthread", *build.SAN_FLAGS["asan"], "-I", build.INC, "-I", build.CSRC, "-o", out] +
                   src + ["-lz", "-ldl"])
    return out


@pytest.mark.parametrize("n, threads, gt", [(0, 1, 0), (7, 4, 1), (40000, 3, 0), (40000, 4, 1)])
@pytest.mark.parametrize("rearr, bnd", [(0, 1), (BOTH, 1), (BOTH, 0)])
def test_writer_under_asan_ubsan(driver, rearr, bnd, n, threads, gt):
    """40 000 calls: three pieces formatted by three threads, the ranks carried from piece to piece."""
    p = subprocess.run([driver, str(n), str(rearr), str(bnd), str(threads), str(gt)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=ENV, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-4000:]
    calls, gts = generated(n)
    want = host.format_calls(calls, ["chr1", "chr2"], genotypes=gts if gt else None, sample="S1", threads=threads,
                             rearrangements=("DUP", "INV") if rearr else (), breakends=bool(bnd))
    assert p.stdout.decode("latin-1") == want
    if n == 40000 and bnd:
        assert f"svtrek.BND.{(n + 4) // 6}\t" in want and f"svtrek.BND.{(n + 4) // 6 + 1}\t" not in want


def test_cli_on_the_cpu_backend_refuses(tmp_path):
    if not os.path.exists(CPU_CLI):
        pytest.fail(f"{CPU_CLI} not built (run __graft_entry__.build())")
    assert not has_bnd(bind_abi(C.CDLL(CPU_LIB)))
    import test_junction_ingest as T
    bam = T.write(tmp_path / "x.bam", [T.rec(0, 1000, [(0, 100)])])
    p = subprocess.run([CPU_CLI, "call", "-b", bam, "--breakends"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode != 0 and "[ERROR] breakends: not supported by this backend" in p.stderr and p.stdout == ""
    p = subprocess.run([CPU_CLI, "call", "-b", bam, "--breakends", "--ins-seq"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode != 0 and "--breakends cannot be combined with --ins-seq" in p.stderr and p.stdout == ""
    p = subprocess.run([CPU_CLI, "call", "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert "--breakends" in p.stdout


def test_audt_of_a_bnd_vcf_on_the_cpu_backend(tmp_path):
    """The writer's BND lines through `svtrek audt`: parsed as type BND with no END (its end is what any line without
    one gets), reported as an unknown type and refined to NA NA -- what a hand-written SVTYPE=BND line gets -- while the
    DEL line beside them is audited as ever; the text equals the oracle's."""
    import test_junction_ingest as T
    from test_cpu_backend import cpu_engine
    from svtrek_amd import from_reads
    bam = T.write(tmp_path / "x.bam", [T.rec(0, 1000, [(0, 1000), (2, 300), (0, 700)])] * 3)
    calls = np.array(ROWS, dtype=CALL_DTYPE)
    text = host.format_calls(calls, NAMES5, rearrangements=("DUP",), breakends=True)
    hand = "chr1\t2000\t.\tN\tN[chr5:7000[\t.\tPASS\tSVTYPE=BND\n"
    vcf = tmp_path / "b.vcf"
    vcf.write_text(text + hand)
    loci = host.parse_vcf_text(vcf.read_bytes())[0]
    p = subprocess.run([CPU_CLI, "audt", "-b", bam, "-v", str(vcf)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    pl = from_reads(3, [(0, 1000, [(0, 1000), (2, 300), (0, 700)])] * 3, clip={})
    assert p.stdout == O.audit_text(vcf.read_text(), pl)
    assert p.stderr.count("[ERROR] Unkown type.") == 6 and "BND" not in p.stdout          # DUP, four BND lines, the hand-written one
    assert [ln[:5] for ln in p.stdout.split("\n") if ln.startswith("(")] == ["(INS)", "(DEL)"]
    is_bnd = loci["type"] == SVT_BND
    b = loci[is_bnd]
    assert len(b) == 5 and b[0] == b[4]                        # BND.1 parses as the hand-written line at its place does
    assert (b["end"].astype(np.int64) - b["pos"] == int(b["end"][4]) - int(b["pos"][4])).all()   # no key taken for END
    with cpu_engine() as e:
        e.load_pileup(pl)
        res = e.refine(loci)
    assert (res["start"][is_bnd] == SVT_NA).all() and (res["end"][is_bnd] == SVT_NA).all()     # NA NA
    assert np.array_equal(res[is_bnd][:4], np.repeat(res[is_bnd][4:], 4))
