"""tests/callseq_ref.py, the numpy model of include/svtrek_callseq.h, on hand-built pileups with the answers
written out; the header's claim that a call's items are exactly the ops the scan counted (item count ==
call.support for call_ref / call_split_ref at len_permille 0 and 100, on the fuzz pileups); and the VCF
formatter of `svtrek call --ins-seq` (svth_format_calls_seq).  No GPU."""
import numpy as np
import pytest

from svtrek_amd import from_reads, host
from svtrek_amd._lib import CALL_DTYPE, POA_RESULT_DTYPE, SVT_DEL, SVT_INS

import call_ref
import call_split_ref
import callseq_ref
import fuzz

M, I, D, N, S, H = 0, 1, 2, 3, 4, 5


def test_items_indices_and_reach_worked_example():
    # read 0 (pos 100): I60 at x 150, I49 (no item), I80 at x 250; read 1 (pos 120): leading S and H, I50 at x 120 + 7;
    # contig 1's read (pos 10): I70 at x 10 (first op)
    reads = [(0, 100, [(M, 50), (I, 60), (M, 40), (I, 49), (D, 60), (I, 80), (M, 5)]),
             (0, 120, [(S, 9), (H, 7), (I, 50), (M, 30)]),
             (1, 10, [(I, 70), (M, 20)])]
    pl = from_reads(2, reads, clip={})
    it = callseq_ref.ins_items(pl)
    assert [a.tolist() for a in it[0]] == [[150, 250, 127], [60, 80, 50], [0, 1, 2], [100, 100, 120]]
    assert [a.tolist() for a in it[1]] == [[10], [70], [3], [10]]
    assert callseq_ref.reach(pl) == 150
    call = np.zeros(1, dtype=CALL_DTYPE)
    call[0] = (SVT_INS, 1, 150, 151, 1, 1, 60, 50, 60, 127, 150, 0)
    assert callseq_ref.call_items(it, call[0]).tolist() == [0, 2]
    assert callseq_ref.call_support(it, call[0], max_len=55)[0] == 1
    n, ks = callseq_ref.call_support(it, call[0], max_support=1)
    assert n == 2 and ks.tolist() == [0]
    call[0]["chrom"] = 2
    assert callseq_ref.call_items(it, call[0]).tolist() == []


def test_saturated_items_belong_to_no_call():
    reads = [(0, 5, [(H, (1 << 28) - 1)] * 4 + [(M, 10), (I, 60), (M, 1)]), (0, 7, [(M, 3), (I, 60), (M, 1)])]
    pl = from_reads(1, reads, clip={})
    it = callseq_ref.ins_items(pl)
    assert it[0][0].tolist() == [1 << 30, 10]
    assert callseq_ref.reach(pl) == 3
    call = np.zeros(1, dtype=CALL_DTYPE)
    call[0] = (SVT_INS, 1, 0, 0, 0, 0, 60, 0, 100, 0, 0xFFFFFFFF, 0)
    assert callseq_ref.call_items(it, call[0]).tolist() == [1]


def test_consensus_of_identical_sequences_and_del_record():
    rng = np.random.default_rng(3)
    allele = rng.integers(0, 4, 70).astype(np.uint8)
    reads = [(0, 1000, [(M, 500), (I, 70), (M, 800)])] * 4 + [(0, 1100, [(M, 300), (D, 90), (M, 700)])] * 3
    pl = from_reads(1, reads, clip={})
    calls = call_ref.call(pl)[0]
    assert [int(t) for t in calls["type"]] == [SVT_DEL, SVT_INS]
    off = np.arange(5, dtype=np.uint64) * 70
    res, seqs = callseq_ref.consensus(pl, calls, off, np.tile(allele, 4))
    assert [tuple(int(v) for v in r) for r in res] == [(-1, 0, 0, 0), (70, 4, 4, 0)]
    assert np.array_equal(seqs[1], allele) and len(seqs[0]) == 0
    res, _ = callseq_ref.consensus(pl, calls, off, np.tile(allele, 4), max_len=69)
    assert tuple(int(v) for v in res[1]) == (0, 0, 0, 0)
    res, _ = callseq_ref.consensus(pl, calls, off, np.tile(allele, 4), max_support=3, max_seqs=2)
    assert tuple(int(v) for v in res[1]) == (70, 4, 2, 0)
    assert callseq_ref.padded(seqs, 10).shape == (2, 10) and np.array_equal(callseq_ref.padded(seqs, 10)[1], allele[:10])


@pytest.mark.parametrize("seed, n_reads, max_ops", [(901, 400, 60), (905, 120, 600)], ids=["short901", "long905"])
@pytest.mark.parametrize("P", [0, 100])
def test_item_count_is_the_calls_support(seed, n_reads, max_ops, P):
    rng = np.random.default_rng(seed)
    hot = [int(x) for x in rng.integers(5000, 55000, size=5)]
    pl = fuzz.random_pileup(rng, n_targets=2, contig_len=60000, n_reads=n_reads, max_ops=max_ops, hot=hot)
    it = callseq_ref.ins_items(pl)
    n_ins = 0
    for ms in (1, 3):
        for link in (10, 200):
            calls = call_ref.call(pl, link, ms)[0] if P == 0 else call_split_ref.call(pl, link, ms, len_permille=P)[0]
            for c in calls:
                if int(c["type"]) == SVT_INS:
                    n_ins += 1
                    assert len(callseq_ref.call_items(it, c)) == int(c["support"]), c
    assert n_ins > 20


# ---------------------------------------------------------------- the formatter
def fmt_calls():
    calls = np.zeros(4, dtype=CALL_DTYPE)
    calls[0] = (SVT_DEL, 1, 500, 581, 3, 9, 80, 80, 80, 500, 500, 0)
    calls[1] = (SVT_INS, 1, 500, 501, 3, 9, 6, 6, 6, 500, 500, 0)
    calls[2] = (SVT_INS, 2, 900, 901, 4, 5, 300, 290, 310, 898, 902, 0)
    calls[3] = (SVT_INS, 2, 990, 991, 4, 5, 300, 290, 310, 988, 992, 0)
    res = np.zeros(4, dtype=POA_RESULT_DTYPE)
    res[0] = (-1, 0, 0, 0)
    res[1] = (6, 3, 3, 0)
    res[2] = (9, 4, 2, 0)          # longer than cap 8: <INS> stays
    res[3] = (0, 4, 0, 0)          # no consensus
    bases = np.zeros((4, 8), dtype=np.uint8)
    bases[1, :6] = [0, 1, 2, 3, 4, 0]
    bases[2] = 3
    return calls, res, bases


def test_format_alt_and_info():
    calls, res, bases = fmt_calls()
    plain = host.format_calls(calls, ["chrA", "chrB"]).splitlines()
    got = host.format_calls(calls, ["chrA", "chrB"], consensus=(res, bases)).splitlines()
    head = [ln for ln in got if ln.startswith("#")]
    assert [ln for ln in head if "CONS" in ln] == [
        '##INFO=<ID=CONSLEN,Number=1,Type=Integer,Description="INS: length of the consensus inserted sequence (0: none)">',
        '##INFO=<ID=CONSREADS,Number=1,Type=Integer,Description="INS: inserted sequences fused into the consensus">']
    assert [ln for ln in head if "CONS" not in ln] == [ln for ln in plain if ln.startswith("#")]
    assert head[-1].startswith("#CHROM") and "CONS" in head[-2] and "CONS" in head[-3]
    rec = [ln.split("\t") for ln in got if not ln.startswith("#")]
    old = [ln.split("\t") for ln in plain if not ln.startswith("#")]
    assert rec[0] == old[0]                                            # DEL: unchanged
    assert rec[1][3:5] == ["N", "NACGTNA"] and rec[1][7] == old[1][7] + ";CONSLEN=6;CONSREADS=3"
    assert rec[2][3:5] == ["N", "<INS>"] and rec[2][7] == old[2][7] + ";CONSLEN=9;CONSREADS=2"
    assert rec[3][3:5] == ["N", "<INS>"] and rec[3][7] == old[3][7] + ";CONSLEN=0;CONSREADS=0"
    for r, o in zip(rec, old):
        assert r[:3] == o[:3] and r[5:7] == o[5:7] and r[7].startswith("SVTYPE=") and r[7].split(";")[1].startswith("END=")
        # the text parses back to the locus of the <INS> form
        assert host.parse_line("\t".join(r)) == host.parse_line("\t".join(o))
        assert host.parse_line("\t".join(r))[0] == 1


def test_format_with_genotypes_and_without_consensus():
    from svtrek_amd._lib import GT_DTYPE
    calls, res, bases = fmt_calls()
    gts = np.zeros(4, dtype=GT_DTYPE)
    gts["gt"] = [1, 2, -1, 0]
    a = host.format_calls(calls, ["chrA", "chrB"], genotypes=gts, consensus=(res, bases)).splitlines()
    b = host.format_calls(calls, ["chrA", "chrB"], genotypes=gts).splitlines()
    ra, rb = [ln.split("\t") for ln in a if ln[0] != "#"], [ln.split("\t") for ln in b if ln[0] != "#"]
    assert [r[8:] for r in ra] == [r[8:] for r in rb] and ra[1][4] == "NACGTNA"
    # without consensus arguments: svth_format_calls / svth_format_calls_gt byte for byte
    import ctypes as C
    L = host.load_host()
    names = (C.c_char_p * 2)(b"chrA", b"chrB")
    n1, n2 = C.c_size_t(0), C.c_size_t(0)
    p1 = L.svth_format_calls(calls.ctypes.data, 4, names, 2, 1, 2, C.byref(n1))
    p2 = L.svth_format_calls_seq(calls.ctypes.data, None, None, None, 0, 4, names, 2, None, 1, 2, C.byref(n2))
    try:
        assert C.string_at(p1, n1.value) == C.string_at(p2, n2.value)
        assert C.string_at(p1, n1.value).decode() == host.format_calls(calls, ["chrA", "chrB"])
    finally:
        L.svth_free(p1)
        L.svth_free(p2)
    # no calls: the header still names the two keys
    empty = host.format_calls(calls[:0], ["chrA"], consensus=(res[:0], bases[:0]))
    assert "ID=CONSLEN" in empty and empty.endswith("INFO\n")


def test_cpu_backend_cli_has_no_ins_seq(tmp_path):
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_cpu", "svtrek_cpu")
    bam = tmp_path / "x.bam"
    bam.write_bytes(b"")
    p = subprocess.run([cli, "call", "-b", str(bam), "--ins-seq"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode != 0 and p.stderr.decode() == "[ERROR] ins-seq: not supported by this backend\n"
    h = subprocess.run([cli, "call", "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert all(f in h.stdout.decode() for f in ("--ins-seq", "--ins-seq-cap"))
