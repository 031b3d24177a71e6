"""include/svtrek_genotype.h on the CPU: the numpy model (tests/genotype_ref.py) on a hand-built pileup
with every count written out, the PL arithmetic's worked values, the model on the calls of a
simulated pileup, and the VCF text of svth_format_calls_gt through svth_parse_line."""
import functools
import os
import subprocess
from dataclasses import replace

import numpy as np

from svtrek_amd import calls_to_sites, from_reads, gt_costs, host, sim, sites_from_loci
from svtrek_amd._lib import CALL_DTYPE, GT_DTYPE, GT_SITE_DTYPE, LOCUS_DTYPE, RESULT_DTYPE, SVT_DEL, SVT_INS, SVT_NA

import call_ref
import genotype_ref

M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
ANY = 0xFFFFFFFF


def hand_reads():
    """A DEL of 200 at x = 10 000 (site [10 000, 10 201], flank 50: a = 9 950, b = 10 251) and an INS of
    80 at the same x (site [10 000, 10 001]: a = 9 950, b = 10 051)."""
    return [
        (0, 9000, [(M, 1000), (D, 200), (M, 1000)]),   # 3 carriers, [9000, 11200): they span
        (0, 9000, [(M, 1000), (D, 200), (M, 1000)]),
        (0, 9000, [(M, 1000), (D, 200), (M, 1000)]),
        (0, 9951, [(M, 49), (D, 200), (M, 1000)]),     # a carrier starting at a + 1: alt_all only
        (0, 9000, [(M, 1000), (D, 200), (M, 51)]),     # a carrier ending at b = 10 251: alt_all only
        (0, 9000, [(M, 1251)]),                        # a reference read ending at b: does not span
        (0, 9000, [(M, 1252)]),                        # two ending at b + 1: they span
        (0, 9000, [(M, 1252)]),
        (0, 9950, [(M, 2000)]),                        # starting at a: spans
        (0, 9951, [(M, 2000)]),                        # starting at a + 1: does not
        (0, 9000, [(M, 1000), (D, 60), (M, 1500)]),    # spans with a D of another length: ref
        (0, 9000, [(M, 1006), (D, 200), (M, 1000)]),   # spans with the D at x = 10 006, outside [9995, 10005]: ref
        (0, 9000, [(M, 1000), (I, 80), (M, 1500)]),    # spans with an I at 10 000: ref for the DEL, alt for the INS
        (1, 100, [(M, 50)]),                           # contig 2 has a read, contig 3 none
    ]


HAND_SITES = genotype_ref.sites([
    (SVT_DEL, 1, 10000, 10201, 9995, 10005, 150, 250),
    (SVT_INS, 1, 10000, 10001, 9990, 10010, 50, ANY),
    (SVT_DEL, 1, 10000, 10201, 9995, 10006, 51, ANY),    # every D > 50 near the start
])
# DEL: span = 3 carriers + 2 + 1 + the three reads with other ops = 9; alt_all = 3 + 1 + 1; alt = 3; ref = 6
#      L = {6 * 223 + 3 * 13010, 9 * 3010, 6 * 13010 + 3 * 223} = {40368, 27090, 78729}: 0/1, PL 13,0,52
# INS: b = 10 051, so the reads ending at 10 251 span too: 13 reads - the two starting at 9951 = 11;
#      alt_all = alt = 1, ref = 10; L = {15240, 33110, 130323}: 0/0, PL 0,18,115
# the wide DEL: alt_all = 7 (all D ops), alt = 5 (without the two that do not span), ref = 4;
#      L = {65942, 27090, 53155}: 0/1, PL 39,0,26
HAND_WANT = [(3, 6, 9, 5, 1, 13, (13, 0, 52)), (1, 10, 11, 1, 0, 18, (0, 18, 115)), (5, 4, 9, 7, 1, 26, (39, 0, 26))]


def rec(g):
    return (int(g["alt"]), int(g["ref"]), int(g["span"]), int(g["alt_all"]), int(g["gt"]), int(g["gq"]),
            tuple(int(v) for v in g["pl"]))


def test_model_on_a_hand_built_pileup():
    pl = from_reads(3, hand_reads(), clip={})
    got = genotype_ref.genotype(pl, HAND_SITES)
    assert [rec(g) for g in got] == HAND_WANT
    # flank 0: a = 10 000, b = 10 201 -- the reads starting at 9951 and those ending at 10 251 span too
    g0 = genotype_ref.genotype(pl, HAND_SITES[:1], flank=0)[0]
    assert rec(g0)[:4] == (5, 8, 13, 5)
    # invalid sites: type, chrom 0 / past the last, x_lo > x_hi, len_lo > len_hi, a contig without reads
    bad = genotype_ref.sites([(3, 1, 10000, 10201, 9995, 10005, 150, 250), (SVT_DEL, 0, 10000, 10201, 9995, 10005, 150, 250),
                              (SVT_DEL, 4, 10000, 10201, 9995, 10005, 150, 250), (SVT_DEL, 1, 10000, 10201, 10005, 9995, 150, 250),
                              (SVT_DEL, 1, 10000, 10201, 9995, 10005, 250, 150), (SVT_DEL, 3, 10000, 10201, 9995, 10005, 150, 250)])
    for g in genotype_ref.genotype(pl, bad):
        assert rec(g) == (0, 0, 0, 0, -1, 0, (0, 0, 0))
    # a valid site nobody spans: counts 0, no call
    assert rec(genotype_ref.genotype(pl, genotype_ref.sites([(SVT_DEL, 2, 120, 200, 0, 10, 0, ANY)]))[0]) == \
        (0, 0, 0, 0, -1, 0, (0, 0, 0))


def test_likelihood_worked_values():
    assert genotype_ref.likelihood(20, 0) == (2, 56, [256, 56, 0])
    assert genotype_ref.likelihood(10, 10) == (1, 72, [72, 0, 72])
    assert genotype_ref.likelihood(1, 19) == (0, 43, [0, 43, 230])
    assert genotype_ref.likelihood(0, 0) == (-1, 0, [0, 0, 0])
    # equal costs: every L ties, the lowest g wins
    assert genotype_ref.likelihood(7, 9, (1000, 1000, 1000), (1000, 1000, 1000)) == (0, 0, [0, 0, 0])
    # the caps: PL at 65535, GQ at 99
    assert genotype_ref.likelihood(100000, 0) == (2, 99, [65535, 65535, 0])
    assert genotype_ref.likelihood(0, 40) == (0, 99, [0, 111, 511])
    assert gt_costs(0.05) == (genotype_ref.REF_COST, genotype_ref.ALT_COST)
    assert gt_costs(0.01) == ((44, 3010, 20000), (20000, 3010, 44))


@functools.lru_cache(maxsize=None)
def sim_case():
    r = sim.generate(replace(sim.WORKLOADS["cfg4_1m_delins_30x_hifi"], n_loci=2000, n_targets=2))
    calls = call_ref.call(r.pileup)[0]
    return r, calls, genotype_ref.genotype(r.pileup, calls)


def test_model_on_the_calls_of_a_simulated_pileup():
    _, calls, gts = sim_case()
    assert len(calls) >= 2000
    assert np.array_equal(gts["alt_all"], calls["support"])
    assert (gts["alt"] <= gts["span"]).all()
    assert np.array_equal(gts["ref"], gts["span"] - gts["alt"])
    # (the simulator has no zygosity truth: the split is printed, not asserted)
    print("0/0, 0/1, 1/1, no call:", [int((gts["gt"] == g).sum()) for g in (0, 1, 2, -1)])


def test_sites_of_calls_and_loci():
    _, calls, _ = sim_case()
    s = calls_to_sites(calls[:50])
    assert s.dtype == GT_SITE_DTYPE and GT_SITE_DTYPE.itemsize == 32 and GT_DTYPE.itemsize == 32
    for f in GT_SITE_DTYPE.names:
        assert np.array_equal(s[f], calls[f][:50])
    loci = np.array([(SVT_DEL, 1, 990, 1310), (SVT_INS, 2, 5, 6), (SVT_DEL, 1, 990, 1310), (SVT_INS, 1, 70, 71),
                     (SVT_DEL, 1, 990, 1310)], dtype=LOCUS_DTYPE)
    refined = np.array([(1000, 1301), (4, SVT_NA), (SVT_NA, 1301), (SVT_NA, SVT_NA), (1000, SVT_NA)], dtype=RESULT_DTYPE)
    s = sites_from_loci(loci, refined, radius=10, len_tol=20)
    assert tuple(s[0]) == (SVT_DEL, 1, 1000, 1301, 990, 1010, 280, 320)
    assert tuple(s[1]) == (SVT_INS, 2, 4, 5, 0, 14, 0, ANY)
    assert tuple(sites_from_loci(loci, refined)[0])[6:] == (0, ANY)
    for k in (2, 3, 4):   # a refined NA: an invalid site
        assert int(s[k]["type"]) == 0 and int(s[k]["x_lo"]) > int(s[k]["x_hi"])


def test_format_calls_with_genotypes():
    pl = from_reads(3, hand_reads(), clip={})
    hand_calls = call_ref.call(pl, min_support=1)[0]
    _, sim_calls, sim_gts = sim_case()
    calls = np.concatenate([hand_calls, sim_calls[:200]])
    gts = np.concatenate([genotype_ref.genotype(pl, hand_calls), sim_gts[:200]])
    gts[-1]["gt"] = -1   # a no call prints ./. and zeros whatever the record holds
    text = host.format_calls(calls, ["1", "2", "3"], genotypes=gts, sample="HG002")
    lines = text.splitlines()
    head = [ln for ln in lines if ln.startswith("#")]
    body = [ln for ln in lines if not ln.startswith("#")]
    assert head[0] == "##fileformat=VCFv4.2" and head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tHG002"
    assert [h.split(",")[0] for h in head if h.startswith("##FORMAT")] == \
        [f"##FORMAT=<ID={k}" for k in ("GT", "GQ", "DR", "DV", "PL")]
    assert all(h.startswith("##") for h in head[:-1]) and len(body) == len(calls)
    # the INS at 10 000 comes first: the INS site of HAND_SITES (1 alt, 10 ref of 11 spanning reads)
    assert body[0] == ("1\t10000\tsvtrek.INS.1\tN\t<INS>\t.\tPASS\tSVTYPE=INS;END=10001;SVLEN=80;SUPPORT=1;DEPTH=13;"
                       "XRANGE=10000,10000;LENRANGE=80,80\tGT:GQ:DR:DV:PL\t0/0:18:10:1:0,18,115")
    # the seven D ops at 10 000 .. 10 006 are one call: pos 10 001, len (6 * 200 + 60 + 3) // 7 = 180, end
    # (5 * 10201 + 10061 + 10207 + 3) // 7 = 10 182; a = 9951, b = 10 232: all 13 reads span, 7 alt, 6 ref;
    # L = {92408, 39130, 79621}
    assert body[1] == ("1\t10001\tsvtrek.DEL.1\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=10182;SVLEN=-180;SUPPORT=7;DEPTH=13;"
                       "XRANGE=10000,10006;LENRANGE=60,200\tGT:GQ:DR:DV:PL\t0/1:40:6:7:53,0,40")
    assert body[-1].endswith("\tGT:GQ:DR:DV:PL\t./.:0:0:0:0,0,0")
    for ln, c in zip(body, calls):
        assert len(ln.split("\t")) == 10
        act, got, err = host.parse_line(ln)
        assert act == 1 and err == "" and got == tuple(int(c[f]) for f in ("type", "chrom", "pos", "end")), ln
    # without genotypes: the sites-only text, byte for byte svth_format_calls'
    L = host.load_host()
    import ctypes as C
    arr = (C.c_char_p * 3)(b"1", b"2", b"3")
    n = C.c_size_t(0)
    cc = np.ascontiguousarray(calls, dtype=CALL_DTYPE)
    p = L.svth_format_calls(cc.ctypes.data, len(cc), arr, 3, 1, 4, C.byref(n))
    old = C.string_at(p, n.value).decode("latin-1")
    L.svth_free(p)
    assert host.format_calls(calls, ["1", "2", "3"], genotypes=None) == old == host.format_calls(calls, ["1", "2", "3"])
    assert [ln + "\t" + b.split("\t", 8)[8] for ln, b in zip(old.splitlines()[-len(calls):], body)] == body
    assert "FORMAT" not in old
    # no calls: the header alone still names the sample
    assert host.format_calls(calls[:0], ["1"], genotypes=gts[:0]).splitlines()[-1].endswith("\tFORMAT\tSAMPLE")
    assert host.format_calls(calls[:0], ["1"], genotypes=gts[:0], header=False) == ""


def test_cpu_backend_cli_has_no_genotype(tmp_path):
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_cpu", "svtrek_cpu")
    bam = tmp_path / "x.bam"
    bam.write_bytes(b"")
    p = subprocess.run([cli, "call", "-b", str(bam), "--genotype"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode != 0 and p.stderr.decode() == "[ERROR] genotype: not supported by this backend\n"
    p = subprocess.run([cli, "call", "-b", str(bam)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode != 0 and p.stderr.decode() == "[ERROR] call: not supported by this backend\n"
    h = subprocess.run([cli, "call", "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert all(f in h.stdout.decode() for f in ("--genotype", "--flank", "--sample"))
