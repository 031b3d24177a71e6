"""include/svtrek_genotype.h on the HIP engine: Engine.genotype / genotype_calls against the numpy
model (tests/genotype_ref.py, pinned by tests/test_genotype_model.py), record for record, on pileups
built to reach every path of svt_genotype.inc (bucket edges, a contig's last bucket, several trips of
both loops, every kind of invalid site), the API's status codes, and `svtrek call --genotype`."""
import functools
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

from svtrek_amd import Engine, Params, SvtError, calls_to_sites, from_reads, gt_costs, host, sim
from svtrek_amd._lib import GT_DTYPE, SVT_DEL, SVT_EINVAL, SVT_ESTATE, SVT_INS

import call_ref
import fuzz
import genotype_ref
from test_genotype_model import HAND_SITES, HAND_WANT, hand_reads, rec
from test_gpu_call import exact_reads, write_bam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "svtrek_amd", "svtrek")
M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
ANY = 0xFFFFFFFF
NO_CALL = (0, 0, 0, 0, -1, 0, (0, 0, 0))


def same(got, want):
    assert got.dtype == GT_DTYPE and want.dtype == GT_DTYPE
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(want)} records differ; first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


def check(eng, pl, sites, flank=None, costs=None):
    """Engine.genotype == the model; returns the records."""
    want = genotype_ref.genotype(pl, sites, 50 if flank is None else flank,
                                 (genotype_ref.REF_COST, genotype_ref.ALT_COST) if costs is None else costs)
    got = eng.genotype(sites, flank=flank, costs=costs)
    same(got, want)
    return got


def carrier(x, ln=100, tid=0, lead=2000, op=D, tail=3000):
    return (tid, x - lead, [(M, lead), (op, ln), (M, tail)])


def counts(g):
    return rec(g)[:4]   # alt, ref, span, alt_all


@pytest.fixture(scope="module")
def eng():
    with Engine(Params(), device=0) as e:
        yield e


def test_hand_built_pileup(eng):
    import torch
    pl = from_reads(3, hand_reads(), clip={})
    eng.load_pileup(pl)
    got = check(eng, pl, HAND_SITES)
    assert [rec(g) for g in got] == HAND_WANT
    assert counts(check(eng, pl, HAND_SITES, flank=0)[0]) == (5, 8, 13, 5)
    assert len(eng.genotype(HAND_SITES[:0])) == 0                                  # n = 0
    # device buffers on a non-default stream
    d_sites = torch.from_numpy(HAND_SITES.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(len(HAND_SITES) * GT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.genotype_device(d_sites.data_ptr(), len(HAND_SITES), d_out.data_ptr(), stream=s.cuda_stream)
    eng.sync(s.cuda_stream)
    same(d_out.cpu().numpy().view(GT_DTYPE), got)


def test_pos_below_flank_clamps_to_zero(eng):
    reads = [(0, 0, [(M, 30), (D, 100), (M, 500)])] * 3 + [(0, 1, [(M, 1000)]), (0, 0, [(M, 182)]), (0, 0, [(M, 181)])]
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got = check(eng, pl, genotype_ref.sites([(SVT_DEL, 1, 30, 131, 20, 40, 51, ANY)]))
    assert counts(got[0]) == (3, 1, 4, 3)   # a = 0, b = 181: the reads at pos 0 ending past 181


def test_x_range_across_a_bucket_edge(eng):
    xs = (1019, 1020, 1022, 1024, 1027, 1030, 1031)   # buckets 0 and 1; the first and last lie outside
    pl = from_reads(1, [carrier(x, lead=900) for x in xs], clip={})
    eng.load_pileup(pl)
    got = check(eng, pl, genotype_ref.sites([(SVT_DEL, 1, 1025, 1126, 1020, 1030, 51, ANY), (SVT_DEL, 1, 1025, 1126, 1024, 1024, 51, ANY)]))
    assert counts(got[0]) == (5, 2, 7, 5) and counts(got[1]) == (1, 6, 7, 1)


def test_x_range_over_four_buckets(eng):
    xs = (1100, 1500, 2500, 3600, 3900)   # 1100 and 3900 share the end buckets with 1500 and 3600
    pl = from_reads(1, [carrier(x, lead=1000, tail=4000) for x in xs] + [carrier(2500, op=I, lead=1000, tail=4000)], clip={})
    eng.load_pileup(pl)
    got = check(eng, pl, genotype_ref.sites([(SVT_DEL, 1, 2500, 2601, 1500, 3600, 51, ANY)]), flank=0)
    assert counts(got[0]) == (2, 2, 4, 3)   # 1500, 2500, 3600; the reads at 100, 500 and 1500 (the D and the I) span


def test_site_in_the_contigs_last_bucket(eng):
    """H ops lengthen the walk but not endpos (185 here): every x = 300 100 + 97 k lies in the contig's
    last bucket, far past its nominal 1 kb."""
    reads = [(0, 100, [(H, 300000 + 97 * k), (D, 80), (M, 5)]) for k in range(60)]
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    x0 = 300100
    sites = genotype_ref.sites([(SVT_DEL, 1, 150, 151, x0 + 97 * 10, x0 + 97 * 20, 51, ANY),
                                (SVT_DEL, 1, 150, 151, x0 + 97 * 59, ANY, 51, ANY),        # x_hi is clamped
                                (SVT_DEL, 1, 150, 151, 1 << 30, ANY, 51, ANY)])            # no items past the clamp
    got = check(eng, pl, sites, flank=10)
    assert [counts(g) for g in got] == [(11, 49, 60, 11), (1, 59, 60, 1), (0, 60, 60, 0)]


def test_two_lengths_at_one_start(eng):
    reads = [carrier(7000, 300)] * 4 + [carrier(7000, 500)] * 3 + [(0, 5000, [(M, 5000)])] * 2
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    sites = genotype_ref.sites([(SVT_DEL, 1, 7000, 7301, 7000, 7000, 300, 300), (SVT_DEL, 1, 7000, 7501, 7000, 7000, 500, 500),
                                (SVT_DEL, 1, 7000, 7501, 7000, 7000, 300, 500)])
    got = check(eng, pl, sites)
    assert [counts(g) for g in got] == [(4, 5, 9, 4), (3, 6, 9, 3), (7, 2, 9, 7)]
    assert [int(g["gt"]) for g in got] == [1, 1, 1]       # 7 of 9: L = {91516, 27090, 27581}


def test_trailing_soft_clips_are_not_items(eng):
    reads = [carrier(8000), carrier(8001)] + [(0, 7000 + k, [(M, 1000 - k), (S, 30)]) for k in range(5)]
    reads += [(0, 6000, [(M, 5000)])]
    pl = from_reads(1, reads, clip=None)
    eng.load_pileup(pl)
    got = check(eng, pl, genotype_ref.sites([(SVT_DEL, 1, 8000, 8101, 7990, 8010, 0, ANY)]))
    assert counts(got[0]) == (2, 1, 3, 2)


def test_del_and_ins_at_one_x(eng):
    reads = [(0, 400, [(M, 1000), (I, 80), (D, 80), (M, 1000)])] * 3 + [carrier(1400, 80, op=I, lead=1000, tail=1000)] * 2
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    sites = genotype_ref.sites([(SVT_DEL, 1, 1400, 1481, 1400, 1400, 80, 80), (SVT_INS, 1, 1400, 1401, 1400, 1400, 80, 80)])
    got = check(eng, pl, sites)
    assert [counts(g) for g in got] == [(3, 2, 5, 3), (5, 0, 5, 5)]


def test_more_than_one_trip_of_both_loops(eng):
    reads = [carrier(20000 + k % 5, 120 + k % 3, lead=1500 + k) for k in range(200)]
    reads += [(0, 17000 + 7 * k, [(M, 6000)]) for k in range(150)]
    reads += [carrier(20000, 120, lead=20, tail=4000)] * 7      # carriers that start inside the flank
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got = check(eng, pl, genotype_ref.sites([(SVT_DEL, 1, 20002, 20123, 20000, 20004, 120, 122)]))
    assert counts(got[0]) == (200, 150, 350, 207) and int(got[0]["gt"]) == 1


def test_a_read_with_two_matching_items(eng):
    pl = from_reads(1, [(0, 0, [(M, 100), (D, 60), (M, 10), (D, 60), (M, 500)])], clip={})
    eng.load_pileup(pl)
    got = check(eng, pl, genotype_ref.sites([(SVT_DEL, 1, 100, 231, 90, 180, 51, ANY)]))
    assert rec(got[0]) == (2, 0, 1, 2, 2, 6, (26, 6, 0))   # ref saturates at 0; L = {26020, 6020, 446}


def test_invalid_sites_and_contigs_without_reads(eng):
    pl = from_reads(3, hand_reads(), clip={})   # contig 3 has no reads
    eng.load_pileup(pl)
    ok = (SVT_DEL, 1, 10000, 10201, 9995, 10005, 150, 250)
    rows = [ok, (3, *ok[1:]), (0, *ok[1:]), (-1, *ok[1:]), (SVT_DEL, 0, *ok[2:]), (SVT_DEL, -1, *ok[2:]), (SVT_DEL, 4, *ok[2:]),
            (SVT_DEL, 1, 10000, 10201, 10005, 9995, 150, 250), (SVT_DEL, 1, 10000, 10201, 9995, 10005, 250, 150),
            (SVT_DEL, 3, *ok[2:]), (SVT_INS, 3, *ok[2:]), ok]
    got = check(eng, pl, genotype_ref.sites(rows))
    assert rec(got[0]) == HAND_WANT[0] == rec(got[-1])
    assert all(rec(g) == NO_CALL for g in got[1:-1])


def test_empty_pileup(eng):
    pl = from_reads(2, [], clip={})
    eng.load_pileup(pl)
    got = check(eng, pl, HAND_SITES)
    assert all(rec(g) == NO_CALL for g in got)
    assert len(eng.call()) == 0 and len(eng.genotype_calls()) == 0
    pl = from_reads(1, [(0, 5, [(M, 500)])], clip={})    # reads, no items
    eng.load_pileup(pl)
    got = check(eng, pl, genotype_ref.sites([(SVT_DEL, 1, 100, 200, 90, 110, 0, ANY)]))
    assert rec(got[0]) == (0, 1, 1, 0, 0, 3, (0, 3, 13))


def test_custom_costs(eng):
    pl = from_reads(3, hand_reads(), clip={})
    eng.load_pileup(pl)
    check(eng, pl, HAND_SITES, costs=gt_costs(0.01))
    got = check(eng, pl, HAND_SITES, costs=((1000, 1000, 1000), (1000, 1000, 1000)))
    assert [(int(g["gt"]), int(g["gq"])) for g in got] == [(0, 0)] * 3                  # all tied: the lowest g
    got = check(eng, pl, HAND_SITES, costs=((0, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF, 0)))
    assert [tuple(int(v) for v in g["pl"]) for g in got][0] == (0, 65535, 65535)        # the caps


@functools.lru_cache(maxsize=None)
def fuzz_pileup(seed, n_reads, max_ops):
    rng = np.random.default_rng(seed)
    hot = [int(x) for x in rng.integers(5000, 55000, size=5)]
    return fuzz.random_pileup(rng, n_targets=2, contig_len=60000, n_reads=n_reads, max_ops=max_ops, hot=hot), hot


def random_sites(rng, n, hot):
    rows = []
    for _ in range(n):
        ty = int(rng.choice([SVT_DEL, SVT_DEL, SVT_INS, SVT_INS, 3, 0]))
        chrom = int(rng.choice([1, 1, 1, 2, 2, 2, 0, 3]))
        pos = int(rng.choice(hot)) + int(rng.integers(-60, 61)) if rng.random() < 0.8 else int(rng.integers(0, 60000))
        pos = max(pos, 0)
        end = pos + int(rng.choice([0, 1, 51, 300, 1500, 20000]))
        if rng.random() < 0.05:
            end = max(pos - 40, 0)
        r = int(rng.choice([0, 3, 10, 600, 3000]))
        x_lo, x_hi = max(pos - r, 0), pos + r
        ln = int(rng.choice([49, 50, 51, 80, 500, 1500]))
        len_lo, len_hi = [(0, ANY), (ln, ln), (50, 80), (ln, ANY), (0, ln)][int(rng.integers(0, 5))]
        if rng.random() < 0.04:
            x_lo, x_hi = x_hi + 1, x_lo
        if rng.random() < 0.04:
            len_lo, len_hi = 81, 80
        rows.append((ty, chrom, pos, end, x_lo, x_hi, len_lo, len_hi))
    return genotype_ref.sites(rows)


@pytest.mark.parametrize("seed, n_reads, max_ops", [(901, 400, 60), (905, 120, 600)], ids=["short901", "long905"])
def test_fuzz_pileups(eng, seed, n_reads, max_ops):
    pl, hot = fuzz_pileup(seed, n_reads, max_ops)
    eng.load_pileup(pl)
    calls = call_ref.call(pl, min_support=1)[0]
    sites = np.concatenate([calls_to_sites(calls), random_sites(np.random.default_rng(seed + 1), 200, hot)])
    assert len(calls) > 50
    got = check(eng, pl, sites)
    assert np.array_equal(got["alt_all"][:len(calls)], calls["support"])
    assert (got["gt"] >= 0).sum() > 50
    check(eng, pl, sites, flank=0)
    check(eng, pl, sites, flank=700, costs=gt_costs(0.2))
    # genotype_calls: the same calls where the scan left them
    assert np.array_equal(eng.call(min_support=1), calls)
    same(eng.genotype_calls(), got[:len(calls)])


def test_genotype_calls_on_the_exact_and_the_sim_pileup(eng):
    pl = from_reads(1, exact_reads(), clip={})
    eng.load_pileup(pl)
    calls = eng.call()
    want = genotype_ref.genotype(pl, call_ref.call(pl)[0])
    got = eng.genotype_calls()
    same(got, want)
    assert [rec(g) for g in got] == [(6, 0, 6, 6, 2, 17, (77, 17, 0))] * 5   # L = {78060, 18060, 1338}
    same(eng.genotype(calls_to_sites(calls)), want)
    r = sim.generate(replace(sim.WORKLOADS["cfg4_1m_delins_30x_hifi"], n_loci=2000, n_targets=2))
    eng.load_pileup(r.pileup)
    calls = eng.call()
    want = genotype_ref.genotype(r.pileup, calls)
    got = eng.genotype_calls()
    same(got, want)
    assert len(got) >= 2000 and np.array_equal(got["alt_all"], calls["support"]) and (got["alt"] <= got["span"]).all()
    eng.reindex()
    same(eng.genotype_calls(), want)
    same(eng.genotype_calls(flank=0), genotype_ref.genotype(r.pileup, calls, flank=0))


def test_status_codes(eng, monkeypatch):
    with Engine(Params(), device=0) as e0:
        for f in (lambda: e0.genotype(HAND_SITES), lambda: e0.genotype(HAND_SITES[:0]), e0.genotype_calls):
            with pytest.raises(SvtError) as ei:
                f()
            assert ei.value.code == SVT_ESTATE
    pl, _ = fuzz_pileup(901, 400, 60)
    eng.load_pileup(pl)
    with pytest.raises(SvtError) as ei:   # loaded, not scanned
        eng.genotype_calls()
    assert ei.value.code == SVT_ESTATE and "svt_call_scan" in str(ei.value)
    for flank in (-1, (1 << 20) + 1):
        with pytest.raises(SvtError) as ei:
            eng.genotype(HAND_SITES, flank=flank)
        assert ei.value.code == SVT_EINVAL
    check(eng, pl, HAND_SITES, flank=1 << 20)
    n = len(eng.call())
    out = np.empty(n + 1, dtype=GT_DTYPE)
    p = eng.gt_params()
    assert eng.lib.svt_genotype_calls(eng._h, p, out.ctypes.data, n + 1) == SVT_EINVAL
    assert eng.lib.svt_genotype_calls(eng._h, None, out.ctypes.data, n) == SVT_EINVAL
    assert eng.lib.svt_genotype_batch(eng._h, p, None, 3, out.ctypes.data) == SVT_EINVAL
    assert eng.lib.svt_genotype_batch(eng._h, p, HAND_SITES.ctypes.data, 3, None) == SVT_EINVAL
    monkeypatch.setenv("SVTREK_INDEX", "lists")
    with Engine(Params(), device=0) as e1:
        e1.load_pileup(pl)
        with pytest.raises(SvtError) as ei:
            e1.genotype(HAND_SITES)
        assert ei.value.code == SVT_ESTATE and "SVTREK_INDEX=lists" in str(ei.value)


@pytest.mark.parametrize("inflate", ["cpu", "gpu"])
def test_cli_call_genotype_then_audt(tmp_path, inflate):
    reads = exact_reads()
    bam, vcf, vcf8 = str(tmp_path / "x.bam"), str(tmp_path / "g.vcf"), str(tmp_path / "c.vcf")
    write_bam(bam, reads)
    pl = from_reads(1, reads, clip={})
    calls = call_ref.call(pl)[0]

    def run(*args):
        return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    p = run("call", "-b", bam, "-o", vcf, "--inflate", inflate, "--genotype", "--verbose")
    assert p.returncode == 0 and p.stdout == "" and "calls 5" in p.stderr and "genotype " in p.stderr, p.stderr
    with open(vcf) as f:
        assert f.read() == host.format_calls(calls, ["1"], genotypes=genotype_ref.genotype(pl, calls))
    p = run("call", "-b", bam, "--inflate", inflate, "--genotype", "--flank", "900", "--sample", "NA12878")
    assert p.returncode == 0 and p.stdout == host.format_calls(calls, ["1"], genotypes=genotype_ref.genotype(pl, calls, flank=900),
                                                               sample="NA12878")
    assert p.stdout.count("\t1/1:11:0:4:51,11,0\n") == 5     # the four reads of a site that start 900 before it span
    p = run("call", "-b", bam, "-o", vcf8, "--inflate", inflate)
    with open(vcf8) as f:
        assert p.returncode == 0 and f.read() == host.format_calls(calls, ["1"])
    a10, a8 = (run("audt", "-b", bam, "-v", v, "--inflate", inflate) for v in (vcf, vcf8))
    assert a10.returncode == 0 and a8.returncode == 0, a10.stderr
    lines = [ln for ln in a10.stdout.splitlines() if ln.startswith("(")]
    assert len(lines) == 5 and lines == [ln for ln in a8.stdout.splitlines() if ln.startswith("(")]
    bad = run("call", "-b", bam, "--genotype", "--flank", "-3")
    assert bad.returncode == 1 and "--flank" in bad.stderr
