"""include/svtrek_call.h on the HIP engine: Engine.call against the numpy model (tests/call_ref.py,
pinned by tests/test_call_model.py), record for record, on pileups built to reach every path of
svt_call.inc (segments of several buckets, big buckets, chains over many segments, contig and type
boundaries, the 2^30 cut), the API's status codes, and `svtrek call` into `svtrek audt`."""
import functools
import os
import random
import struct
import subprocess
from dataclasses import replace

import numpy as np
import pytest

from svtrek_amd import Engine, Params, SvtError, calls_to_loci, from_reads, host, sim
from svtrek_amd._lib import CALL_DTYPE, SVT_DEL, SVT_EINVAL, SVT_ESTATE, SVT_INS, SVT_NA

import bamfix
import call_ref
import fuzz

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "svtrek_amd", "svtrek")
M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
NAMES = {"DEL": SVT_DEL, "INS": SVT_INS}


def same(got, want):
    assert got.dtype == CALL_DTYPE and want.dtype == CALL_DTYPE
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(want)} records differ; first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


def check(eng, pl, link=None, min_support=None, types=("DEL", "INS")):
    """Engine.call == the model, the stats too; returns (calls, engine stats)."""
    want, wst = call_ref.call(pl, 10 if link is None else link, 3 if min_support is None else min_support,
                              tuple(NAMES[t] for t in types))
    got = eng.call(link=link, min_support=min_support, types=types)
    same(got, want)
    st = eng.call_stats()
    assert {k: st[k] for k in wst} == wst
    assert st["scan_ms"] >= 0.0
    return got, st


def d_at(x, ln=100, tid=0, lead=200, op=D, tail=60):
    return (tid, x - lead, [(M, lead), (op, ln), (M, tail)])


def rec(c):
    return tuple(int(v) for v in c)[:5]   # type, chrom, pos, end, support


@pytest.fixture(scope="module")
def eng():
    with Engine(Params(), device=0) as e:
        yield e


def test_cluster_across_a_bucket_edge(eng):
    pl = from_reads(1, [d_at(x) for x in (1020, 1022, 1024, 1027)], clip={})   # buckets 0 and 1
    eng.load_pileup(pl)
    got, _ = check(eng, pl)
    assert [rec(c) for c in got] == [(SVT_DEL, 1, 1023, 1124, 4)]


def test_gap_equal_to_link_and_one_more(eng):
    xs = [5000, 5010, 5020, 5031, 5041, 5051]   # 5020 -> 5031 is link + 1
    pl = from_reads(1, [d_at(x, op=I) for x in xs] + [d_at(x) for x in xs], clip={})
    eng.load_pileup(pl)
    got, _ = check(eng, pl)
    assert [rec(c) for c in got] == [(SVT_INS, 1, 5010, 5011, 3), (SVT_DEL, 1, 5010, 5111, 3),
                                     (SVT_INS, 1, 5041, 5042, 3), (SVT_DEL, 1, 5041, 5142, 3)]
    assert len(check(eng, pl, link=11)[0]) == 2
    assert len(check(eng, pl, link=9, min_support=1)[0]) == 12
    got, _ = check(eng, pl, link=0, min_support=1, types=("DEL",))
    assert len(got) == 6 and (got["type"] == SVT_DEL).all()
    check(eng, pl, types=("INS",))


def test_support_at_and_below_min_support(eng):
    pl = from_reads(1, [d_at(2000), d_at(2001)] + [d_at(9000), d_at(9001), d_at(9002)], clip={})
    eng.load_pileup(pl)
    got, st = check(eng, pl)
    assert [rec(c) for c in got] == [(SVT_DEL, 1, 9001, 9102, 3)] and st["clusters"] == 2
    assert len(check(eng, pl, min_support=2)[0]) == 2
    assert len(check(eng, pl, min_support=4)[0]) == 0


def test_link_zero_and_equal_starts(eng):
    pl = from_reads(1, [d_at(700, ln) for ln in (60, 70, 80)] + [d_at(701, 90)] * 3, clip={})
    eng.load_pileup(pl)
    got, _ = check(eng, pl, link=0)
    assert [rec(c) for c in got] == [(SVT_DEL, 1, 700, 771, 3), (SVT_DEL, 1, 701, 792, 3)]
    assert (int(got[0]["len_lo"]), int(got[0]["len_hi"]), int(got[0]["len"])) == (60, 80, 70)


def test_length_thresholds(eng):
    reads = [d_at(3000, 50)] * 3 + [d_at(4000, 51)] * 3 + [d_at(5000, 49, op=I)] * 3 + [d_at(6000, 50, op=I)] * 3
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, st = check(eng, pl)
    assert [rec(c) for c in got] == [(SVT_DEL, 1, 4000, 4052, 3), (SVT_INS, 1, 6000, 6001, 3)] and st["events"] == 6


def test_trailing_soft_clips_are_not_items(eng):
    # reads whose walk ends at 8000 with a trailing S: markers of array S at the cluster's x
    reads = [d_at(8000), d_at(8001)] + [(0, 7000 + k, [(M, 1000 - k), (S, 30)]) for k in range(5)]
    pl = from_reads(1, reads, clip=None)
    eng.load_pileup(pl)
    got, st = check(eng, pl, min_support=2)
    assert [rec(c) for c in got] == [(SVT_DEL, 1, 8001, 8102, 2)] and st["events"] == 2


def test_del_and_ins_at_one_pos_are_ordered_by_type(eng):
    reads = [(0, 400, [(M, 100), (I, 80), (D, 80), (M, 50)])] * 3 + [(1, 400, [(M, 100), (D, 80), (I, 80), (M, 50)])] * 3
    pl = from_reads(2, reads, clip={})
    eng.load_pileup(pl)
    got, _ = check(eng, pl)
    assert [rec(c) for c in got] == [(SVT_INS, 1, 500, 501, 3), (SVT_DEL, 1, 500, 581, 3),
                                     (SVT_DEL, 2, 500, 581, 3), (SVT_INS, 2, 580, 581, 3)]


def test_one_chain_over_many_segments(eng):
    """x = 3000 + 2k, k < 5000: 10 buckets, several segments, one call."""
    pl = from_reads(1, [d_at(3000 + 2 * k, 100 + k % 7) for k in range(5000)], clip={})
    eng.load_pileup(pl)
    got, st = check(eng, pl)
    assert len(got) == 1 and rec(got[0]) == (SVT_DEL, 1, 7999, 8103, 5000)
    assert (int(got[0]["x_lo"]), int(got[0]["x_hi"])) == (3000, 12998) and st["clusters"] == 1
    assert len(check(eng, pl, link=1, min_support=1)[0]) == 5000


def test_big_bucket(eng):
    """3 000 items at one x (more than a tile holds) with varied len, neighbours on both sides."""
    rng = np.random.default_rng(7)
    lens = rng.integers(51, 5000, size=3000)
    reads = [d_at(50500, int(ln)) for ln in lens] + [d_at(50489), d_at(50511), d_at(49000), d_at(52000)]
    reads += [d_at(50500, int(ln), op=I) for ln in lens[:2100]]
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, st = check(eng, pl, min_support=1)
    assert st["big_buckets"] == 2
    assert [int(c["support"]) for c in got] == [1, 1, 2100, 3000, 1, 1]
    big = got[3]
    assert (int(big["len_lo"]), int(big["len_hi"])) == (int(lens.min()), int(lens.max()))
    check(eng, pl, link=11, min_support=1)   # the neighbours join


def test_big_overflow_bucket(eng):
    """More than a tile of items in the contig's last bucket, which holds every value past the
    others: H ops lengthen the walk but not endpos (185 here, ~66 buckets), so x = 300 100 .. 445 503
    all lie in that one bucket, spread over far more than its nominal 1 kb."""
    reads = [(0, 100, [(H, 300000 + 97 * (k % 1500)), (D, 80), (M, 5)]) for k in range(4500)]
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, st = check(eng, pl)
    assert st["big_buckets"] == 1
    assert len(got) == 1500 and (got["support"] == 3).all() and int(got[-1]["pos"]) == 100 + 300000 + 97 * 1499


def test_contigs_do_not_link(eng):
    """The last item of contig 1 (x = 900) and the first of contig 3 (x = 902) are 2 apart in x, with
    the empty contig 2 between them: only the contig boundary keeps them apart."""
    pl = from_reads(3, [d_at(900, tid=0)] * 2 + [d_at(902, tid=2)] * 2, clip={})
    eng.load_pileup(pl)
    for link in (None, 2, 5, 1000):
        got, st = check(eng, pl, link=link, min_support=2)
        assert [rec(c) for c in got] == [(SVT_DEL, 1, 900, 1001, 2), (SVT_DEL, 3, 902, 1003, 2)]
        assert st["clusters"] == 2
    assert len(check(eng, pl, link=1000, min_support=3)[0]) == 0
    # the same across the two types' arrays: INS items of contig 3 at 902 follow DEL items of contig 3
    pl = from_reads(3, [d_at(900, tid=2)] * 2 + [d_at(902, tid=0, op=I)] * 2 + [d_at(901, tid=2, op=I)] * 2, clip={})
    eng.load_pileup(pl)
    got, st = check(eng, pl, link=1000, min_support=2)
    assert [rec(c) for c in got] == [(SVT_INS, 1, 902, 903, 2), (SVT_DEL, 3, 900, 1001, 2), (SVT_INS, 3, 901, 902, 2)]
    assert st["clusters"] == 3


def test_items_at_x_zero(eng):
    pl = from_reads(2, [(1, 0, [(D, 100), (M, 60)])] * 3 + [(1, 0, [(I, 70), (M, 60)])] * 3 + [d_at(8, tid=1, lead=8)], clip={})
    eng.load_pileup(pl)
    got, st = check(eng, pl)
    assert [rec(c) for c in got] == [(SVT_INS, 2, 0, 1, 3), (SVT_DEL, 2, 2, 103, 4)] and st["clusters"] == 2


def test_big_bucket_with_many_starts_and_markers(eng):
    """2 500 items over 900 distinct x of one 1-kb bucket (69 700 .. 70 599, bucket 68) and 400
    trailing-S markers ending in the same bucket: more than a tile holds, not the last bucket."""
    reads = [d_at(69700 + (7 * k) % 900, 60 + k % 11) for k in range(2500)]
    reads += [(0, 69000 + k, [(M, 1000), (S, 20)]) for k in range(400)]
    pl = from_reads(1, reads, clip=None)
    eng.load_pileup(pl)
    got, st = check(eng, pl, link=0, min_support=1)
    assert st["big_buckets"] == 1 and st["events"] == 2500 and len(got) == 900
    check(eng, pl, link=1, min_support=3)
    check(eng, pl)


def test_items_past_2_30_are_skipped(eng):
    big = (1 << 28) - 1
    reads = [(0, 10, [(N, big)] * 3 + [(N, 1000), (D, 100), (M, 5)])] * 3   # x = 1010 + 3 * (2^28 - 1) < 2^30
    reads += [(0, 20, [(N, big)] * 5 + [(D, 100), (M, 5)])] * 4        # x >= 2^30: dropped
    reads += [d_at(500)] * 3
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, st = check(eng, pl)
    assert st["skipped"] == 4 and st["events"] == 10
    assert [rec(c)[2] for c in got] == [500, 1010 + 3 * big]


def test_empty_pileup(eng):
    pl = from_reads(2, [], clip={})
    eng.load_pileup(pl)
    got = eng.call()
    assert len(got) == 0 and got.dtype == CALL_DTYPE and eng.call_stats()["calls"] == 0
    assert eng.call_device() == (0, 0)
    pl = from_reads(1, [(0, 5, [(M, 50)])], clip={})    # reads, no items
    eng.load_pileup(pl)
    check(eng, pl)


@functools.lru_cache(maxsize=None)
def fuzz_pileup(seed, n_reads, max_ops):
    rng = np.random.default_rng(seed)
    hot = [int(x) for x in rng.integers(5000, 55000, size=5)]
    return fuzz.random_pileup(rng, n_targets=2, contig_len=60000, n_reads=n_reads, max_ops=max_ops, hot=hot)


@pytest.mark.parametrize("seed, n_reads, max_ops", [(901, 400, 60), (905, 120, 600)], ids=["short901", "long905"])
def test_fuzz_pileups(eng, seed, n_reads, max_ops):
    pl = fuzz_pileup(seed, n_reads, max_ops)
    eng.load_pileup(pl)
    got, st = check(eng, pl)
    assert len(got) >= 5 and st["events"] > 100
    check(eng, pl, link=3, min_support=2)
    check(eng, pl, link=200, min_support=1)


def test_rescan_after_reindex_and_fetch_windows(eng):
    pl = fuzz_pileup(901, 400, 60)
    eng.load_pileup(pl)
    first, _ = check(eng, pl, min_support=2)
    eng.reindex()
    same(eng.call(min_support=2), first)
    n = len(first)
    assert n > 6
    same(eng.call_fetch(0, n), first)
    same(eng.call_fetch(2, 3), first[2:5])
    same(eng.call_fetch(n - 1, 1), first[n - 1:])
    assert len(eng.call_fetch(n, 0)) == 0
    ptr, cnt = eng.call_device()
    assert ptr != 0 and cnt == n
    for a, b in ((n, 1), (0, n + 1), (n + 1, 0)):
        with pytest.raises(SvtError) as ei:
            eng.call_fetch(a, b)
        assert ei.value.code == SVT_EINVAL


def test_status_codes(eng, monkeypatch):
    with Engine(Params(), device=0) as e0:
        with pytest.raises(SvtError) as ei:
            e0.call()
        assert ei.value.code == SVT_ESTATE
    pl = fuzz_pileup(901, 400, 60)
    eng.load_pileup(pl)
    for kw in ({"link": -1}, {"link": (1 << 20) + 1}, {"min_support": 0}, {"types": ()}):
        with pytest.raises(SvtError) as ei:
            eng.call(**kw)
        assert ei.value.code == SVT_EINVAL, kw
    check(eng, pl, link=1 << 20, min_support=1)
    with pytest.raises(ValueError):
        eng.call(types=("DUP",))
    monkeypatch.setenv("SVTREK_INDEX", "lists")
    with Engine(Params(), device=0) as e1:
        e1.load_pileup(pl)
        with pytest.raises(SvtError) as ei:
            e1.call()
        assert ei.value.code == SVT_ESTATE and "SVTREK_INDEX=lists" in str(ei.value)


def test_min_support_defaults_to_consensus_min_count():
    pl = from_reads(1, [d_at(2000), d_at(2001)] + [d_at(9000)] * 5, clip={})
    with Engine(Params(consensus_min_count=2), device=0) as e:
        e.load_pileup(pl)
        same(e.call(), call_ref.call(pl, min_support=2)[0])
        assert len(e.call()) == 2


def exact_reads():
    """tests/test_call_model.py's exact pileup: 3 DEL sites, 2 INS sites, six reads each."""
    sites = [(D, 100000, 300), (D, 160000, 51), (D, 220000, 4000), (I, 280000, 50), (I, 340000, 900)]
    reads = []
    for op, x, ln in sites:
        for k in range(6):
            lead = 700 + 150 * k
            reads.append((0, x - lead, [(M, lead), (op, ln), (M, 2500 - 100 * k)]))
    return reads


def test_refine_of_the_calls_returns_them(eng):
    pl = from_reads(1, exact_reads(), clip={})
    eng.load_pileup(pl)
    calls, _ = check(eng, pl)
    assert len(calls) == 5
    refined = eng.refine(calls_to_loci(calls))
    assert np.array_equal(refined["start"], calls["pos"])
    is_del = calls["type"] == SVT_DEL
    assert np.array_equal(refined["end"][is_del], calls["end"][is_del]) and (refined["end"][~is_del] == SVT_NA).all()


def test_sim_workload_matches_the_model(eng):
    r = sim.generate(replace(sim.WORKLOADS["cfg4_1m_delins_30x_hifi"], n_loci=2000, n_targets=2))
    eng.load_pileup(r.pileup)
    got, _ = check(eng, r.pileup)
    assert len(got) >= 2000


def write_bam(path, reads, n_ref=1):
    rng = random.Random(1)
    text = b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(b"@SQ\tSN:%d\tLN:1000000\n" % (t + 1) for t in range(n_ref))
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref)
    for t in range(n_ref):
        nm = b"%d\0" % (t + 1)
        raw += struct.pack("<i", len(nm)) + nm + struct.pack("<i", 1000000)
    for k, (tid, pos, ops) in enumerate(sorted(reads, key=lambda r: (r[0], r[1]))):
        raw += bamfix.record(tid, pos, b"r%d" % k, ops, 0, 0, b"", False, rng)
    with open(path, "wb") as f:
        f.write(bamfix.bgzf_blocks(raw))


@pytest.mark.parametrize("inflate", ["cpu", "gpu"])
def test_cli_call_then_audt(tmp_path, inflate):
    reads = exact_reads()
    bam, vcf = str(tmp_path / "x.bam"), str(tmp_path / "c.vcf")
    write_bam(bam, reads)
    p = subprocess.run([CLI, "call", "-b", bam, "-o", vcf, "--inflate", inflate, "--verbose"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout == "" and "calls 5" in p.stderr, p.stderr
    want = host.format_calls(call_ref.call(from_reads(1, reads, clip={}))[0], ["1"])
    with open(vcf) as f:
        assert f.read() == want
    p = subprocess.run([CLI, "call", "-b", bam, "--inflate", inflate, "--types", "INS", "--min-support", "6", "--link", "0"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout == host.format_calls(call_ref.call(from_reads(1, reads, clip={}), 0, 6, (SVT_INS,))[0], ["1"])
    a = subprocess.run([CLI, "audt", "-b", bam, "-v", vcf, "--inflate", inflate], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert a.returncode == 0, a.stderr
    lines = [ln for ln in a.stdout.splitlines() if ln.startswith("(")]
    dels, inss = [ln for ln in lines if ln.startswith("(DEL)")], [ln for ln in lines if ln.startswith("(INS)")]
    assert len(dels) == 3 and len(inss) == 2
    assert all(ln.endswith("diff pos: 0, diff end: 0") for ln in dels), dels
    assert all(ln.endswith("diff: 0") for ln in inss), inss
    bad = subprocess.run([CLI, "call", "-b", bam, "--types", "DUP"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert bad.returncode == 1 and "--types" in bad.stderr
    disc = subprocess.run([CLI, "disc"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert disc.returncode == 1 and "disc mode is not part of svtrek_amd" in disc.stderr
