"""svt_call_params.len_permille on the HIP engine: Engine.call(len_permille=P) against the numpy model
(tests/call_split_ref.py, pinned by tests/test_call_split_model.py), record for record and both stats,
on pileups built to reach every path of the split in svt_call.inc (candidates next to other clusters,
chains over segments with sentinels in between, big candidates of both big-bucket kinds, many groups
in one cluster), the lifecycle of its scratch, genotype_calls on split calls, and the CLI."""
import functools
import os
import subprocess

import numpy as np
import pytest

from svtrek_amd import Engine, Params, SvtError, calls_to_sites, from_reads, host
from svtrek_amd._lib import CALL_DTYPE, SVT_DEL, SVT_EINVAL, SVT_INS, has_call_split

import call_ref
import call_split_ref
import fuzz
import genotype_ref
from test_gpu_call import write_bam

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


def check(eng, pl, P=100, link=None, min_support=None, types=("DEL", "INS")):
    """Engine.call(len_permille=P) == the model, both stats too; returns (calls, stats, split stats)."""
    want, wst, wsp = call_split_ref.call(pl, 10 if link is None else link, 3 if min_support is None else min_support,
                                         tuple(NAMES[t] for t in types), P)
    got = eng.call(link=link, min_support=min_support, types=types, len_permille=P)
    same(got, want)
    st, sp = eng.call_stats(), eng.call_split_stats()
    assert {k: st[k] for k in wst} == wst
    assert sp == wsp
    return got, st, sp


def d_at(x, ln=100, tid=0, lead=200, op=D, tail=60):
    return (tid, x - lead, [(M, lead), (op, ln), (M, tail)])


def rec(c):
    return tuple(int(c[f]) for f in ("type", "pos", "end", "len", "support"))


@pytest.fixture(scope="module")
def eng():
    with Engine(Params(), device=0) as e:
        assert has_call_split(e.lib)
        yield e


def worked_reads():
    return [d_at(x, 300, lead=50) for x in (100, 100, 100, 110)] + [d_at(104, 500, lead=50)] * 3


def test_worked_example(eng):
    pl = from_reads(1, worked_reads(), clip={})
    eng.load_pileup(pl)
    got, st, sp = check(eng, pl, 100)
    assert [rec(c) for c in got] == [(SVT_DEL, 103, 404, 300, 4), (SVT_DEL, 104, 605, 500, 3)]
    assert st["clusters"] == 1 and sp == {"candidates": 1, "split": 1, "groups": 2, "big": 0}
    got, _, sp = check(eng, pl, 0)
    assert [rec(c) for c in got] == [(SVT_DEL, 103, 490, 386, 7)] and sp == call_split_ref.SPLIT_ZERO


@pytest.mark.parametrize("a, b, link, P, n", [(300, 330, 10, 100, 1), (300, 331, 10, 100, 2), (60, 70, 10, 100, 1),
                                               (60, 71, 10, 100, 2), (309, 339, 10, 100, 1), (309, 340, 10, 100, 2),
                                               (300, 600, 10, 1000, 1), (300, 601, 10, 1000, 2), (300, 350, 50, 100, 1),
                                               (300, 351, 50, 100, 2)])
def test_gap_thresholds(eng, a, b, link, P, n):
    pl = from_reads(1, [d_at(1000, a)] * 3 + [d_at(1000, b)] * 3, clip={})
    eng.load_pileup(pl)
    got, _, sp = check(eng, pl, P, link=link)
    assert len(got) == n and sp["candidates"] == n - 1


def test_single_linkage_and_min_support_per_group(eng):
    pl = from_reads(1, [d_at(1000, ln) for ln in (300, 320, 340, 360)], clip={})
    eng.load_pileup(pl)
    got, _, sp = check(eng, pl, 100)
    assert [rec(c)[3:] for c in got] == [(330, 4)] and sp == {"candidates": 1, "split": 0, "groups": 1, "big": 0}
    pl = from_reads(1, [d_at(1000, 300)] * 3 + [d_at(1001, 500)] * 2, clip={})     # 3 + 2
    eng.load_pileup(pl)
    got, _, sp = check(eng, pl, 100)
    assert [rec(c)[1:] for c in got] == [(1000, 1301, 300, 3)] and sp["groups"] == 2
    pl = from_reads(1, [d_at(1000, 300)] * 2 + [d_at(1001, 500)] * 2 + [d_at(1002, 900)], clip={})   # 2 + 2 + 1
    eng.load_pileup(pl)
    got, _, sp = check(eng, pl, 100)
    assert len(got) == 0 and sp == {"candidates": 1, "split": 1, "groups": 3, "big": 0}
    assert len(check(eng, pl, 100, min_support=2)[0]) == 2
    assert len(check(eng, pl, 100, min_support=6)[0]) == 0     # 5 items: no candidate


def test_del_and_ins_both_split_at_one_pos(eng):
    reads = [(0, 400, [(M, 100), (I, 80), (D, 80), (M, 50)])] * 3 + [(0, 400, [(M, 100), (I, 800), (D, 800), (M, 50)])] * 3
    reads += [(1, 400, [(M, 100), (D, 90), (M, 50)])] * 3
    pl = from_reads(2, reads, clip={})
    eng.load_pileup(pl)
    got, _, sp = check(eng, pl, 100)
    assert [rec(c)[:2] + rec(c)[3:4] for c in got] == [(SVT_INS, 500, 80), (SVT_INS, 500, 800), (SVT_DEL, 500, 80),
                                                        (SVT_DEL, 500, 800), (SVT_DEL, 500, 90)]
    assert sp == {"candidates": 2, "split": 2, "groups": 4, "big": 0}
    check(eng, pl, 100, types=("INS",))
    check(eng, pl, 100, types=("DEL",))


def test_pos_order_against_len_order_and_equal_pos(eng):
    reads = [d_at(1008, 300)] * 3 + [d_at(1004, 500)] * 3 + [d_at(1000, 900)] * 3     # len up, pos down
    reads += [d_at(5000, 900)] * 3 + [d_at(5000, 300)] * 3                             # one pos
    reads += [d_at(9000 + k, ln) for ln in (100, 200, 400) for k in (0, 1, 2)]          # one pos again (9001), three groups
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, _, _ = check(eng, pl, 100)
    assert [rec(c)[1::2] for c in got] == [(1000, 900), (1004, 500), (1008, 300), (5000, 300), (5000, 900),
                                            (9001, 100), (9001, 200), (9001, 400)]


def test_cluster_across_a_bucket_edge(eng):
    xs = (1020, 1022, 1024, 1027, 1030)   # buckets 0 and 1
    pl = from_reads(1, [d_at(x, 300) for x in xs] + [d_at(x, 500) for x in xs[1:]], clip={})
    eng.load_pileup(pl)
    got, _, _ = check(eng, pl, 100)
    assert [rec(c)[1:] for c in got] == [(1025, 1326, 300, 5), (1026, 1527, 500, 4)]


def test_one_chain_over_many_segments(eng):
    """x = 3000 + 2k, k < 5000, over ten buckets with two alternating lengths: one candidate of more
    items than a tile holds whose keys lie in several segments, with sentinels (the trailing-S markers
    of other reads, filed in the same buckets) behind every segment's keys."""
    reads = [d_at(3000 + 2 * k, 300 if k % 2 == 0 else 500) for k in range(5000)]
    reads += [(0, 2000 + 500 * k, [(M, 1000), (S, 20)]) for k in range(20)]    # markers inside the chain's buckets
    pl = from_reads(1, reads, clip=None)
    eng.load_pileup(pl)
    got, st, sp = check(eng, pl, 100)
    assert [rec(c) for c in got] == [(SVT_DEL, 7998, 8299, 300, 2500), (SVT_DEL, 8000, 8501, 500, 2500)]
    assert st["clusters"] == 1 and sp == {"candidates": 1, "split": 1, "groups": 2, "big": 1}
    assert len(check(eng, pl, 100, link=1, min_support=1)[0]) == 5000      # 5 000 clusters of one item: no candidate


def test_big_bucket_at_one_x(eng):
    """3 000 items at one x (the counting-sort bucket) with three lengths, neighbours on both sides."""
    reads = [d_at(50500, (300, 500, 900)[k % 3]) for k in range(3000)] + [d_at(50489), d_at(50511), d_at(49000), d_at(52000)]
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, st, sp = check(eng, pl, 100, min_support=1)
    assert st["big_buckets"] == 1 and sp["candidates"] == 1 and sp["big"] == 1 and sp["groups"] == 3
    assert sorted(int(c["support"]) for c in got) == [1, 1, 1, 1, 1000, 1000, 1000]
    check(eng, pl, 100, link=11, min_support=1)   # the neighbours (len 100) join: a fourth group
    check(eng, pl, 100)


def test_big_overflow_bucket(eng):
    """4 500 items in the contig's last bucket (test_gpu_call.py's layout), two lengths per start."""
    reads = [(0, 100, [(H, 300000 + 97 * (k % 1500)), (D, 80 if k // 1500 != 1 else 400), (M, 5)]) for k in range(4500)]
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, st, sp = check(eng, pl, 100, min_support=1)
    assert st["big_buckets"] == 1 and len(got) == 3000 and sp == {"candidates": 1500, "split": 1500, "groups": 3000, "big": 0}
    check(eng, pl, 100)                                  # 2 + 1 at min_support 3: no call
    got, _, sp = check(eng, pl, 100, link=97)           # one start cluster of 4 500
    assert [int(c["support"]) for c in got] == [3000, 1500] and sp["big"] == 1


def test_six_hundred_groups_in_one_cluster(eng):
    """600 items at one start with lengths 100 + 40 i: 600 calls from one cluster, whose order by
    (pos, len) is the reverse of some of their len order once the starts differ."""
    pl = from_reads(1, [d_at(7000, 100 + 40 * i) for i in range(600)], clip={})
    eng.load_pileup(pl)
    got, _, sp = check(eng, pl, 1, min_support=1)        # (P = 1: the link floor of 10 decides everywhere)
    assert len(got) == 600 and sp == {"candidates": 1, "split": 1, "groups": 600, "big": 0}
    assert np.array_equal(got["len"], 100 + 40 * np.arange(600))
    pl = from_reads(1, [d_at(7000 + (7 * i) % 10, 100 + 40 * i) for i in range(600)], clip={})
    eng.load_pileup(pl)
    got, _, _ = check(eng, pl, 1, min_support=1)
    assert len(got) == 600 and len(np.unique(got["pos"])) == 10
    # more groups than a tile holds: the order kernel's sort in device memory
    lens = [100]
    while len(lens) < 2500:
        lens.append(lens[-1] + max(10, lens[-1] // 1000) + 1)      # one more than the gap allowed: a cut everywhere
    pl = from_reads(1, [d_at(7000 + (7 * i) % 10, ln) for i, ln in enumerate(lens)], clip={})
    eng.load_pileup(pl)
    got, _, sp = check(eng, pl, 1, min_support=1)
    assert len(got) == 2500 and sp["big"] == 1


def test_trailing_soft_clips_at_the_clusters_x(eng):
    reads = [d_at(8000, 300)] * 3 + [d_at(8001, 500)] * 3 + [(0, 7000 + k, [(M, 1000 - k), (S, 30)]) for k in range(5)]
    pl = from_reads(1, reads, clip=None)
    eng.load_pileup(pl)
    got, st, _ = check(eng, pl, 100)
    assert [rec(c)[1:] for c in got] == [(8000, 8301, 300, 3), (8001, 8502, 500, 3)] and st["events"] == 6


def test_candidate_between_other_clusters(eng):
    reads = [d_at(4000, 300)] * 4 + [d_at(4020, 300)] * 3 + [d_at(4021, 500)] * 4 + [d_at(4040, 500)] * 3
    reads += [d_at(4020, 90, op=I)] * 3 + [d_at(4060, 70), d_at(4061, 700)]     # the last: too few items
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, st, sp = check(eng, pl, 100)
    assert [rec(c) for c in got] == [(SVT_DEL, 4000, 4301, 300, 4), (SVT_INS, 4020, 4021, 90, 3), (SVT_DEL, 4020, 4321, 300, 3),
                                     (SVT_DEL, 4021, 4522, 500, 4), (SVT_DEL, 4040, 4541, 500, 3)]
    assert st["clusters"] == 5 and sp == {"candidates": 1, "split": 1, "groups": 2, "big": 0}
    unsplit = eng.call()
    same(unsplit[[0, 1, 3]], got[[0, 1, 4]])                 # the neighbours' records are the unsplit scan's


def test_parameter_edges(eng):
    pl = from_reads(1, worked_reads() + [d_at(104, 1001, lead=50)] * 3, clip={})
    eng.load_pileup(pl)
    got, _, _ = check(eng, pl, 1000)
    assert [rec(c)[3:] for c in got] == [(386, 7), (1001, 3)]     # 500 -> 1001 is one more than 500 * 1000 / 1000
    got = eng.call(len_permille=0)
    same(got, call_ref.call(pl)[0])
    assert eng.call_split_stats() == call_split_ref.SPLIT_ZERO
    with pytest.raises(SvtError) as ei:
        eng.call(len_permille=1001)
    assert ei.value.code == SVT_EINVAL
    pl = from_reads(2, [], clip={})
    eng.load_pileup(pl)
    assert len(eng.call(len_permille=100)) == 0 and eng.call_split_stats() == call_split_ref.SPLIT_ZERO
    pl = from_reads(1, [(0, 5, [(M, 50)])], clip={})    # reads, no items
    eng.load_pileup(pl)
    check(eng, pl, 100)


@functools.lru_cache(maxsize=None)
def fuzz_pileup(seed, n_reads, max_ops):
    """tests/test_gpu_call.py's generator (a copy)."""
    rng = np.random.default_rng(seed)
    hot = [int(x) for x in rng.integers(5000, 55000, size=5)]
    return fuzz.random_pileup(rng, n_targets=2, contig_len=60000, n_reads=n_reads, max_ops=max_ops, hot=hot)


@pytest.mark.parametrize("seed, n_reads, max_ops", [(901, 400, 60), (905, 120, 600)], ids=["short901", "long905"])
def test_fuzz_pileups(eng, seed, n_reads, max_ops):
    pl = fuzz_pileup(seed, n_reads, max_ops)
    eng.load_pileup(pl)
    cands = 0
    for P in (50, 200, 1000):
        for ms in (1, 3):
            cands += check(eng, pl, P, min_support=ms)[2]["split"]
    assert cands > 0
    check(eng, pl, 50, link=200, min_support=1)


def test_lifecycle(eng):
    pl = fuzz_pileup(901, 400, 60)
    eng.load_pileup(pl)
    first, _, sp = check(eng, pl, 50, min_support=2)
    assert sp["split"] > 0
    plain = eng.call(min_support=2)
    same(plain, call_ref.call(pl, min_support=2)[0])
    assert eng.call_split_stats() == call_split_ref.SPLIT_ZERO
    with Engine(Params(), device=0) as fresh:               # a P = 0 scan after a split scan equals a fresh one
        fresh.load_pileup(pl)
        same(plain, fresh.call(min_support=2))
        assert fresh.call_stats()["clusters"] == eng.call_stats()["clusters"]
    same(eng.call(min_support=2, len_permille=50), first)
    eng.reindex()
    same(eng.call(min_support=2, len_permille=50), first)
    assert eng.call_split_stats() == sp
    same(eng.call_fetch(1, 3), first[1:4])


def carrier(x, ln, lead=2000, tail=3000):
    return (0, x - lead, [(M, lead), (D, ln), (M, tail)])


def test_genotype_calls_after_a_split_scan(eng):
    reads = [carrier(7000, 300)] * 4 + [carrier(7000, 500)] * 3 + [(0, 5000, [(M, 5000)])] * 2    # 9 spanning reads
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    calls, _, _ = check(eng, pl, 100)
    got = eng.genotype_calls()
    want = genotype_ref.genotype(pl, calls_to_sites(calls))
    assert np.array_equal(got, want)
    assert [tuple(int(g[f]) for f in ("alt", "ref", "span", "alt_all")) for g in got] == [(4, 5, 9, 4), (3, 6, 9, 3)]
    assert [int(g["gt"]) for g in got] == [1, 1]            # two 0/1 records
    pl = fuzz_pileup(901, 400, 60)
    eng.load_pileup(pl)
    for P, ms in ((50, 1), (200, 3)):
        calls, _, _ = check(eng, pl, P, min_support=ms)
        got = eng.genotype_calls()
        assert np.array_equal(got, genotype_ref.genotype(pl, calls_to_sites(calls)))
        assert np.array_equal(got["alt_all"], calls["support"])


def cli_reads():
    reads = []
    for x, lens in ((100000, (300, 500)), (160000, (51, 51)), (220000, (4000, 400))):
        for k in range(8):
            lead = 700 + 150 * k
            reads.append((0, x - lead, [(M, lead), (D, lens[k % 2]), (M, 2500 - 100 * k)]))
    for k in range(8):
        lead = 700 + 150 * k
        reads.append((0, 280000 - lead, [(M, lead), (I, (60, 900)[k % 2]), (M, 2500 - 100 * k)]))
    return reads


@pytest.mark.parametrize("inflate", ["cpu", "gpu"])
def test_cli_len_permille(tmp_path, inflate):
    reads = cli_reads()
    bam, vcf = str(tmp_path / "x.bam"), str(tmp_path / "c.vcf")
    write_bam(bam, reads)
    pl = from_reads(1, reads, clip={})
    want = call_split_ref.call(pl, len_permille=100)[0]
    assert len(want) == 7

    def run(*args):
        return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    p = run("call", "-b", bam, "-o", vcf, "--inflate", inflate, "--len-permille", "100", "--verbose")
    assert p.returncode == 0 and p.stdout == "" and "calls 7" in p.stderr and "candidates 3  split 3  groups 6" in p.stderr, p.stderr
    with open(vcf) as f:
        assert f.read() == host.format_calls(want, ["1"])
    p = run("call", "-b", bam, "--inflate", inflate, "--len-permille", "100", "--genotype")
    assert p.returncode == 0 and p.stdout == host.format_calls(want, ["1"], genotypes=genotype_ref.genotype(pl, calls_to_sites(want)))
    a = run("audt", "-b", bam, "-v", vcf, "--inflate", inflate)
    assert a.returncode == 0, a.stderr
    lines = [ln for ln in a.stdout.splitlines() if ln.startswith("(")]
    assert len([ln for ln in lines if ln.startswith("(DEL)")]) == 5 and len([ln for ln in lines if ln.startswith("(INS)")]) == 2
    p = run("call", "-b", bam, "--inflate", inflate)                        # without the flag: the format as it was
    assert p.returncode == 0 and p.stdout == host.format_calls(call_ref.call(pl)[0], ["1"])
    p = run("call", "-b", bam, "--inflate", inflate, "--len-permille", "0")
    assert p.returncode == 0 and p.stdout == host.format_calls(call_ref.call(pl)[0], ["1"])
    for bad in ("1001", "-1"):
        p = run("call", "-b", bam, "--len-permille", bad)
        assert p.returncode == 1 and "--len-permille" in p.stderr
