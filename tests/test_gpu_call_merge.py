"""svt_call_params.merge_gap / merge_min on the HIP engine: Engine.call(merge_gap=G) against the numpy
model (tests/call_merge_ref.py, pinned by tests/test_call_merge_model.py), record for record and every
stat, on reads built to reach every path of the walk in svt_callmerge.inc (64 ops a trip, 16 in a
pileup of short reads: fragments on both sides of a trip boundary, runs over several trips, open runs at the read's end), the shape of the
merged index (bucket edges, a contig's last bucket, a big bucket), its lifecycle, genotype_calls on
merged calls, and the CLI."""
import functools
import os
import subprocess

import numpy as np
import pytest

from svtrek_amd import Engine, Params, SvtError, calls_to_sites, from_reads, host
from svtrek_amd._lib import CALL_DTYPE, SVT_DEL, SVT_EINVAL, SVT_ESTATE, SVT_INS, has_call_merge

import call_merge_ref as R
import fuzz
from test_gpu_call import write_bam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "svtrek_amd", "svtrek")
M, I, D, N, S, H, P = 0, 1, 2, 3, 4, 5, 6
NAMES = {"DEL": SVT_DEL, "INS": SVT_INS}
INT_STATS = ("fragments", "runs", "joined_items", "items")


def same(got, want):
    assert got.dtype == CALL_DTYPE and want.dtype == CALL_DTYPE
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(want)} records differ; first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


def check(eng, pl, G=50, m=20, link=None, min_support=None, types=("DEL", "INS"), P=0):
    """Engine.call(merge_gap=G, merge_min=m) == the model, the three stats too; returns (calls, stats, merge stats)."""
    want, wst, wsp, wms = R.call(pl, 10 if link is None else link, 3 if min_support is None else min_support,
                                 tuple(NAMES[t] for t in types), P, G, m)
    got = eng.call(link=link, min_support=min_support, types=types, len_permille=P, merge_gap=G, merge_min=m)
    same(got, want)
    st, ms = eng.call_stats(), eng.call_merge_stats()
    assert {k: st[k] for k in wst} == wst
    assert eng.call_split_stats() == wsp
    assert {k: ms[k] for k in INT_STATS} == wms
    return got, st, ms


def rec(c):
    return tuple(int(c[f]) for f in ("type", "pos", "end", "len", "support"))


def run_of(x, ops, pos=None, tid=0, tail=60, lead_op=M):
    """A read whose first op after the lead lies at walk position x."""
    pos = x - 200 if pos is None else pos
    return (tid, pos, [(lead_op, x - pos)] + list(ops) + [(M, tail)])


def frag(n=4, x=1000, a=180, gap=5, b=120, op=D, **kw):
    return [run_of(x, [(op, a), (M, gap), (op, b)], **kw)] * n


@pytest.fixture(scope="module")
def eng():
    with Engine(Params(), device=0) as e:
        assert has_call_merge(e.lib)
        yield e


def test_the_issues_example(eng):
    pl = from_reads(1, frag(), clip={})
    eng.load_pileup(pl)
    got, st, ms = check(eng, pl)
    assert [rec(c) for c in got] == [(SVT_DEL, 1000, 1301, 300, 4)]
    assert {k: ms[k] for k in INT_STATS} == {"fragments": 8, "runs": 4, "joined_items": 4, "items": 4} and ms["build_ms"] > 0
    plain = eng.call()
    assert [rec(c)[1:] for c in plain] == [(1000, 1181, 180, 4), (1185, 1306, 120, 4)]
    assert eng.call_merge_stats() == {**R.MERGE_ZERO, "build_ms": 0.0}


@pytest.mark.parametrize("op, a, b, n", [(D, 30, 30, 1), (D, 25, 25, 0), (I, 25, 25, 1), (I, 25, 24, 0), (D, 26, 25, 1)])
def test_sums_at_the_threshold(eng, op, a, b, n):
    pl = from_reads(1, frag(3, a=a, gap=2 if a == 25 else 3, b=b, op=op), clip={})
    eng.load_pileup(pl)
    got, _, ms = check(eng, pl)
    assert len(got) == n and ms["runs"] == 3 and ms["items"] == 3 * n
    if n:
        assert int(got[0]["len"]) == a + b


@pytest.mark.parametrize("op", [D, I])
@pytest.mark.parametrize("G", [1, 50, 1 << 20])
def test_distance_exactly_the_gap_and_one_more(eng, op, G):
    """DEL: from the tail (x + len) of the fragment before; INS: from its x."""
    reads = frag(3, x=5000, a=60, gap=G, b=70, op=op, pos=4000) + frag(3, x=9000, a=60, gap=G + 1, b=70, op=op, pos=8000)
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, _, ms = check(eng, pl, G=G, link=0)              # (link 0: items 2 apart stay two clusters)
    second = 9000 + G + 1 + (60 if op == D else 0)
    assert [(int(c["pos"]), int(c["len"])) for c in got] == [(5000, 130), (9000, 60), (second, 70)]
    assert ms["joined_items"] == 3 and ms["runs"] == 9


def test_fragment_of_merge_min_and_one_less(eng):
    reads = frag(3, x=2000, a=40, b=20) + frag(3, x=4000, a=40, b=19) + frag(3, x=6000, a=49, gap=1, b=1)
    reads += [run_of(8000, [(D, 40), (M, 20), (D, 19), (M, 11), (D, 40)])] * 3      # the 19D adds 19 to the distance: 50
    reads += [run_of(9000, [(D, 40), (M, 20), (D, 19), (M, 12), (D, 40)])] * 3      # 51
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, _, _ = check(eng, pl)
    assert [(int(c["pos"]), int(c["len"])) for c in got] == [(2000, 60), (8000, 80)]
    got, _, _ = check(eng, pl, m=19)
    assert [(int(c["pos"]), int(c["len"])) for c in got] == [(2000, 60), (4000, 59), (8000, 99), (9000, 99)]
    check(eng, pl, m=1)                                                              # 49D 1M 1D: sum 50, no DEL item
    assert len(check(eng, pl, m=50)[0]) == 0                                         # no fragment at all


def test_single_linkage_and_types_apart(eng):
    reads = [run_of(3000, [(D, 30), (M, 50), (D, 30), (M, 50), (D, 30)])] * 3       # each at G: span past G
    reads += [run_of(7000, [(D, 40), (M, 2), (I, 40), (M, 2), (D, 40), (M, 2), (I, 40)])] * 3
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, _, _ = check(eng, pl)
    assert [rec(c)[:2] + rec(c)[3:] for c in got] == [(SVT_DEL, 3000, 90, 3), (SVT_DEL, 7000, 80, 3), (SVT_INS, 7042, 80, 3)]
    check(eng, pl, types=("INS",))
    check(eng, pl, types=("DEL",))


@pytest.mark.parametrize("op, joined", [(N, False), (H, False), (P, False), (11, False), (S, True), (I, True)])
def test_ops_between_fragments(eng, op, joined):
    """N, H, P and the codes 9-15 count in the distance, S and I do not."""
    pl = from_reads(1, [run_of(1000, [(D, 40), (M, 30), (op, 21), (D, 40)])] * 3, clip={})
    eng.load_pileup(pl)
    got, _, _ = check(eng, pl, m=22)
    assert len(got) == (1 if joined else 0)


def pad(n):
    """n ops that are no fragments and advance the walk by n."""
    return [(M, 1), (7, 1)] * (n // 2) + [(M, 1)] * (n % 2)


@pytest.mark.parametrize("lead, ops", [
    (62, [(D, 30), (M, 3), (D, 30)]),                    # ops 62 and 64: an M ends the trip between them
    (63, [(D, 30), (D, 30)]),                            # ops 63 and 64: the last of one trip, the first of the next
    (63, [(I, 30), (I, 30)]),
    (61, [(D, 20)] + pad(63) + [(D, 20)] + pad(63) + [(D, 20)]),     # a run over three trips (ops 61, 125, 189), 63 apart
    (0, [(D, 30)] + pad(40) + [(D, 30)] + pad(120) + [(D, 60)] + pad(30) + [(D, 55)]),   # closed by a later trip's head
    (130, [(D, 25), (M, 1), (I, 30), (D, 25), (I, 30), (D, 25)]),
])
@pytest.mark.parametrize("filler", [0, 40], ids=["wave", "team16"])
def test_trip_boundaries(eng, lead, ops, filler):
    """filler: short reads that bring the pileup's mean below 64 ops a read, where the build walks with 16
    lanes a read and 16 ops a trip (every 64-op boundary is one of those too)."""
    reads = [(0, 500, pad(lead) + list(ops) + [(M, 60)])] * 3 + [(0, 90000 + k, [(M, 50)]) for k in range(filler)]
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, _, ms = check(eng, pl, G=64)
    assert len(got) >= 1 and ms["joined_items"] >= 3
    check(eng, pl, G=62)
    check(eng, pl, G=1)


@pytest.mark.parametrize("nops", [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129])
def test_read_lengths_around_the_trip_width(eng, nops):
    """Reads of exactly nops ops whose last op is a fragment that joins the one before it: the run is
    still open at the read's end; nops = 1: a read that is one fragment only."""
    if nops == 1:
        reads = [(0, 700, [(D, 80)])] * 3 + [(0, 900, [(I, 80)])] * 3
    else:
        reads = [(0, 700, pad(nops - 2) + [(D, 30), (D, 30)])] * 3
        reads += [(0, 700, [(I, 30)] + pad(nops - 2) + [(I, 30)])] * 3
    pl = from_reads(1, reads, clip={})
    assert all(int(n) == nops for n in np.diff(pl.cig_off.astype(np.int64)))
    eng.load_pileup(pl)
    got, _, ms = check(eng, pl, G=200)
    assert len(got) == 2 and ms["items"] == 6
    check(eng, pl, G=1)


@functools.lru_cache(maxsize=None)
def fuzz_case(seed, n_reads, max_ops):
    rng = np.random.default_rng(seed)
    hot = [int(x) for x in rng.integers(5000, 55000, size=5)]
    pl = fuzz.random_pileup(rng, n_targets=2, contig_len=60000, n_reads=n_reads, max_ops=max_ops, hot=hot)
    return pl, R.fragment(pl, np.random.default_rng(seed + 1), 50, 20)


@pytest.mark.parametrize("seed, n_reads, max_ops", [(901, 400, 60), (905, 120, 600)], ids=["short901", "long905"])
def test_fuzz_pileups_of_both_filing_paths(eng, seed, n_reads, max_ops):
    pl, (fr, eligible, cut) = fuzz_case(seed, n_reads, max_ops)
    eng.load_pileup(pl)
    whole, _, ms = check(eng, pl, min_support=2)
    assert ms["joined_items"] > 0                         # (LEN_CHOICES' short M runs: the fuzz joins by itself)
    check(eng, pl, G=1, m=50)
    check(eng, pl, G=1 << 20, m=1, link=200, min_support=1)
    check(eng, pl, G=300, m=20, P=100, min_support=1)
    eng.load_pileup(fr)
    got, _, _ = check(eng, fr, min_support=2)
    assert cut > 0
    same(got, whole)


def test_run_across_a_bucket_edge(eng):
    """The run starts in bucket 0 (x = 1020) while its later fragments lie in bucket 1."""
    reads = [run_of(1020 + k, [(D, 30), (M, 2), (D, 30), (M, 2), (D, 30)], pos=500) for k in range(5)]
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, _, _ = check(eng, pl)
    assert [rec(c) for c in got] == [(SVT_DEL, 1022, 1113, 90, 5)]


def test_last_bucket_and_an_empty_contig(eng):
    """H ops lengthen the walk but not endpos: the runs lie in their contig's last bucket, far past its
    nominal 1 kb; contig 2 is empty, and contig 3's items follow contig 1's in the merged index."""
    ops = [(D, 30), (M, 5), (D, 30)]
    reads = [(0, 100, [(H, 300000 + 10 * (k // 3))] + ops + [(M, 5)]) for k in range(9)]
    reads += [(2, 100, [(H, 300002)] + ops + [(M, 5)])] * 3 + frag(3, x=900, tid=2)
    pl = from_reads(3, reads, clip={})
    eng.load_pileup(pl)
    got, _, _ = check(eng, pl)
    assert [(int(c["chrom"]), int(c["pos"]), int(c["len"])) for c in got] == [(1, 300110, 60), (3, 900, 300), (3, 300102, 60)]
    assert len(check(eng, pl, link=1000)[0]) == 3        # the contigs do not link


def test_big_bucket_of_the_merged_index(eng):
    """3 000 merged items at one x: more than the tile sort holds."""
    reads = frag(3000, x=50500, a=40, b=40) + frag(1, x=50489, a=40, b=41) + frag(1, x=52000, a=30, b=30)
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, st, ms = check(eng, pl, min_support=1)
    assert st["big_buckets"] == 1 and ms["items"] == 3002 and sorted(int(c["support"]) for c in got) == [1, 1, 3000]
    assert len(eng.call(min_support=1)) == 0 and eng.call_stats()["big_buckets"] == 0      # no single op is an item


def test_runs_around_2_30(eng):
    big = (1 << 28) - 1
    lead = [(N, big)] * 3 + [(N, (1 << 30) - 3 * big - 110)]                # x = 2^30 - 100 after it, from pos 10
    reads = [(0, 10, lead + [(D, 40), (M, 80), (D, 40), (M, 5)])] * 3       # the second fragment past 2^30: kept
    reads += [(0, 10, lead + [(M, 100), (D, 40), (M, 8), (D, 40), (M, 5)])] * 4      # the first at 2^30: skipped
    reads += [(0, 10, lead + [(M, 5000), (I, 40), (M, 8), (I, 40), (M, 5)])] * 2
    reads += frag(3, x=500)
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, st, ms = check(eng, pl, G=100)
    assert [(int(c["pos"]), int(c["len"])) for c in got] == [(500, 300), ((1 << 30) - 100, 80)]
    assert st["skipped"] == 6 and st["events"] == 12 and ms["items"] == 12


def test_split_by_length_on_merged_items(eng):
    reads = frag(4, x=1000) + [run_of(1000, [(D, 500)])] * 4
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    got, _, _ = check(eng, pl, P=100)
    assert [rec(c)[1:] for c in got] == [(1000, 1301, 300, 4), (1000, 1501, 500, 4)]
    assert len(check(eng, pl, P=0)[0]) == 1


def carrier(x, ops, lead=2000, tail=3000):
    return (0, x - lead, [(M, lead)] + list(ops) + [(M, tail)])


def test_genotype_calls_after_a_merged_scan(eng):
    reads = [carrier(7000, [(D, 180), (M, 5), (D, 120)])] * 4 + [(0, 5000, [(M, 5000)])] * 4
    pl = from_reads(1, reads, clip={})
    eng.load_pileup(pl)
    calls, _, _ = check(eng, pl)
    got = eng.genotype_calls()
    assert np.array_equal(got, R.genotype(pl, calls_to_sites(calls), 50))
    assert [tuple(int(g[f]) for f in ("alt", "ref", "span", "alt_all", "gt")) for g in got] == [(4, 4, 8, 4, 1)]   # 0/1, DV 4, DR 4
    # sites through the batch entry point keep seeing the single ops: no 300 bp item there
    assert int(eng.genotype(calls_to_sites(calls))[0]["alt_all"]) == 0
    pl, (fr, _, _) = fuzz_case(901, 400, 60)
    eng.load_pileup(fr)
    for G, ms_ in ((50, 1), (300, 3)):
        calls, _, _ = check(eng, fr, G=G, min_support=ms_)
        got = eng.genotype_calls()
        assert np.array_equal(got, R.genotype(fr, calls_to_sites(calls), G))
        assert np.array_equal(got["alt_all"], calls["support"])
    plain = eng.call(min_support=1)
    assert np.array_equal(eng.genotype_calls()["alt_all"], plain["support"])     # the plain index again


def test_lifecycle(eng):
    pl, (fr, _, _) = fuzz_case(901, 400, 60)
    eng.load_pileup(fr)
    first, _, ms = check(eng, fr, min_support=2)
    again, _, ms2 = check(eng, fr, min_support=2, link=3)                  # the same (G, m): the index is kept
    assert ms2 == ms
    eng.reindex()
    same(eng.call(min_support=2, merge_gap=50, merge_min=20), first)
    assert eng.call_merge_stats() == ms
    same(eng.call_fetch(1, 3), first[1:4])
    other, _, ms3 = check(eng, fr, G=51, min_support=2)                    # a change of G or m rebuilds it
    other, _, ms4 = check(eng, fr, G=51, m=30, min_support=2)
    assert ms4["fragments"] < ms3["fragments"]
    same(check(eng, fr, min_support=2)[0], first)
    plain = eng.call(min_support=2)                                        # a plain scan after a merged one
    want, wst, _, _ = R.call(fr, min_support=2)
    same(plain, want)
    st = eng.call_stats()
    assert {k: st[k] for k in wst} == wst and eng.call_merge_stats() == {**R.MERGE_ZERO, "build_ms": 0.0}
    with Engine(Params(), device=0) as fresh:
        fresh.load_pileup(fr)
        same(plain, fresh.call(min_support=2))
        assert fresh.call_merge_stats() == {**R.MERGE_ZERO, "build_ms": 0.0}
    eng.load_pileup(pl)                                                    # a new pileup: a new merged index
    check(eng, pl, min_support=2)
    eng.load_pileup(from_reads(2, [], clip={}))
    assert len(eng.call(merge_gap=50)) == 0 and eng.call_merge_stats() == {**R.MERGE_ZERO, "build_ms": 0.0}
    pl0 = from_reads(1, [(0, 5, [(M, 50)])], clip={})                      # reads, no fragments
    eng.load_pileup(pl0)
    check(eng, pl0)


def test_status_codes(eng):
    pl = from_reads(1, frag(), clip={})
    eng.load_pileup(pl)
    for kw in ({"merge_gap": (1 << 20) + 1}, {"merge_gap": 50, "merge_min": 0}, {"merge_gap": 50, "merge_min": 51},
               {"merge_gap": 1, "merge_min": 1 << 31}):
        with pytest.raises(SvtError) as ei:
            eng.call(**kw)
        assert ei.value.code == SVT_EINVAL, kw
    assert len(eng.call(merge_gap=0, merge_min=0)) == 2                    # merge_min is ignored without a gap
    assert len(eng.call(merge_gap=1 << 20, merge_min=50)) == 1
    assert len(eng.call(merge_gap=50)) == 1                                # merge_min defaults to 20
    with pytest.raises(SvtError) as ei:
        eng.call_consensus()
    assert ei.value.code == SVT_ESTATE and "merge" in str(ei.value)
    with Engine(Params(), device=0) as e0:
        with pytest.raises(SvtError) as ei:
            e0.call(merge_gap=50)
        assert ei.value.code == SVT_ESTATE


def cli_reads():
    reads = []
    for x, ops in ((100000, [(D, 180), (M, 5), (D, 120)]), (160000, [(D, 25), (M, 2), (D, 26)]),
                   (220000, [(I, 30), (M, 7), (I, 30), (M, 9), (I, 30)]), (280000, [(D, 400)])):
        for k in range(8):
            lead = 700 + 150 * k
            reads.append((0, x - lead, [(M, lead)] + ops + [(M, 2500 - 100 * k)]))
    return reads


@pytest.mark.parametrize("inflate", ["cpu", "gpu"])
def test_cli_merge_gap(tmp_path, inflate):
    reads = cli_reads()
    bam, vcf = str(tmp_path / "x.bam"), str(tmp_path / "c.vcf")
    write_bam(bam, reads)
    pl = from_reads(1, reads, clip={})
    want = R.call(pl, merge_gap=50)[0]
    assert [(int(c["pos"]), int(c["len"])) for c in want] == [(100000, 300), (160000, 51), (220000, 90), (280000, 400)]

    def run(*args):
        return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    p = run("call", "-b", bam, "-o", vcf, "--inflate", inflate, "--merge-gap", "50", "--verbose")
    assert p.returncode == 0 and p.stdout == "" and "calls 4" in p.stderr, p.stderr
    assert "merge-gap 50  merge-min 20  fragments 64  runs 32  joined items 24  items 32" in p.stderr, p.stderr
    with open(vcf) as f:
        assert f.read() == host.format_calls(want, ["1"])
    p = run("call", "-b", bam, "--inflate", inflate, "--merge-gap", "50", "--merge-min", "26", "--genotype")
    want26 = R.call(pl, merge_gap=50, merge_min=26)[0]
    assert len(want26) == 3
    assert p.returncode == 0 and p.stdout == host.format_calls(want26, ["1"], genotypes=R.genotype(pl, calls_to_sites(want26), 50, 26))
    p = run("call", "-b", bam, "--inflate", inflate)                      # without the flag: single ops
    assert p.returncode == 0 and p.stdout == host.format_calls(R.call(pl)[0], ["1"])
    p = run("call", "-b", bam, "--merge-gap", "50", "--ins-seq")
    assert p.returncode != 0 and "--merge-gap" in p.stderr and "--ins-seq" in p.stderr
    for flag, bad in (("--merge-gap", "1048577"), ("--merge-gap", "-1"), ("--merge-min", "0"), ("--merge-min", "51")):
        p = run("call", "-b", bam, "--merge-gap", "50", flag, bad)
        assert p.returncode == 1 and flag in p.stderr
