"""svt_call_params.merge_gap / merge_min on the CPU: the numpy model (tests/call_merge_ref.py) on
hand-built reads with the answers written out, and its defining property on simulated pileups -- a
pileup whose D > 50 / I >= 50 ops are cut into pieces (call_merge_ref.fragment) gives, merged, exactly
the calls of the whole pileup, which the plain model on the pieces does not."""
import functools
from dataclasses import replace

import numpy as np

from svtrek_amd import from_reads, sim
from svtrek_amd._lib import SVT_DEL, SVT_INS

import call_merge_ref as R
import call_ref

M, I, D, N, S, H, P = 0, 1, 2, 3, 4, 5, 6


def items(reads, gap=50, m=20, n_targets=1, tid=0):
    """[(x, len), ...] per type of hand-built reads, in read order."""
    it = R.merged_items(from_reads(n_targets, reads, clip={}), tid, gap, m)
    return {ty: [(int(x), int(ln)) for x, ln in zip(it[ty][0], it[ty][1])] for ty in (SVT_DEL, SVT_INS)}


def test_the_issues_example_and_the_thresholds():
    assert items([(0, 100, [(M, 900), (D, 180), (M, 5), (D, 120), (M, 50)])]) == {SVT_DEL: [(1000, 300)], SVT_INS: []}
    assert items([(0, 100, [(M, 900), (D, 40), (M, 3), (D, 40), (M, 50)])])[SVT_DEL] == [(1000, 80)]
    assert items([(0, 100, [(M, 900), (D, 30), (M, 3), (D, 30), (M, 50)])])[SVT_DEL] == [(1000, 60)]
    assert items([(0, 100, [(M, 900), (D, 25), (M, 2), (D, 25), (M, 50)])])[SVT_DEL] == []          # sum 50: no DEL
    assert items([(0, 100, [(M, 900), (I, 25), (M, 2), (I, 25), (M, 50)])])[SVT_INS] == [(1000, 50)]  # sum 50: an INS
    assert items([(0, 100, [(M, 900), (I, 25), (M, 2), (I, 24), (M, 50)])])[SVT_INS] == []


def test_distance_from_the_tail_for_del_and_from_x_for_ins():
    for g, n in ((50, 1), (51, 2)):
        got = items([(0, 0, [(M, 100), (D, 60), (M, g), (D, 70), (M, 9)])])[SVT_DEL]
        assert got == ([(100, 130)] if n == 1 else [(100, 60), (160 + g, 70)])
        got = items([(0, 0, [(M, 100), (I, 60), (M, g), (I, 70), (M, 9)])])[SVT_INS]
        assert got == ([(100, 130)] if n == 1 else [(100, 60), (100 + g, 70)])


def test_fragment_of_m_and_of_m_minus_1():
    assert items([(0, 0, [(M, 100), (D, 40), (M, 5), (D, 20), (M, 9)])])[SVT_DEL] == [(100, 60)]
    assert items([(0, 0, [(M, 100), (D, 40), (M, 5), (D, 19), (M, 9)])])[SVT_DEL] == []
    # a 19D is no fragment: it only adds 19 to the distance between its neighbours
    assert items([(0, 0, [(M, 100), (D, 40), (M, 20), (D, 19), (M, 11), (D, 40), (M, 9)])])[SVT_DEL] == [(100, 80)]
    assert items([(0, 0, [(M, 100), (D, 40), (M, 20), (D, 19), (M, 12), (D, 40), (M, 9)])])[SVT_DEL] == []
    assert items([(0, 0, [(M, 100), (D, 40), (M, 5), (D, 19), (M, 9)])], m=19)[SVT_DEL] == [(100, 59)]


def test_single_linkage_and_types_apart():
    # three fragments, each 40 past the one before at G = 50: one run although the span is past G
    assert items([(0, 0, [(M, 100), (D, 30), (M, 40), (D, 30), (M, 40), (D, 30), (M, 9)])])[SVT_DEL] == [(100, 90)]
    got = items([(0, 0, [(M, 100), (D, 40), (M, 2), (I, 40), (M, 2), (D, 40), (M, 2), (I, 40), (M, 9)])])
    assert got == {SVT_DEL: [(100, 80)], SVT_INS: [(142, 80)]}
    # N, H, P and a code 9-15 between two fragments count in the distance; S and I do not
    for op, joined in ((N, False), (H, False), (P, False), (11, False), (S, True), (I, True)):
        got = items([(0, 0, [(M, 100), (D, 40), (M, 30), (op, 21), (D, 40), (M, 9)])], m=22)[SVT_DEL]
        assert (got == [(100, 80)]) == joined, op


def test_clamps_and_reads_apart():
    big = (1 << 28) - 1
    lead = [(N, big)] * 3 + [(N, (1 << 30) - 3 * big - 110)]                      # x = 2^30 - 100 after it (pos 10)
    got = items([(0, 10, lead + [(D, 40), (M, 80), (D, 40), (M, 5)])], gap=100)[SVT_DEL]
    assert got == [((1 << 30) - 100, 80)]                                         # the second fragment lies past 2^30: kept
    got = items([(0, 10, lead + [(M, 100), (D, 40), (M, 8), (D, 40), (M, 5)])])[SVT_DEL]
    assert got == [(1 << 30, 80)]                                                 # x clamped (the scan skips and counts it)
    got = items([(0, 10, lead + [(M, 160), (D, 40), (M, 8), (D, 40), (M, 5)])])[SVT_DEL]
    assert got == [(1 << 30, 80)]                                                 # (the walk itself is not saturated: they join)
    got = items([(0, 0, [(M, 5), (D, big), (M, 1), (D, big), (M, 1)])])[SVT_DEL]
    assert got == [(5, big)]                                                      # L clamped to 2^28 - 1
    # the last fragment of one read and the first of the next never join
    reads = [(0, 0, [(M, 100), (D, 30)]), (0, 0, [(D, 30), (M, 100)])]
    pl = from_reads(1, reads, clip={})
    assert items(reads)[SVT_DEL] == [] and R.merge_stats(pl, 50, 20) == {"fragments": 2, "runs": 2, "joined_items": 0, "items": 0}


def test_call_on_merged_items():
    reads = [(0, 100, [(M, 900), (D, 180), (M, 5), (D, 120), (M, 1000)])] * 4
    pl = from_reads(1, reads, clip={})
    calls, st, sp, ms = R.call(pl, merge_gap=50)
    # end = the mean of x + len + 1 with the summed len: 1301, five short of the last fragment's end + 1
    assert [tuple(int(v) for v in c) for c in calls] == [(SVT_DEL, 1, 1000, 1301, 4, 4, 300, 300, 300, 1000, 1000, 0)]
    assert st == {"events": 4, "skipped": 0, "clusters": 1, "calls": 1}
    assert ms == {"fragments": 8, "runs": 4, "joined_items": 4, "items": 4}
    plain, st0, _, ms0 = R.call(pl)
    assert [(int(c["pos"]), int(c["len"])) for c in plain] == [(1000, 180), (1185, 120)] and ms0 == R.MERGE_ZERO
    # with the split: four fragmented reads of 300 and four whole reads of 500 at one start
    reads += [(0, 100, [(M, 900), (D, 500), (M, 1000)])] * 4
    pl = from_reads(1, reads, clip={})
    calls = R.call(pl, len_permille=100, merge_gap=50)[0]
    assert [(int(c["pos"]), int(c["len"]), int(c["support"])) for c in calls] == [(1000, 300, 4), (1000, 500, 4)]
    gt = R.genotype(pl, calls, 50)
    assert np.array_equal(gt["alt_all"], calls["support"])


def same_items(a, b, n_targets, gap, m):
    for tid in range(n_targets):
        ia, ib = R.merged_items(a, tid, gap, m), R.merged_items(b, tid, gap, m)
        for ty in (SVT_DEL, SVT_INS):
            for u, v in zip(ia[ty], ib[ty]):
                assert np.array_equal(u, v)


@functools.lru_cache(maxsize=None)
def hifi_case():
    pl = sim.generate(replace(sim.WORKLOADS["cfg4_1m_delins_30x_hifi"], n_loci=2000, n_targets=2)).pileup
    return pl, R.fragment(pl, np.random.default_rng(31), 50, 20)


def test_fragmented_hifi_pileup_merges_back():
    pl, (fr, eligible, cut) = hifi_case()
    print(f"cfg4 n_loci=2000: {cut} of {eligible} ops fragmented, {pl.n_ops} -> {fr.n_ops} ops")
    assert cut >= 0.9 * eligible and eligible == 35391
    # in the whole pileup no two fragments join: its merged items are the plain items
    ms = R.merge_stats(pl, 50, 20)
    assert ms["runs"] == ms["fragments"] == 35840 and ms["joined_items"] == 0
    for tid in range(2):
        plain, merged = call_ref.items(pl, tid), R.merged_items(pl, tid, 50, 20)
        for ty in (SVT_DEL, SVT_INS):
            assert np.array_equal(plain[ty][0], merged[ty][0]) and np.array_equal(plain[ty][1], merged[ty][1])
    same_items(fr, pl, 2, 50, 20)
    want, wst = call_ref.call(pl)
    got, st, _, fms = R.call(fr, merge_gap=50, merge_min=20)
    assert np.array_equal(got, want) and st == wst               # record for record, depth included
    assert fms["items"] == ms["items"] and fms["joined_items"] == cut and fms["runs"] == ms["runs"]
    plain = call_ref.call(fr)[0]
    assert not (len(plain) == len(want) and np.array_equal(plain, want))
    assert fms["fragments"] >= ms["fragments"] + cut


@functools.lru_cache(maxsize=None)
def ont_case():
    pl = sim.generate(replace(sim.WORKLOADS["cfg3_50k_delins_30x_ont"], n_loci=200)).pileup
    return pl, R.fragment(pl, np.random.default_rng(32), 50, 20), R.fragment(pl, np.random.default_rng(33), 100, 20)


def test_fragmented_ont_pileup_merges_back():
    pl, (fr, eligible, cut), (fr100, eligible100, cut100) = ont_case()
    print(f"cfg3 n_loci=200: {cut} of {eligible} ops fragmented at G = 50, {cut100} of {eligible100} at G = 100")
    assert cut >= 0.2 * eligible and eligible > 1000
    nt = pl.n_targets
    same_items(fr, pl, nt, 50, 20)
    got = R.call(fr, merge_gap=50)
    want = R.call(pl, merge_gap=50)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    plain = call_ref.call(fr)[0]
    assert not (len(plain) == len(want[0]) and np.array_equal(plain, want[0]))
    # G = 100: the pileup has genuine joins of its own, so merged == merged (not merged == plain)
    assert cut100 > 0
    same_items(fr100, pl, nt, 100, 20)
    assert R.merge_stats(pl, 100, 20)["joined_items"] > 0
    assert np.array_equal(R.call(fr100, merge_gap=100)[0], R.call(pl, merge_gap=100)[0])
