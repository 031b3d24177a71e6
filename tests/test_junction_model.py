"""tests/junction_ref.py, the model of include/svtrek_junction.h, pinned on hand-built reads whose answers
are written out here, then on a simulated pileup in which every second supporting read is cut into two
records: the union scan finds what the scan of the whole reads found."""
from dataclasses import replace

import numpy as np
import pytest

from svtrek_amd import from_reads, sim
from svtrek_amd._lib import JUNCTION_SEG_DTYPE, SVT_DEL, SVT_INS

import call_merge_ref
import call_ref
import junction_ref as J

M, I, D, N, S, H = 0, 1, 2, 3, 4, 5


def rows(*segs):
    return np.array(list(segs), dtype=JUNCTION_SEG_DTYPE).reshape(len(segs))


def plus(r_beg, r_end, q_beg, q_end, tid=0):
    return (tid, 0, r_beg, r_end, q_beg, q_end)


def minus(r_beg, r_end, q_beg, q_end, tid=0):
    return (tid, 1, r_beg, r_end, q_beg, q_end)


def test_segments_of_cigars_and_clips():
    # strand +: q_beg is the leading clip; strand -: the trailing one; H counts like S; D and N advance the reference
    assert J.seg_of(0, 0, 1000, "10S90M5I20D30M7S") == (0, 0, 1000, 1140, 10, 135)
    assert J.seg_of(0, 1, 1000, "10S90M5I20D30M7S") == (0, 1, 1000, 1140, 7, 132)
    assert J.seg_of(2, 0, 5, "3H4S10=2X6N1M9H") == (2, 0, 5, 24, 7, 20)
    assert J.seg_of(2, 1, 5, "3H4S10=2X6N1M9H") == (2, 1, 5, 24, 9, 22)
    assert J.seg_of(0, 0, 0, [(M, 5)]) == (0, 0, 0, 5, 0, 5)


@pytest.mark.parametrize("dr, dq, want", [
    (51, 0, (SVT_DEL, 51)), (50, 0, None),                       # d = 51 / 50
    (52, 1, (SVT_DEL, 51)), (51, 1, None),                       # the same with dq = 1
    (1, -50, (SVT_DEL, 51)), (0, -51, None),                     # dr = 1 / 0 (a query overlap: len = dr - dq)
    (0, 50, (SVT_INS, 50)), (0, 49, None),                       # -d = 50 / 49
    (-50, 1, (SVT_INS, 51)), (-51, 1, "other"),                  # dr = -50 / -51
    (-50, 0, None), (-60, 0, None),                              # dq = 0: no INS whatever -d
    (300, 40, (SVT_DEL, 260)),                                   # unaligned query bases inside a deletion
    (10, 400, (SVT_INS, 390)),
])
@pytest.mark.parametrize("strand", [0, 1])
def test_thresholds(dr, dq, want, strand):
    if strand == 0:   # A = left on the reference, B right
        A, B = plus(1000, 2000, 10, 1010), plus(2000 + dr, 3000 + dr, 1010 + dq, 2010 + dq)
        x = 2000
    else:             # A = the query-first segment is the RIGHT one on the reference
        A, B = minus(5000, 6000, 10, 1010), minus(4000 - dr, 5000 - dr, 1010 + dq, 2010 + dq)
        x = 5000 - dr
    j = J.junction(rows(A, B))
    if want is None:
        assert j == ("none",)
    elif want == "other":
        assert j == ("other",)
    else:
        assert j[:4] == (want[0], 0, x, want[1])
        assert j[4:] == ((1000, 3000 + dr) if strand == 0 else (4000 - dr, 6000))
    assert J.junction(rows(B, A)) is None   # the later segment's record has no junction to emit here


def test_chain_shuffled_sa_equal_tuples_and_other():
    a, b, c = plus(1000, 2000, 0, 1000), plus(2300, 3300, 1000, 2000), plus(3300, 4300, 2100, 3100)
    # three segments, two junctions, each emitted once: by its query-first record
    assert J.junction(rows(a, b, c))[:4] == (SVT_DEL, 0, 2000, 300)
    assert J.junction(rows(a, c, b))[:4] == (SVT_DEL, 0, 2000, 300)      # SA order does not matter
    assert J.junction(rows(b, a, c))[:4] == (SVT_INS, 0, 3300, 100)
    assert J.junction(rows(b, c, a))[:4] == (SVT_INS, 0, 3300, 100)
    assert J.junction(rows(c, a, b)) is None
    # equal tuples never pair: a twin of A is not greater than A
    assert J.junction(rows(a, a)) is None
    assert J.junction(rows(a, a, b))[:4] == (SVT_DEL, 0, 2000, 300)
    # ties between candidates go by (q_beg, q_end, tid, r_beg, strand)
    assert J.junction(rows(a, plus(2400, 3400, 1000, 2000), b))[:4] == (SVT_DEL, 0, 2000, 300)
    assert J.junction(rows(a, plus(2400, 3300, 1000, 1900), b))[:4] == (SVT_DEL, 0, 2000, 400)
    # another contig or strand: other
    assert J.junction(rows(a, plus(2300, 3300, 1000, 2000, tid=1))) == ("other",)
    assert J.junction(rows(a, minus(2300, 3300, 1000, 2000))) == ("other",)
    # ... even when a qualifying segment follows later in the query
    assert J.junction(rows(a, minus(2300, 3300, 1000, 2000), c)) == ("other",)


def test_clamps_and_stats():
    sat = 1 << 30
    seg = rows(plus(0, sat - 1, 0, 100), plus(sat + 99, sat + 199, 100, 200),           # x = 2^30 - 1: kept
               plus(0, sat, 0, 100), plus(sat + 100, sat + 200, 100, 200),              # x = 2^30: skipped
               plus(0, 10, 0, 10), plus((1 << 29) + 10, (1 << 29) + 20, 10, 20),        # len 2^29 -> 2^28 - 1
               plus(0, 10, 0, 10))                                                       # a record without a junction
    table = (np.array([0, 1, 2, 3], dtype=np.uint64), np.array([0, 2, 4, 6, 7], dtype=np.uint64), seg)
    it, st = J.items(None, table)
    x, ln, lo, hi = it[0][SVT_DEL]
    assert x.tolist() == [sat - 1, sat, 10] and ln.tolist() == [100, 100, (1 << 28) - 1]
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [sat + 199, sat + 200, (1 << 29) + 20]
    assert st == {"records": 4, "segments": 7, "junctions": 3, "del_items": 3, "ins_items": 0, "other": 0, "skipped": 1}


def test_cut_h_against_s_clips_both_strands():
    # one read with a hard clip in front and a soft clip behind, cut at its 300D and (another read) at its 80I
    reads = [(0, 1000, [(H, 7), (M, 500), (D, 300), (M, 400), (S, 9)]), (0, 1000, [(S, 5), (M, 500), (I, 80), (M, 400)])]
    for strand in (0, 1):
        pl = from_reads(1, reads, clip={})
        pl.flag = np.array([strand << 4] * 2, dtype=np.uint16)
        out, (read, off, seg), index = J.cut(pl, [(0, 2), (1, 2)])
        assert out.n_reads == 4 and index.tolist() == [-1, -1]
        assert [out.cigar_string(r) for r in range(4)] == ["7H500M409S", "5S500M480S", "585S400M", "507S400M9S"]
        it, st = J.items(out, (read, off, seg))
        assert st["junctions"] == 2 and st["del_items"] == 1 and st["ins_items"] == 1 and st["other"] == 0
        assert [a.tolist() for a in it[0][SVT_DEL]] == [[1500], [300], [1000], [2200]]
        assert [a.tolist() for a in it[0][SVT_INS]] == [[1500], [80], [1000], [1900]]
        # every record carries its own segment and its partner's
        assert len(read) == 4 and off.tolist() == [0, 2, 4, 6, 8]


def every_second(pl):
    """[(read, op index)] of every second supporting op of every (contig, type, start) in start order, at most
    one a read and only where both halves keep an aligned base (the simulator ends some reads in I S)."""
    which, taken = [], set()
    for tid in range(pl.n_targets):
        a = int(pl.tid_off[tid])
        op, ln, read_of, x = call_merge_ref.walk(pl, tid)
        first = pl.cig_off[a + read_of].astype(np.int64) - int(pl.cig_off[a])
        for sel in ((op == 2) & (ln > 50), (op == 1) & (ln >= 50)):
            idx = np.nonzero(sel)[0]
            idx = idx[np.argsort(x[idx], kind="stable")]
            for k in idx[1::2]:
                r = a + int(read_of[k])
                if r not in taken and J.cuttable(J.parse_cigar(pl.read_cigar(r)), int(k - first[k])):
                    taken.add(r)
                    which.append((r, int(k - first[k])))
    return which


@pytest.fixture(scope="module")
def cut_world():
    r = sim.generate(replace(sim.WORKLOADS["cfg4_1m_delins_30x_hifi"], n_loci=2000, n_targets=2))
    # The walk of svtrek_call.h advances x over H ops (the reference's quirk), a segment's r_end does not: a read
    # with a leading hard clip files its CIGAR items that much to the right of the junction its halves give.
    # The comparison below is about the cut, so the simulated hard clips are written as soft clips first.
    pl = replace(r.pileup, cigar=np.where((r.pileup.cigar & 15) == H, (r.pileup.cigar & ~np.uint32(15)) | np.uint32(S),
                                          r.pileup.cigar).astype(np.uint32))
    which = every_second(pl)
    return pl, which, J.cut(pl, which)


def test_cut_reads_are_called_like_whole_ones(cut_world):
    pl, which, (out, table, index) = cut_world
    assert len(which) > 5000 and out.n_reads == pl.n_reads + len(which)
    want, wst = call_ref.call(pl)
    got, st, sp, mg, jst = J.call(out, table)
    assert jst["junctions"] == len(which) == jst["del_items"] + jst["ins_items"] and jst["other"] == 0
    assert jst["records"] == 2 * len(which) and jst["segments"] == 4 * len(which)
    assert {k: st[k] for k in wst} == wst
    fields = [f for f in want.dtype.names if f != "depth"]
    assert len(got) == len(want) > 1500
    for f in fields:
        assert np.array_equal(got[f], want[f]), f
    # depth by the model's own definition: the records of the cut pileup covering pos (the halves of a cut
    # read end / begin at the site and no longer cover it)
    for c in got[:: max(len(got) // 200, 1)]:
        r0, r1 = int(out.tid_off[c["chrom"] - 1]), int(out.tid_off[c["chrom"]])
        p = int(c["pos"])
        assert int(c["depth"]) == int(((out.pos[r0:r1] <= p) & (out.endpos[r0:r1] > p)).sum())
    assert (got["depth"] <= want["depth"]).all() and (got["depth"] < want["depth"]).any()


def test_the_plain_model_loses_the_cut_reads(cut_world):
    pl, which, (out, table, index) = cut_world
    want, _ = call_ref.call(pl, min_support=1)
    plain, _ = call_ref.call(out, min_support=1)
    assert int(plain["support"].sum()) == int(want["support"].sum()) - len(which)
    full, *_ = J.call(out, table, min_support=1)
    assert int(full["support"].sum()) == int(want["support"].sum())


def test_genotype_counts_split_reads_as_alt_not_ref():
    # 4 whole reference reads, 2 reads with the 300D in the CIGAR, 2 cut at it
    reads = [(0, 1000, [(M, 3000)])] * 4 + [(0, 1000, [(M, 1000), (D, 300), (M, 1700)])] * 4
    pl = from_reads(1, reads, clip={})
    out, table, _ = J.cut(pl, [(6, 1), (7, 1)])
    calls, st, *_ = J.call(out, table)
    assert [(int(c["pos"]), int(c["len"]), int(c["support"])) for c in calls] == [(2000, 300, 4)]
    g = J.genotype(out, table, calls)[0]
    assert (int(g["alt"]), int(g["ref"]), int(g["span"]), int(g["alt_all"]), int(g["gt"])) == (4, 4, 6, 4, 1)
