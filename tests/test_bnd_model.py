"""tests/bnd_ref.py, the model of include/svtrek_bnd.h, pinned on hand-built segment rows whose answers are
written out here (the four orientations from both read strands, the canonical swap, the clamps, classes,
groups, min_support, the order), then by a simulation that does not use the header's formulas: sample
chromosomes joining three reference contigs are written as piecewise sample -> reference maps, reads are cut
from both strands of the SAMPLE across every breakpoint, their alignments follow from the map alone, and the
model has to call exactly the breakpoints' items with every crossing read as support."""
import numpy as np
import pytest

from svtrek_amd import from_reads
from svtrek_amd._lib import JUNCTION_SEG_DTYPE, SVT_BND, SVT_DEL, SVT_DUP, SVT_INS, SVT_INV, call_mate

import bnd_ref as B
import junction_ref as J

M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
SAT = 1 << 30


def rows(*segs):
    return np.array(list(segs), dtype=JUNCTION_SEG_DTYPE).reshape(len(segs))


def seg(tid, strand, r_beg, r_end, q_beg, q_end):
    return (tid, strand, r_beg, r_end, q_beg, q_end)


def table_of(records):
    """(read, off, seg) of a list of row arrays, read k = k."""
    off = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
    return (np.arange(len(records), dtype=np.uint64), off,
            np.concatenate(records) if records else np.zeros(0, dtype=JUNCTION_SEG_DTYPE))


# The junction "contig 1 at 2000 | contig 5 at 7000" in each orientation, as the read of the forward sample strand
# sees it (A then B) and as the read of the other strand does (B mirrored, then A mirrored).
#   o = 1: left of 2000 joined to right of 7000;  o = 0: left | left;  o = 3: right | right;  o = 2: right | left
FWD = {1: (seg(1, 0, 1000, 2000, 0, 1000), seg(5, 0, 7000, 8000, 1000, 2000)),
       0: (seg(1, 0, 1000, 2000, 0, 1000), seg(5, 1, 6000, 7000, 1000, 2000)),
       3: (seg(1, 1, 2000, 3000, 0, 1000), seg(5, 0, 7000, 8000, 1000, 2000)),
       2: (seg(1, 1, 2000, 3000, 0, 1000), seg(5, 1, 6000, 7000, 1000, 2000))}


def mirrored(A, Bs):
    """The same two alignments as the read of the other strand has them: strands flipped, query order swapped."""
    flip = lambda s, q0: (s[0], 1 - s[1], s[2], s[3], q0, q0 + (s[5] - s[4]))   # noqa: E731
    return flip(Bs, 0), flip(A, Bs[5] - Bs[4])


@pytest.mark.parametrize("o", [0, 1, 2, 3])
def test_four_orientations_each_from_both_read_strands(o):
    A, Bs = FWD[o]
    want = (1, 2000, 5, 7000, o)
    assert B.breakend(rows(A, Bs)) == want
    A2, B2 = mirrored(A, Bs)
    assert A2[0] == 5 and B.breakend(rows(A2, B2)) == want          # A.tid > B.tid: the breakends swap


def test_a_tid_above_b_tid_swaps_the_breakends():
    # A on contig 4 strand + ends at 900 (left of 900 in the read); B on contig 2 strand + starts at 300 (right of it)
    assert B.breakend(rows(seg(4, 0, 100, 900, 0, 800), seg(2, 0, 300, 700, 800, 1200))) == (2, 300, 4, 900, 2 * 1 + 0)


def test_no_item_without_another_contig_a_b_or_a_later_tuple():
    A = seg(0, 0, 1000, 2000, 0, 1000)
    assert B.breakend(rows(A)) is None
    assert B.breakend(rows(A, A)) is None                                          # equal tuples never pair
    assert B.breakend(rows(A, seg(0, 1, 5000, 6000, 1000, 2000))) is None            # B.tid == A.tid
    assert B.breakend(rows(seg(0, 0, 1000, 2000, 500, 1500), seg(3, 0, 10, 510, 0, 500))) is None   # query-earlier: no B
    far, near, same = seg(2, 1, 9000, 9500, 3000, 3500), seg(1, 0, 5000, 6000, 1000, 2000), seg(0, 0, 2300, 2800, 1000, 1500)
    want = (0, 2000, 1, 5000, 1)
    assert B.breakend(rows(A, far, near)) == B.breakend(rows(A, near, far)) == want   # shuffled SA order
    assert B.breakend(rows(A, near, same, far)) is None      # (1000, 1500, tid 0) < (1000, 2000, tid 1): B is on A's contig


def test_x_and_y_at_the_clamp():
    recs = [rows(seg(0, 0, x - 100, x, 0, 100), seg(1, 0, y, y + 100, 100, 200))
            for x, y in ((SAT - 1, 500), (SAT, 500), (700, SAT - 1), (700, SAT), (SAT + 9, SAT + 9))]
    kept, st = B.items(table_of(recs))
    assert kept == [(0, SAT - 1, 1, 500, 1), (0, 700, 1, SAT - 1, 1)] and st == {"items": 5, "skipped": 3}


def world(n_targets, reads, sa, flags=None):
    assert [(t, p) for t, p, _ in reads] == sorted((t, p) for t, p, _ in reads)
    pl = from_reads(n_targets, reads, clip={})
    pl.flag = np.array(flags if flags is not None else [0] * len(reads), dtype=np.uint16)
    return pl, J.segments(pl, sa)


def bnd(x, y, tid=0, mate=1, o=1, q=1000):
    """One record whose item is (tid, x, mate, y, o), tid < mate: (read, its SA entry, flag).  The own segment is
    on tid: strand + ending at x for o in (0, 1), strand - beginning at x for o in (2, 3); B is on mate: strand +
    beginning at y for o in (1, 3), strand - ending at y for o in (0, 2)."""
    own_minus, b_minus = o >= 2, (o & 1) == 0
    own = (tid, x, [(S, q), (M, 500)]) if own_minus else (tid, x - 500, [(M, 500), (S, q)])
    b = (mate, y - 500 + 1, "-", [(M, 500), (S, 500)]) if b_minus else (mate, y + 1, "+", [(S, 500), (M, 500)])
    return own, b, 16 if own_minus else 0


def build(specs, n_targets):
    order = sorted(range(len(specs)), key=lambda i: (specs[i][0][0], specs[i][0][1]))
    reads = [specs[i][0] for i in order]
    sa = {k: [specs[i][1]] for k, i in enumerate(order) if specs[i][1] is not None}
    return world(n_targets, reads, sa, flags=[specs[i][2] for i in order])


def recs(calls):
    mc, o = call_mate(calls)
    return [(int(c["chrom"]), int(c["pos"]), int(mc[i]), int(c["end"]), int(o[i]), int(c["support"])) for i, c in enumerate(calls)]


def test_the_helper_builds_what_it_says():
    for o in range(4):
        pl, table = build([bnd(2000, 7000, o=o)], 2)
        assert B.items(table)[0] == [(0, 2000, 1, 7000, o)]


def test_classes_groups_and_min_support():
    specs = [bnd(2000, 7000)] * 3 + [bnd(2000, 7000, mate=2)] * 3 + [bnd(2000, 7000, o=0)] * 3     # same x: three classes
    specs += [bnd(30000 + k, 9000) for k in (0, 1, 2)] + [bnd(30000 + k, 9011 + k) for k in (3, 4, 5)]   # y in two runs
    specs += [bnd(50000 + 10 * k, 4000 + 10 * k) for k in range(6)]                                # a chain, each link apart
    specs += [bnd(70000, 100)] * 3 + [bnd(70001, 200)] * 2                                         # 3 + 2: one call
    pl, table = build(specs, 3)
    calls, st, *_, bst = B.call(pl, table, types=())
    assert (calls["type"] == SVT_BND).all() and not calls["len"].any()
    assert recs(calls) == [(1, 2000, 2, 7000, 0, 3), (1, 2000, 2, 7000, 1, 3), (1, 2000, 3, 7000, 1, 3),
                           (1, 30001, 2, 9000, 1, 3), (1, 30004, 2, 9015, 1, 3), (1, 50025, 2, 4025, 1, 6), (1, 70000, 2, 100, 1, 3)]
    assert bst == {"items": 26, "skipped": 0, "classes": 3, "clusters": 6, "groups": 8, "calls": 7}
    assert {k: st[k] for k in ("events", "skipped", "clusters", "calls")} == {"events": 26, "skipped": 0, "clusters": 6, "calls": 7}
    c = calls[5]
    assert (int(c["x_lo"]), int(c["x_hi"]), int(c["len_lo"]), int(c["len_hi"])) == (50000, 50050, 4000, 4050)
    assert int(c["depth"]) == 3 and int(calls[0]["depth"]) == 0    # (an own segment [x - 500, x) does not cover its x)
    assert len(B.call(pl, table, types=(), link=9)[0]) == 6        # the chain falls apart into six groups of one
    assert recs(B.call(pl, table, types=(), min_support=2)[0])[-2:] == [(1, 70000, 2, 100, 1, 3), (1, 70001, 2, 200, 1, 2)]


def test_tie_order_of_bnd_calls_and_of_all_five_types():
    specs = []
    for _ in range(3):                                     # CIGAR: 300D and 80I at x = 2000
        specs += [((0, 1000, [(M, 1000), (D, 300), (M, 700)]), None, 0), ((0, 1000, [(M, 1000), (I, 80), (M, 700)]), None, 0)]
    for _ in range(3):                                     # DUP [2000, 2400) and INV [2000, 2600)
        specs += [((0, 1000, [(M, 1400), (S, 500)]), (0, 2000 + 1, "+", [(S, 1400), (M, 500)]), 0)]
        specs += [((0, 1000, [(M, 1000), (S, 500)]), (0, 2100 + 1, "-", [(M, 500), (S, 1000)]), 0)]
    # BND calls at (chrom 1, 2000): mate 3 before ...; mate 2 with o 0 before o 1; o 1 with end 600 before end 9000
    specs += [bnd(2000, 500, mate=2)] * 3 + [bnd(2000, 9000, mate=1)] * 3 + [bnd(2000, 600, mate=1)] * 3 + [bnd(2000, 9000, mate=1, o=0)] * 3
    pl, table = build(specs, 3)
    calls = B.call(pl, table, rearrangements=(SVT_DUP, SVT_INV))[0]
    assert [int(t) for t in calls["type"]] == [SVT_INS, SVT_DEL, SVT_INV, SVT_DUP] + [SVT_BND] * 4
    assert (calls["pos"] == 2000).all() and (calls["chrom"] == 1).all()
    assert recs(calls[4:]) == [(1, 2000, 2, 9000, 0, 3), (1, 2000, 2, 600, 1, 3), (1, 2000, 2, 9000, 1, 3), (1, 2000, 3, 500, 1, 3)]
    # the BND calls change nothing else: the same scan without them is the list's head, stats apart
    base = B.call(pl, table, rearrangements=(SVT_DUP, SVT_INV), breakends=False)
    assert np.array_equal(base[0], calls[:4]) and base[6] == B.BND_ZERO
    g = B.genotype(pl, table, calls)
    assert (g["gt"][4:] == -1).all() and not g["alt"][4:].any() and not g["span"][4:].any() and (g["gt"][:2] >= 0).all()


# ---- the simulation: sample chromosomes as piecewise maps onto three reference contigs -------------------
def alignments(pcs, u, v, rstrand):
    """The alignments of the read that is sample[u, v) (rstrand 1: its reverse complement), from the map alone:
    [(tid, strand, r_beg, r_end, q_beg, q_end)], query coordinates in the read's own orientation."""
    out = []
    for sb, se, tid, r0, r1, rev in pcs:
        a, b = max(u, sb), min(v, se)
        if a >= b:
            continue
        r_beg, r_end = (r1 - (b - sb), r1 - (a - sb)) if rev else (r0 + (a - sb), r0 + (b - sb))
        q_beg, q_end = (v - b, v - a) if rstrand else (a - u, b - u)
        out.append((tid, rstrand ^ rev, r_beg, r_end, q_beg, q_end))
    return out


def chromosome(*parts):
    """[(sample_beg, sample_end, tid, ref_beg, ref_end, reversed)] of (tid, ref_beg, ref_end, reversed) parts."""
    out, at = [], 0
    for tid, r0, r1, rev in parts:
        out.append((at, at + (r1 - r0), tid, r0, r1, rev))
        at += r1 - r0
    return out


def records_of(reads, n_targets):
    """One pileup record per alignment of (pieces, u, v, rstrand) reads, soft-clipped to the read's length in
    REFERENCE orientation, every record's SA entries the read's other alignments."""
    recs_, by_read = [], {}
    for rid, (pcs, u, v, rstrand) in enumerate(reads):
        n = v - u
        by_read[rid] = []
        for k, (tid, st, r_beg, r_end, q_beg, q_end) in enumerate(alignments(pcs, u, v, rstrand)):
            lead, trail = (n - q_end, q_beg) if st else (q_beg, n - q_end)
            cig = [(S, lead)] * (lead > 0) + [(M, r_end - r_beg)] + [(S, trail)] * (trail > 0)
            by_read[rid].append((tid, r_beg, "-" if st else "+", cig))
            recs_.append((tid, r_beg, cig, 16 if st else 0, rid, k))
    order = sorted(range(len(recs_)), key=lambda i: recs_[i][:2])
    sa = {}
    for new, i in enumerate(order):
        rid, k = recs_[i][4:]
        others = [(tid, r_beg + 1, st, cig) for j, (tid, r_beg, st, cig) in enumerate(by_read[rid]) if j != k]
        if others:
            sa[new] = others
    return world(n_targets, [recs_[i][:3] for i in order], sa, [recs_[i][3] for i in order])


@pytest.mark.parametrize("seed", [1, 2])
def test_simulated_translocations(seed):
    rng = np.random.default_rng(seed)
    L = 60000
    # a reciprocal translocation between contig 0 at 20000 and contig 1 at 31000 ...
    s1 = chromosome((0, 0, 20000, 0), (1, 31000, L, 0))
    s2 = chromosome((1, 0, 31000, 0), (0, 20000, L, 0))
    # ... and an inverted one: contig 2 up to 12000 joined to contig 1 read DOWNWARDS from 45000, and its reciprocal,
    # contig 1 read downwards to 45000 joined to contig 2 from 12000 on
    s3 = chromosome((2, 0, 12000, 0), (1, 40000, 45000, 1))
    s4 = chromosome((1, 45000, 50000, 1), (2, 12000, L, 0))
    # what each breakpoint is, by what of the reference lies on which side of it in the sample:
    #   s1: left of 0:20000 | right of 1:31000;   s2: left of 1:31000 | right of 0:20000
    #   s3: left of 2:12000 | left of 1:45000;    s4: right of 1:45000 | right of 2:12000
    want = {"s1": (0, 20000, 1, 31000, 1), "s2": (0, 20000, 1, 31000, 2), "s3": (1, 45000, 2, 12000, 0), "s4": (1, 45000, 2, 12000, 3)}
    chroms = {"s1": s1, "s2": s2, "s3": s3, "s4": s4}
    reads, crossing = [], {}
    for name, pcs in chroms.items():
        bp = pcs[0][1]
        crossing[name] = 0
        for rstrand in (0, 1):
            for _ in range(int(rng.integers(3, 7))):
                a, b = (int(x) for x in rng.integers(300, 900, size=2))
                reads.append((pcs, bp - a, bp + b, rstrand))
                crossing[name] += 1
        for _ in range(5):   # reads that cross nothing, on both strands, in the reversed pieces too
            u = int(rng.integers(0, pcs[-1][1] - 1000))
            if not (u - 5 < bp < u + 805):
                reads.append((pcs, u, u + 800, int(rng.integers(0, 2))))
    pl, table = records_of(reads, 3)
    n_cross = sum(crossing.values())
    assert len(table[0]) == 2 * n_cross and pl.n_reads == len(reads) + n_cross
    kept, n = B.items(table)
    assert n == {"items": n_cross, "skipped": 0}
    assert sorted(set(kept)) == sorted(want.values())
    for name, it in want.items():
        assert kept.count(it) == crossing[name]
    calls, st, sp, mg, jst, rst, bst = B.call(pl, table, min_support=1, junctions=True, rearrangements=(SVT_DUP, SVT_INV))
    assert (calls["type"] == SVT_BND).all()                 # no DEL / INS / DUP / INV anywhere
    got = sorted(recs(calls))
    assert got == sorted((t + 1, x, m + 1, y, o, crossing[name]) for name, (t, x, m, y, o) in want.items())
    assert all(int(c["x_lo"]) == int(c["x_hi"]) == int(c["pos"]) and int(c["len_lo"]) == int(c["len_hi"]) == int(c["end"]) for c in calls)
    assert bst == {"items": n_cross, "skipped": 0, "classes": 4, "clusters": 4, "groups": 4, "calls": 4}
    assert jst["other"] == n_cross and jst["junctions"] == n_cross and rst["dup_items"] == 0 and rst["inv_items"] == 0
    assert [int(c["chrom"]) for c in calls] == [1, 1, 2, 2] and [int(o) for o in call_mate(calls)[1]] == [1, 2, 0, 3]
