"""tests/rearr_ref.py, the model of include/svtrek_rearr.h, pinned on hand-built segment rows whose answers
are written out here (every threshold on both strands, both clamps), then by a simulation that does not use
the header's formulas: a sample genome with an inversion and a tandem duplication is written as a piecewise
sample -> reference map, reads are cut from both strands of the SAMPLE across every breakpoint, their
alignments follow from the map alone, and the model has to call exactly the two variants."""
import numpy as np
import pytest

from svtrek_amd import from_reads
from svtrek_amd._lib import JUNCTION_SEG_DTYPE, SVT_DEL, SVT_DUP, SVT_INS, SVT_INV

import junction_ref as J
import rearr_ref as R

M, I, D, N, S, H = 0, 1, 2, 3, 4, 5


def rows(*segs):
    return np.array(list(segs), dtype=JUNCTION_SEG_DTYPE).reshape(len(segs))


def seg(strand, r_beg, r_end, q_beg, q_end, tid=0):
    return (tid, strand, r_beg, r_end, q_beg, q_end)


def dup_rows(strand, dr, dq):
    """A and B of one strand with the given dr and dq; the item's x is 2000 + dr on either strand."""
    if strand == 0:   # A = left on the reference: [1000, 2000), B starts at 2000 + dr
        return rows(seg(0, 1000, 2000, 10, 1010), seg(0, 2000 + dr, 3000 + dr, 1010 + dq, 2010 + dq))
    # the query-first segment is the RIGHT one on the reference: Rt = A = [2000 + dr, ...), Lf = B ends at 2000
    return rows(seg(1, 2000 + dr, 3000 + dr, 10, 1010), seg(1, 1000, 2000, 1010 + dq, 2010 + dq))


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("dr, dq, want", [
    (-50, -1, None), (-50, 0, None),          # dr = -50: -d = 49 / 50
    (-51, -2, None), (-51, -1, 51),           # dr = -51: -d = 49 / 50
    (-51, 5, 51),                             # dq > 0: the overlap junction_ref counts in other
    (-300, 20, 300), (-300, 0, 300), (-300, -100, 300),   # dq positive, zero, negative
    (-300, -250, 300), (-300, -251, None),    # -d = 50 / 49 far from dr's threshold
    (-40, 100, None), (300, 0, None),         # an insertion's small overlap; a deletion
])
def test_dup_thresholds(strand, dr, dq, want):
    j = R.rearrangement(dup_rows(strand, dr, dq))
    assert j == (None if want is None else (SVT_DUP, 0, 2000 + dr, want))


@pytest.mark.parametrize("a_strand", [0, 1])
@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("w, item", [(50, False), (51, True), (0, False), (4000, True)])
def test_inv_thresholds(a_strand, sign, w, item):
    """p = 20000 at A's query-last base, q = p + sign * w at B's query-first base."""
    p, q = 20000, 20000 + sign * w
    A = seg(0, p - 1000, p, 0, 1000) if a_strand == 0 else seg(1, p, p + 1000, 0, 1000)
    B = seg(1, q - 1000, q, 1000, 2000) if a_strand == 0 else seg(0, q, q + 1000, 1000, 2000)
    j = R.rearrangement(rows(A, B))
    assert j == ((SVT_INV, 0, min(p, q), w) if item else None)


def test_other_contig_no_b_and_equal_tuples():
    A = seg(0, 1000, 2000, 0, 1000)
    assert R.rearrangement(rows(A)) is None
    assert R.rearrangement(rows(A, A)) is None                                        # an equal tuple never pairs
    assert R.rearrangement(rows(A, seg(1, 5000, 6000, 1000, 2000, tid=1))) is None    # another contig: out of scope
    assert R.rearrangement(rows(seg(0, 1000, 2000, 500, 1500), seg(1, 5000, 6000, 0, 500))) is None   # B is query-earlier
    # the smallest later tuple is B, whatever the order of the rows
    far, near = seg(1, 9000, 9500, 3000, 3500), seg(1, 5000, 6000, 1000, 2000)
    assert R.rearrangement(rows(A, far, near)) == R.rearrangement(rows(A, near, far)) == (SVT_INV, 0, 2000, 4000)


def world(n_targets, reads, sa, flags):
    assert [(t, p) for t, p, _ in reads] == sorted((t, p) for t, p, _ in reads)
    pl = from_reads(n_targets, reads, clip={})
    pl.flag = np.array(flags, dtype=np.uint16)
    return pl, J.segments(pl, sa)


def test_len_clamp_and_the_junction_stats():
    big = (1 << 28) - 1
    reads, sa, flags = [], {}, []
    for _ in range(3):   # an inversion of 2^28 + 5: len clamped
        sa[len(reads)] = [(0, 1100 + big + 6 - 500 + 1, "-", [(M, 500), (S, 100)])]
        reads.append((0, 1000, [(M, 100), (S, 500)]))
        flags.append(0)
    pl, table = world(1, reads, sa, flags)
    it, n = R.items(table)
    assert n == {"dup_items": 0, "inv_items": 3} and it[0][SVT_INV][0].tolist() == [1100] * 3 and it[0][SVT_INV][1].tolist() == [big] * 3
    calls, st, sp, mg, jst, rst = R.call(pl, table, junctions=True)
    assert [(int(c["type"]), int(c["pos"]), int(c["end"]), int(c["len"]), int(c["support"])) for c in calls] == [(SVT_INV, 1100, 1100 + big, big, 3)]
    assert jst == J.items(pl, table)[1] and jst["other"] == 3 and jst["junctions"] == 3


def test_x_clamp():
    sat = 1 << 30
    table_rows, read, off = [], [], [0]
    for k, x in enumerate((sat - 1, sat, sat + 7)):   # strand +: B.r_beg = x, A ends 300 past it
        table_rows += [seg(0, x + 200, x + 300, 0, 100), seg(0, x, x + 100, 100, 200)]
        read.append(k)
        off.append(len(table_rows))
    table = (np.array(read, dtype=np.uint64), np.array(off, dtype=np.uint64), rows(*table_rows))
    it, n = R.items(table)
    assert n == {"dup_items": 3, "inv_items": 0}
    assert it[0][SVT_DUP][0].tolist() == [sat - 1, sat, sat] and it[0][SVT_DUP][1].tolist() == [300] * 3


# ---- the simulation: a sample genome as a piecewise map onto the reference -----------------------------
def pieces(L, inv, dup):
    """The sample as [(sample_beg, sample_end, ref_beg, ref_end, reversed)]: the reference with [inv) inverted in
    place and [dup) repeated in tandem (the second copy and everything behind it is one collinear piece)."""
    (s, e), (s2, e2) = inv, dup
    assert 0 < s < e < s2 < e2 < L
    out, at = [], 0
    for r0, r1, rev in ((0, s, 0), (s, e, 1), (e, e2, 0), (s2, L, 0)):
        out.append((at, at + (r1 - r0), r0, r1, rev))
        at += r1 - r0
    return out


def alignments(pcs, u, v, rstrand):
    """The alignments of the read that is sample[u, v) (rstrand 1: its reverse complement), from the map alone:
    [(strand, r_beg, r_end, q_beg, q_end)], query coordinates in the read's own orientation."""
    out = []
    for sb, se, r0, r1, rev in pcs:
        a, b = max(u, sb), min(v, se)
        if a >= b:
            continue
        r_beg, r_end = (r1 - (b - sb), r1 - (a - sb)) if rev else (r0 + (a - sb), r0 + (b - sb))
        q_beg, q_end = (v - b, v - a) if rstrand else (a - u, b - u)
        out.append((rstrand ^ rev, r_beg, r_end, q_beg, q_end))
    return out


def records_of(reads, pcs):
    """One pileup record per alignment, soft-clipped to the read's length in REFERENCE orientation, every record's
    SA entries the read's other alignments: (pileup, table, crossing reads per breakpoint count)."""
    recs = []   # (pos, cigar, flag, read id, k)
    by_read = {}
    for rid, (u, v, rstrand) in enumerate(reads):
        als = alignments(pcs, u, v, rstrand)
        n = v - u
        by_read[rid] = []
        for k, (st, r_beg, r_end, q_beg, q_end) in enumerate(als):
            lead, trail = (n - q_end, q_beg) if st else (q_beg, n - q_end)
            cig = [(S, lead)] * (lead > 0) + [(M, r_end - r_beg)] + [(S, trail)] * (trail > 0)
            by_read[rid].append((r_beg, "-" if st else "+", cig))
            recs.append((r_beg, cig, 16 if st else 0, rid, k))
    order = sorted(range(len(recs)), key=lambda i: recs[i][0])
    sa = {}
    for new, i in enumerate(order):
        _, _, _, rid, k = recs[i]
        others = [(0, r_beg + 1, st, cig) for j, (r_beg, st, cig) in enumerate(by_read[rid]) if j != k]
        if others:
            sa[new] = others
    return world(1, [(0, recs[i][0], recs[i][1]) for i in order], sa, [recs[i][2] for i in order])


@pytest.mark.parametrize("seed", [1, 2])
def test_simulated_inversion_and_tandem_duplication(seed):
    rng = np.random.default_rng(seed)
    L, inv, dup = 40000, (10000, 13000), (20000, 22500)
    pcs = pieces(L, inv, dup)
    assert pcs[-1][1] == L + (dup[1] - dup[0])
    # the sample's breakpoints: the inversion's two, and the start of the second copy (= e' in sample coordinates)
    bps = {"inv_left": inv[0], "inv_right": inv[1], "dup": dup[1]}
    reads, crossing = [], {k: 0 for k in bps}
    for name, bp in bps.items():
        for rstrand in (0, 1):
            for _ in range(int(rng.integers(3, 7))):
                a, b = (int(x) for x in rng.integers(300, 900, size=2))
                reads.append((bp - a, bp + b, rstrand))
                crossing[name] += 1
    for _ in range(20):   # reads that cross nothing, on both strands, inside the inverted and the repeated piece too
        u = int(rng.integers(0, pcs[-1][1] - 1000))
        if all(not (u - 5 < bp < u + 805) for bp in bps.values()):
            reads.append((u, u + 800, int(rng.integers(0, 2))))
    pl, table = records_of(reads, pcs)
    n_cross = sum(crossing.values())
    assert len(table[0]) == 2 * n_cross and pl.n_reads == len(reads) + n_cross     # two records per crossing read
    calls, st, sp, mg, jst, rst = R.call(pl, table, min_support=1, junctions=True)
    got = [(int(c["type"]), int(c["pos"]), int(c["len"]), int(c["end"]), int(c["support"])) for c in calls]
    assert got == [(SVT_INV, inv[0], inv[1] - inv[0], inv[1], crossing["inv_left"] + crossing["inv_right"]),
                   (SVT_DUP, dup[0], dup[1] - dup[0], dup[1], crossing["dup"])]
    assert all(int(c["x_lo"]) == int(c["x_hi"]) and int(c["len_lo"]) == int(c["len_hi"]) for c in calls)
    assert rst == {"dup_items": crossing["dup"], "inv_items": crossing["inv_left"] + crossing["inv_right"], "skipped": 0,
                   "clusters": 2, "calls": 2}
    # no DEL / INS item anywhere: not from the junctions, not from the CIGARs
    jit, js = J.items(pl, table)
    assert js["del_items"] == 0 and js["ins_items"] == 0 and js["junctions"] == n_cross and jit == {}
    assert js["other"] == crossing["inv_left"] + crossing["inv_right"]      # (dq == 0: the duplication is no "other" there)
    assert len(R.call(pl, table, min_support=1, rearrangements=(), junctions=True)[0]) == 0
    assert [int(t) for t in R.call(pl, table, min_support=1, types=(), rearrangements=(SVT_INV,))[0]["type"]] == [SVT_INV]
    # the genotypes of such calls: the invalid record
    g = R.genotype(pl, table, calls, junctions=True)
    assert (g["gt"] == -1).all() and not g["alt"].any() and not g["span"].any()


def test_order_and_len_permille():
    """Calls of all four types at one (chrom, pos) come in type-code order INS, DEL, INV, DUP; len_permille cuts a
    DUP start cluster of two lengths."""
    reads, sa, flags = [], {}, []
    for _ in range(3):                                     # CIGAR: 300D and 80I at x = 2000
        reads.append((0, 1000, [(M, 1000), (D, 300), (M, 700)]))
        reads.append((0, 1000, [(M, 1000), (I, 80), (M, 700)]))
    for ln in (400, 400, 400, 900, 900, 900):              # DUP [2000, 2000 + ln): own = Lf ends at 2000 + ln, B starts at 2000
        sa[len(reads)] = [(0, 2000 + 1, "+", [(S, ln + 1000), (M, 500)])]
        reads.append((0, 1000, [(M, ln + 1000), (S, 500)]))
    for _ in range(3):                                     # INV [2000, 2600): own + ends at 2000, B - ends at 2600
        sa[len(reads)] = [(0, 2100 + 1, "-", [(M, 500), (S, 1000)])]
        reads.append((0, 1000, [(M, 1000), (S, 500)]))
    pl, table = world(1, reads, sa, [0] * len(reads))
    calls = R.call(pl, table)[0]
    assert [(int(c["type"]), int(c["pos"]), int(c["len"]), int(c["end"])) for c in calls] == \
        [(SVT_INS, 2000, 80, 2001), (SVT_DEL, 2000, 300, 2301), (SVT_INV, 2000, 600, 2600), (SVT_DUP, 2000, 650, 2650)]
    calls, st, sp, _, _, rst = R.call(pl, table, len_permille=100)
    assert [(int(c["type"]), int(c["len"]), int(c["support"])) for c in calls] == \
        [(SVT_INS, 80, 3), (SVT_DEL, 300, 3), (SVT_INV, 600, 3), (SVT_DUP, 400, 3), (SVT_DUP, 900, 3)]
    assert sp == {"candidates": 1, "split": 1, "groups": 2, "big": 0} and rst["clusters"] == 2 and rst["calls"] == 3
    assert st["events"] == 6 + 9 and st["clusters"] == 4 and st["calls"] == 5


def test_the_lifecycle_world_tells_its_scans_apart():
    """tests/test_gpu_rearr.py's ten-step test compares every scan of one engine with the model; a stale index shows
    there only if the models' own calls differ between the scans it could be taken from.  Models alone, no GPU."""
    import test_gpu_rearr as G
    pl, table, table2 = G.lifecycle_world()
    want = G.lifecycle_want(pl, G.lifecycle_steps(table, table2))
    assert len(want) == 7 and all(want)                                     # every scan calls something
    assert want[1] != want[2] and want[1] != want[4] and want[2] != want[4]  # steps 2, 3 and 5
    assert want[3] == want[1] and want[0] != want[5] and want[4] != want[6]
    assert (SVT_DUP, 18900, 20400, 1500, 2) in want[5] and (SVT_DUP, 20000, 20400, 400, 2) in want[0]
    assert any(w[0] == SVT_INV for w in want[0]) and not any(w[0] == SVT_INV for w in want[5])
