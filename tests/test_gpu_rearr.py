"""svt_call_params.rearr on the HIP engine (include/svtrek_rearr.h): Engine.call(rearrangements=...) against the
model (tests/rearr_ref.py, pinned by tests/test_rearr_model.py) record for record, with call_stats, the split,
merge and junction stats and every rearr stat, on tables built to reach every path of svt_rearr.inc (the
classification's thresholds on both strands, records on both sides of a wave boundary, a record of many rows),
the shape of the rearrangement index (bucket edges, an empty contig, a big bucket, both clamps), the combined
scan and its order, the index's lifecycle, genotype_calls, the status codes and the CLI."""
import numpy as np
import pytest

from svtrek_amd import Engine, Params, SvtError, from_reads
from svtrek_amd._lib import (CALL_DTYPE, JUNCTION_SEG_DTYPE, SVT_DEL, SVT_DUP, SVT_EINVAL, SVT_ESTATE, SVT_INS, SVT_INV,
                             has_rearr)

import call_ref
import junction_ref as J
import rearr_ref as R

pytestmark = pytest.mark.gpu
M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
NAMES = {"DEL": SVT_DEL, "INS": SVT_INS, "DUP": SVT_DUP, "INV": SVT_INV}
JN_STATS = tuple(J.JUNCTION_ZERO)
RR_STATS = tuple(R.REARR_ZERO)
CALL_STATS = ("events", "skipped", "clusters", "calls", "big_buckets")
U64 = np.uint64


def same(got, want):
    assert got.dtype == CALL_DTYPE and want.dtype == CALL_DTYPE
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(want)} records differ; first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


def check(eng, pl, table, link=None, min_support=None, types=("DEL", "INS"), rearr=("DUP", "INV"), P=0, G=0, m=20,
          junctions=False, load=True):
    """Engine.call(rearrangements=rearr) == the model, every stat too; returns (calls, call stats, rearr stats)."""
    if load:
        eng.load_pileup(pl)
        eng.load_junctions(*table)
    want, wst, wsp, wmg, wjs, wrs = R.call(pl, table, 10 if link is None else link, 3 if min_support is None else min_support,
                                           tuple(NAMES[t] for t in types), tuple(NAMES[t] for t in rearr), P, G, m, junctions)
    got = eng.call(link=link, min_support=min_support, types=types, len_permille=P, merge_gap=G or None, merge_min=m if G else None,
                   junctions=junctions, rearrangements=rearr)
    same(got, want)
    st, js, ms, rs = eng.call_stats(), eng.call_junction_stats(), eng.call_merge_stats(), eng.call_rearr_stats()
    assert {k: st[k] for k in wst} == wst
    assert eng.call_split_stats() == wsp
    assert {k: ms[k] for k in wmg} == wmg
    assert {k: js[k] for k in JN_STATS} == wjs
    assert {k: rs[k] for k in RR_STATS} == wrs
    assert (rs["build_ms"] > 0) == bool(rearr)
    return got, st, rs


def rec(c):
    return tuple(int(c[f]) for f in ("type", "pos", "end", "len", "support"))


def world(n_targets, reads, sa, flags=None):
    """(pileup, table) of reads given in (tid, pos) order -- a read's list index is its pileup index -- and
    sa = {read: [(tid, 1-based pos, strand, CIGAR), ...]}."""
    assert [(t, p) for t, p, _ in reads] == sorted((t, p) for t, p, _ in reads)
    pl = from_reads(n_targets, reads, clip={})
    pl.flag = np.array(flags if flags is not None else [0] * len(reads), dtype=np.uint16)
    return pl, J.segments(pl, sa)


def dup(x, ln, strand=0, tid=0):
    """One record whose junction is the duplication [x, x + ln): (read, its SA entry, flag).  Strand +: the own
    segment is Lf = [x - 200, x + ln), B starts at x; strand -: the own segment is Rt = [x, x + 500)."""
    lf, rt = [(M, ln + 200), (S, 500)], [(S, ln + 200), (M, 500)]
    if strand == 0:
        return (tid, x - 200, lf), (tid, x + 1, "+", rt), 0
    return (tid, x, rt), (tid, x - 200 + 1, "-", lf), 16


def inv(x, ln, kind=0, tid=0):
    """One record whose junction is the inversion [x, x + ln): kind 0 / 1 own strand + with p < q / p > q, kind 2 / 3
    own strand - likewise.  p is the own segment's joined end, q the SA entry's."""
    p, q = (x, x + ln) if kind in (0, 2) else (x + ln, x)
    ends_at, starts_at = [(M, 500), (S, 500)], [(S, 500), (M, 500)]
    if kind < 2:   # own + ends at p (query-first: no leading clip); B - ends at q, its query start is its trailing clip
        return (tid, p - 500, ends_at), (tid, q - 500 + 1, "-", ends_at), 0
    return (tid, p, starts_at), (tid, q + 1, "+", starts_at), 16   # own - starts at p; B + starts at q


def build(specs, n_targets=1):
    """world() of (read, SA entry, flag) triples, sorted by (tid, pos) (stable)."""
    order = sorted(range(len(specs)), key=lambda i: (specs[i][0][0], specs[i][0][1]))
    reads = [specs[i][0] for i in order]
    sa = {k: ([specs[i][1]] if not isinstance(specs[i][1], list) else specs[i][1]) for k, i in enumerate(order) if specs[i][1] is not None}
    return world(n_targets, reads, sa, flags=[specs[i][2] for i in order])


def plain(read):
    return (read, None, 0)


@pytest.fixture(scope="module")
def eng():
    with Engine(Params(), device=0) as e:
        assert has_rearr(e.lib)
        yield e


# ---- classification ------------------------------------------------------------------------------------
DUP_CASES = [(-50, -1, None), (-50, 0, None), (-51, -2, None), (-51, -1, 51), (-51, 5, 51), (-300, 20, 300), (-300, 0, 300),
             (-300, -100, 300), (-300, -250, 300), (-300, -251, None), (-40, 100, None), (300, 0, None)]


@pytest.mark.parametrize("strand", [0, 1])
def test_dup_thresholds_on_both_strands(eng, strand):
    """Three records per (dr, dq) pair, 10 kb apart: dr in {-50, -51} x -d in {49, 50}, dq positive, zero and negative."""
    reads, sa, want = [], {}, []
    for k, (dr, dq, ln) in enumerate(DUP_CASES):
        base = 10000 * (k + 1)
        for _ in range(3):
            if strand == 0:   # own: [base, base + 1000) q [10, 1010); SA: r_beg = base + 1000 + dr, q_beg = 1010 + dq
                sa[len(reads)] = [(0, base + 1000 + dr + 1, "+", [(S, 1010 + dq), (M, 1000), (S, 10)])]
                reads.append((0, base, [(S, 10), (M, 1000), (S, 1010 + dq)]))
            else:             # own = Rt: [base, base + 1000) q_beg = its trailing clip 10; SA = Lf: r_end = base - dr
                sa[len(reads)] = [(0, base - dr - 1000 + 1, "-", [(S, 10), (M, 1000), (S, 1010 + dq)])]
                reads.append((0, base, [(S, 1010 + dq), (M, 1000), (S, 10)]))
        if ln:
            want.append((SVT_DUP, base + 1000 + dr if strand == 0 else base, ln, 3))
    pl, table = world(1, reads, sa, flags=[strand << 4] * len(reads))
    got, st, rs = check(eng, pl, table, junctions=True)
    assert [(int(c["type"]), int(c["pos"]), int(c["len"]), int(c["support"])) for c in got if c["type"] == SVT_DUP] == want
    assert rs["dup_items"] == 3 * len(want) and rs["inv_items"] == 0
    js = eng.call_junction_stats()            # svt_call_junction_stats keeps its meaning: (-51, 5) and (-300, 20) are its "other"
    assert js["other"] == 6 and js["junctions"] == 3 * len(DUP_CASES)


def test_inv_thresholds_in_all_four_geometries(eng):
    specs, want = [], []
    for k, (kind, w) in enumerate((kind, w) for kind in range(4) for w in (50, 51)):
        x = 10000 * (k + 1)
        specs += [inv(x, w, kind)] * 3
        if w > 50:
            want.append((SVT_INV, x, x + w, w, 3))
    specs += [inv(200000, 0, 0)] * 3          # a fold-back: p == q
    pl, table = build(specs)
    got, st, rs = check(eng, pl, table, junctions=True)
    assert [rec(c) for c in got] == want
    assert rs["inv_items"] == 12 and rs["dup_items"] == 0 and eng.call_junction_stats()["other"] == 27


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_records_on_both_sides_of_a_wave_boundary(eng, n):
    specs = [dup(5000 + 40 * k, 100 + k, k & 1) if k % 3 else inv(5000 + 40 * k, 100 + k, k & 3) for k in range(n)]
    pl, table = build(specs)
    got, _, rs = check(eng, pl, table, min_support=1)
    assert len(got) == n and rs["dup_items"] + rs["inv_items"] == n


def test_a_record_of_200_rows_other_contigs_and_equal_tuples(eng):
    own = (0, 40000, [(M, 1000), (S, 6000)])
    far = [(0, 50000 + 7 * k, "+", [(S, 5000 + k), (M, 100)]) for k in range(99)]       # later in the query than B
    early = [(0, 60000 + k, "-", [(S, 5000), (M, 10 + k)]) for k in range(99)]           # q_beg 0, q_end < A's: before A
    b = (0, 43000 - 500 + 1, "-", [(M, 500), (S, 1000)])                                 # B: strand -, ends at 43000
    specs = [(own, far + [b] + early, 0)] * 3
    specs += [((0, 70000, [(M, 500), (S, 500)]), (1, 70001, "-", [(M, 500), (S, 500)]), 0)] * 3   # another contig: no item
    specs += [((0, 80000, [(M, 500), (S, 500)]), (0, 80001, "+", [(M, 500), (S, 500)]), 0)] * 3   # an equal tuple: no junction
    specs += [plain((1, 5, [(M, 50)]))]
    pl, table = build(specs, n_targets=2)
    got, _, rs = check(eng, pl, table, junctions=True)
    assert [rec(c) for c in got] == [(SVT_INV, 41000, 43000, 2000, 3)]
    assert rs["inv_items"] == 3 and eng.call_junction_stats()["segments"] == 3 * 200 + 6 * 2


# ---- buckets and clamps --------------------------------------------------------------------------------
def test_bucket_edge_and_an_empty_contig(eng):
    """Clusters over the bucket edge at 1024 (both rows), and items of contig 3 behind the empty contig 2."""
    specs = [dup(1020, 300)] * 2 + [dup(1026, 300, 1)] * 2 + [inv(1018, 700, 0)] * 2 + [inv(1027, 700, 3)] * 2
    specs += [dup(900, 200, 1, tid=2)] * 3 + [inv(9000, 80, 2, tid=2)] * 3
    pl, table = build(specs, n_targets=3)
    got, _, rs = check(eng, pl, table)
    assert [(int(c["chrom"]), *rec(c)) for c in got] == [(1, SVT_INV, 1023, 1723, 700, 4), (1, SVT_DUP, 1023, 1323, 300, 4),
                                                          (3, SVT_DUP, 900, 1100, 200, 3), (3, SVT_INV, 9000, 9080, 80, 3)]
    assert len(check(eng, pl, table, link=5, load=False)[0]) == 2


def test_a_big_bucket_takes_the_counting_sort(eng):
    rng = np.random.default_rng(5)
    lens = rng.integers(51, 5000, size=3000)
    specs = [dup(50500, int(ln), int(ln) & 1) for ln in lens] + [inv(50600, 900, 1)] * 3 + [plain((0, 90000, [(M, 100)]))]
    pl, table = build(specs)
    got, st, rs = check(eng, pl, table)
    assert st["big_buckets"] == 1 and rs["dup_items"] == 3000
    assert rec(got[0])[:2] == (SVT_DUP, 50500) and int(got[0]["support"]) == 3000
    assert (int(got[0]["len_lo"]), int(got[0]["len_hi"])) == (int(lens.min()), int(lens.max()))
    assert rec(got[1]) == (SVT_INV, 50600, 51500, 900, 3)


def test_x_at_2_30(eng):
    """x = 2^30 - 1 is called, x = 2^30 dropped and counted, for both types: N ops carry the own segment's end there."""
    sat, big = 1 << 30, (1 << 28) - 1
    reads, sa = [], {}
    for x in (sat - 1, sat):
        for _ in range(3):   # INV: the own segment + ends at p = x, B - ends at x + 300
            sa[len(reads)] = [(0, x + 300 - 50 + 1, "-", [(M, 50), (S, 100)])]
            reads.append((0, 10, [(M, 100)] + [(N, big)] * 3 + [(N, x - 110 - 3 * big)] + [(S, 50)]))
        for _ in range(3):   # DUP: the own segment + ends at x + 400, B + starts at x
            sa[len(reads)] = [(0, x + 1, "+", [(S, 100), (M, 50)])]
            reads.append((0, 10, [(M, 100)] + [(N, big)] * 4 + [(N, x + 400 - 110 - 4 * big)] + [(S, 50)]))
    pl, table = world(1, reads, sa)
    got, st, rs = check(eng, pl, table)
    assert [rec(c) for c in got] == [(SVT_INV, sat - 1, sat + 299, 300, 3), (SVT_DUP, sat - 1, sat + 399, 400, 3)]
    assert st["skipped"] == 6 and rs["skipped"] == 6 and rs["dup_items"] == 6 and rs["inv_items"] == 6
    assert check(eng, pl, table, rearr=("INV",), load=False)[2]["skipped"] == 3


def test_len_at_the_clamp(eng):
    big = (1 << 28) - 1
    reads, sa = [], {}
    for _ in range(3):   # an inversion of 2^28 + 5
        sa[len(reads)] = [(0, 1100 + big + 6 - 500 + 1, "-", [(M, 500), (S, 100)])]
        reads.append((0, 1000, [(M, 100), (S, 500)]))
    for _ in range(3):   # ... and one of exactly 2^28 - 1
        sa[len(reads)] = [(0, 5100 + big - 500 + 1, "-", [(M, 500), (S, 100)])]
        reads.append((0, 5000, [(M, 100), (S, 500)]))
    pl, table = world(1, reads, sa)
    got, _, _ = check(eng, pl, table)
    assert [rec(c) for c in got] == [(SVT_INV, 1100, 1100 + big, big, 3), (SVT_INV, 5100, 5100 + big, big, 3)]


# ---- the combined scan ---------------------------------------------------------------------------------
def combined():
    specs = []
    for _ in range(3):                                     # CIGAR: 300D and 80I at x = 2000
        specs += [plain((0, 1000, [(M, 1000), (D, 300), (M, 700)])), plain((0, 1000, [(M, 1000), (I, 80), (M, 700)]))]
    for _ in range(2):                                     # junction DEL at 2000: clusters with the CIGAR ones
        specs += [((0, 1000, [(M, 1000), (S, 500)]), (0, 2300 + 1, "+", [(S, 1000), (M, 500)]), 0)]
    for _ in range(3):                                     # a junction INS of 90 at 5000, seen in no CIGAR
        specs += [((0, 4000, [(M, 1000), (S, 590)]), (0, 5000 + 1, "+", [(S, 1090), (M, 500)]), 0)]
    for ln in (400, 400, 400, 900, 900, 900):              # DUP [2000, 2000 + ln)
        specs += [((0, 1000, [(M, ln + 1000), (S, 500)]), (0, 2000 + 1, "+", [(S, ln + 1000), (M, 500)]), 0)]
    for kind in (0, 2, 3):                                 # INV [2000, 2600), three geometries
        specs += [inv(2000, 600, kind)]
    return build(specs)


def test_one_scan_of_all_four_types_in_type_code_order(eng):
    pl, table = combined()
    got, st, rs = check(eng, pl, table, junctions=True)
    assert [rec(c) for c in got] == [(SVT_INS, 2000, 2001, 80, 3), (SVT_DEL, 2000, 2301, 300, 5), (SVT_INV, 2000, 2600, 600, 3),
                                     (SVT_DUP, 2000, 2650, 650, 6), (SVT_INS, 5000, 5001, 90, 3)]
    assert st["events"] == 3 + 3 + 2 + 3 + 6 + 3 and rs["clusters"] == 2 and rs["calls"] == 2
    got, st, rs = check(eng, pl, table, junctions=True, P=100, load=False)       # the DUP start cluster holds two lengths
    assert [(int(c["type"]), int(c["len"]), int(c["support"])) for c in got] == \
        [(SVT_INS, 80, 3), (SVT_DEL, 300, 5), (SVT_INV, 600, 3), (SVT_DUP, 400, 3), (SVT_DUP, 900, 3), (SVT_INS, 90, 3)]
    assert eng.call_split_stats() == {"candidates": 1, "split": 1, "groups": 2, "big": 0} and rs["calls"] == 3
    got, _, _ = check(eng, pl, table, load=False)                                 # without the junction items
    assert [rec(c)[:2] + rec(c)[3:] for c in got] == [(SVT_INS, 2000, 80, 3), (SVT_DEL, 2000, 300, 3), (SVT_INV, 2000, 600, 3),
                                                      (SVT_DUP, 2000, 650, 6)]
    got, st, _ = check(eng, pl, table, types=(), rearr=("INV",), load=False)      # a rearrangement-only scan
    assert [rec(c) for c in got] == [(SVT_INV, 2000, 2600, 600, 3)] and st["events"] == 3
    got, _, _ = check(eng, pl, table, types=("DEL",), rearr=("DUP",), G=50, load=False)
    assert [int(c["type"]) for c in got] == [SVT_DEL, SVT_DUP]


# ---- lifecycle -----------------------------------------------------------------------------------------
def test_plain_scan_after_cached_build_new_table_and_reindex(eng):
    pl, table = combined()
    with Engine(Params(), device=0) as fresh:
        fresh.load_pileup(pl)
        plain_calls, plain_st = fresh.call(min_support=1), fresh.call_stats()
        assert fresh.call_rearr_stats() == {**R.REARR_ZERO, "build_ms": 0.0}
    full, _, rs = check(eng, pl, table, min_support=1)
    # a scan without rearrangements after one with them is the fresh context's, in records and stats
    same(eng.call(min_support=1), plain_calls)
    st = eng.call_stats()
    assert {k: st[k] for k in CALL_STATS} == {k: plain_st[k] for k in CALL_STATS}
    assert eng.call_rearr_stats() == {**R.REARR_ZERO, "build_ms": 0.0}
    assert eng.call_split_stats() == {"candidates": 0, "split": 0, "groups": 0, "big": 0}
    # cached: the second scan does not build (the build's time is the first one's), whatever the mask
    t0 = rs["build_ms"]
    assert check(eng, pl, table, min_support=1, load=False)[2]["build_ms"] == t0
    assert check(eng, pl, table, min_support=1, rearr=("DUP",), junctions=True, load=False)[2]["build_ms"] == t0
    # the same records after svt_reindex, from the same build
    eng.reindex()
    got, _, rs = check(eng, pl, table, min_support=1, load=False)
    same(got, full)
    assert rs["build_ms"] == t0
    # a new table rebuilds: an empty one gives the base scan, the old one everything again
    empty = (np.zeros(0, dtype=U64), np.zeros(1, dtype=U64), np.zeros(0, dtype=JUNCTION_SEG_DTYPE))
    eng.load_junctions(*empty)
    got, _, rs = check(eng, pl, empty, min_support=1, load=False)
    same(got, plain_calls)
    assert rs["dup_items"] == 0 and rs["inv_items"] == 0
    eng.load_junctions(*table)
    same(check(eng, pl, table, min_support=1, load=False)[0], full)


def lifecycle_world():
    """Twelve reads on two contigs, two of each: a 300D, a `180D 5M 120D` (one item for merge_gap >= 5), a
    `100D 55M 100D` (one item for merge_gap >= 55 only), a deletion junction, a DUP and an INV -- and a second table
    for the same pileup whose DUP starts 1100 earlier, in another bucket, and which has no INV record."""
    cig = [(0, 1000, [(M, 1000), (D, 300), (M, 700)]), (0, 5000, [(M, 1000), (D, 180), (M, 5), (D, 120), (M, 500)]),
           (0, 9000, [(M, 1000), (D, 100), (M, 55), (D, 100), (M, 500)])]
    jdel = ((1, 1000, [(M, 1000), (S, 500)]), (1, 2300 + 1, "+", [(S, 1000), (M, 500)]), 0)
    d, v = dup(20000, 400), inv(30000, 600, 0, tid=1)
    moved = (d[0], (0, 18900 + 1, "+", d[1][3]), 0)
    pl, table = build([plain(r) for r in cig] * 2 + [jdel, d, v] * 2, n_targets=2)
    pl2, table2 = build([plain(r) for r in cig] * 2 + [jdel, moved, plain(v[0])] * 2, n_targets=2)
    assert np.array_equal(pl.pos, pl2.pos) and len(table[0]) == 6 and len(table2[0]) == 4
    return pl, table, table2


def lifecycle_steps(table, table2):
    """check()'s arguments of the seven scans of the ten steps: 1 .. 5 on the first table, 7 and 9 on the second."""
    return [dict(table=table), dict(table=table, rearr=(), junctions=True, G=50), dict(table=table, rearr=(), G=60),
            dict(table=table, rearr=(), junctions=True, G=50), dict(table=table, rearr=(), junctions=True),
            dict(table=table2, junctions=True), dict(table=table2, rearr=())]


def lifecycle_want(pl, steps):
    """The models' calls of every scan, as rec() tuples (tests/test_rearr_model.py checks on the CPU that every scan
    calls something and that the scans a stale index would confuse differ)."""
    return [[rec(c) for c in R.call(pl, s["table"], 10, 2, (SVT_DEL, SVT_INS), tuple(NAMES[t] for t in s.get("rearr", ("DUP", "INV"))),
                                   0, s.get("G", 0), 20, s.get("junctions", False))[0]] for s in steps]


def test_which_index_is_rebuilt_reused_or_dropped_when(eng):
    """One engine, one pileup, ten steps: every scan against the model, so that an index kept when its key changed, or
    dropped segments kept when the extents changed, shows as another scan's calls."""
    pl, table, table2 = lifecycle_world()
    kw = dict(min_support=2, load=False)
    steps = lifecycle_steps(table, table2)
    want = lifecycle_want(pl, steps)
    eng.load_pileup(pl)
    eng.load_junctions(*table)
    for s in steps[:5]:                                    # 1 .. 5
        check(eng, pl, **s, **kw)
    eng.load_junctions(*table2)                            # 6: drops the union and the rearrangement index
    got, _, rs = check(eng, pl, **steps[5], **kw)          # 7
    assert [rec(c) for c in got] == want[5] and rs["inv_items"] == 0
    eng.reindex()                                          # 8
    got, _, _ = check(eng, pl, **steps[6], **kw)           # 9: a plain scan
    same(got, call_ref.call(pl, min_support=2)[0])
    assert np.array_equal(eng.genotype_calls(), R.genotype(pl, table2, got))   # 10


# ---- genotypes and status codes ------------------------------------------------------------------------
def test_genotype_calls(eng):
    pl, table = combined()
    for junctions in (False, True):
        calls, _, _ = check(eng, pl, table, junctions=junctions)
        g = eng.genotype_calls()
        assert np.array_equal(g, R.genotype(pl, table, calls, junctions=junctions))
        rr = (calls["type"] == SVT_DUP) | (calls["type"] == SVT_INV)
        assert rr.sum() == 2 and (g["gt"][rr] == -1).all()
        for f in ("alt", "ref", "span", "alt_all", "gq"):
            assert not g[f][rr].any()
        assert not g["pl"][rr].any()
        # ... and the DEL / INS calls' records are those of the same scan without rearrangements
        base = eng.call(junctions=junctions)
        assert np.array_equal(eng.genotype_calls(), g[~rr]) and np.array_equal(base, calls[~rr])


def test_status_codes(eng):
    import ctypes as C

    from svtrek_amd._lib import SvtCallParams
    pl, table = combined()

    def code(fn, *a, **kw):
        with pytest.raises(SvtError) as e:
            fn(*a, **kw)
        return e.value.code

    with Engine(Params(), device=0) as e:
        e.load_pileup(pl)
        assert code(e.call, rearrangements=("DUP",)) == SVT_ESTATE              # no table for the loaded pileup
        assert len(e.call()) == 2
        e.load_junctions(*table)
        assert len(e.call(rearrangements="DUP,INV")) == 4                        # (a comma string)
        assert code(e.call_consensus) == SVT_ESTATE                              # no consensus after such a scan
        assert code(e.call, types=()) == SVT_EINVAL                              # no DEL / INS bit and no rearrangement
        assert len(e.call(types=(), rearrangements=("DUP",))) == 1
        with pytest.raises(ValueError):
            e.call(types=("DUP",))                                               # types keeps meaning DEL / INS only
        with pytest.raises(ValueError):
            e.call(rearrangements=("DEL",))
        prm, n = SvtCallParams(), C.c_uint64(0)
        e.lib.svt_call_default_params(e._h, C.byref(prm))
        assert prm.rearr == 0
        for bad in (1 << SVT_DEL, 1 << SVT_INS, 1, 1 << 5, (1 << SVT_DUP) | (1 << 6), 1 << 31):
            prm.rearr = bad
            assert e.lib.svt_call_scan(e._h, C.byref(prm), C.byref(n)) == SVT_EINVAL, bad
        prm.rearr = (1 << SVT_DUP) | (1 << SVT_INV)
        assert e.lib.svt_call_scan(e._h, C.byref(prm), C.byref(n)) == 0 and n.value == 4
        prm.types = 0
        assert e.lib.svt_call_scan(e._h, C.byref(prm), C.byref(n)) == 0 and n.value == 2
        prm.rearr = 0
        assert e.lib.svt_call_scan(e._h, C.byref(prm), C.byref(n)) == SVT_EINVAL
        e.load_pileup(pl)                                                         # a new pileup drops the table
        assert code(e.call, rearrangements=("INV",)) == SVT_ESTATE
        assert len(e.call()) == 2


# ---- the CLI -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflate", ["cpu", "gpu"])
def test_cli_rearrangements(tmp_path, inflate):
    """`svtrek call --rearrangements DUP,INV [--split-reads] [--genotype]` on a BAM with SA tags: one inversion, one
    tandem duplication and one CIGAR deletion against the model's VCF, byte for byte."""
    import os
    import subprocess

    from svtrek_amd import host

    import test_junction_ingest as T
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svtrek_amd", "svtrek")
    raws = [T.rec(0, 1000, [(M, 1500)]) for _ in range(2)]                                               # reference reads
    raws += [T.rec(0, 1000, [(M, 500), (D, 300), (M, 400)]) for _ in range(3)]                           # 300D at 1500
    raws += [T.rec(0, 1500, [(M, 500), (S, 400)], aux=T.sa_tag([(0, 2201, "-", "400M500S")])) for _ in range(2)]          # INV [2000, 2600), left
    raws += [T.rec(0, 2000, [(S, 400), (M, 500)], flag=16, aux=T.sa_tag([(0, 2601, "+", "500S400M")])) for _ in range(2)]  # ... right, strand -
    raws += [T.rec(1, 700, [(M, 500), (S, 300)], aux=T.sa_tag([(1, 801, "+", "500S300M")])) for _ in range(3)]   # DUP [800, 1200) of chr2
    bam, vcf = T.write(tmp_path / "r.bam", raws), str(tmp_path / "c.vcf")
    pl, info, table = host.read_bam(bam, junctions=True)
    pl.flag = np.array([0] * 7 + [16] * 2 + [0] * 3, dtype=np.uint16)
    want = R.call(pl, table)[0]
    assert [(int(c["chrom"]), *rec(c)) for c in want] == [(1, SVT_DEL, 1500, 1801, 300, 3), (1, SVT_INV, 2000, 2600, 600, 4),
                                                           (2, SVT_DUP, 800, 1200, 400, 3)]
    names = [n.decode() for n in T.NAMES]
    both = ("DUP", "INV")

    def run(*args):
        return subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    p = run("call", "-b", bam, "-o", vcf, "--inflate", inflate, "--rearrangements", "DUP,INV", "--verbose")
    assert p.returncode == 0 and p.stdout == "" and "calls 3" in p.stderr, p.stderr
    assert "rearrangements DUP,INV  DUP items 3  INV items 4  skipped 0  clusters 2  calls 2" in p.stderr, p.stderr
    with open(vcf) as f:
        text = f.read()
    assert text == host.format_calls(want, names, rearrangements=both)
    assert '##ALT=<ID=DUP,Description="Tandem duplication">\n##ALT=<ID=INV,Description="Inversion">\n' in text
    assert "chr1\t2000\tsvtrek.INV.1\tN\t<INV>\t.\tPASS\tSVTYPE=INV;END=2600;SVLEN=600;SUPPORT=4;" in text
    assert "chr2\t800\tsvtrek.DUP.1\tN\t<DUP>\t.\tPASS\tSVTYPE=DUP;END=1200;SVLEN=400;SUPPORT=3;" in text
    p = run("call", "-b", bam, "--inflate", inflate, "--rearrangements", "INV", "--split-reads", "--genotype")
    w = R.call(pl, table, rearrangements=(SVT_INV,), junctions=True)[0]
    assert p.returncode == 0 and p.stdout == host.format_calls(w, names, genotypes=R.genotype(pl, table, w, junctions=True),
                                                               rearrangements=("INV",)), p.stderr
    assert "##ALT=<ID=DUP" not in p.stdout and "\t./.:0:0:0:0,0,0\n" in p.stdout
    p = run("call", "-b", bam, "--inflate", inflate)                      # without the flag: today's output
    assert p.returncode == 0 and p.stdout == host.format_calls(call_ref.call(pl)[0], names) and "DUP" not in p.stdout
    p = run("call", "-b", bam, "--rearrangements", "DUP", "--ins-seq")
    assert p.returncode != 0 and "--rearrangements" in p.stderr and "--ins-seq" in p.stderr
    p = run("call", "-b", bam, "--rearrangements", "DEL")
    assert p.returncode != 0 and "--rearrangements expects" in p.stderr
    p = run("call", "-b", bam, "--types", "DUP")
    assert p.returncode != 0 and "--types expects" in p.stderr
