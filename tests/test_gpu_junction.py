"""svt_call_params.junctions on the HIP engine (include/svtrek_junction.h): Engine.call(junctions=True)
against the model (tests/junction_ref.py, pinned by tests/test_junction_model.py) record for record, with
call_stats and every junction stat, on tables built to reach every path of svt_junction.inc (the
classification's thresholds on both strands, records on both sides of a wave boundary, records of many
rows), the shape of the union index (junction events beside CIGAR and merged events, bucket edges, a
contig's last bucket, big buckets), its lifecycle, genotype_calls on junction calls and the status codes."""
import numpy as np
import pytest

from svtrek_amd import Engine, Params, SvtError, calls_to_sites, from_reads
from svtrek_amd._lib import CALL_DTYPE, JUNCTION_SEG_DTYPE, SVT_DEL, SVT_EINVAL, SVT_ESTATE, SVT_INS, has_junctions

import call_merge_ref
import call_ref
import genotype_ref
import junction_ref as J

pytestmark = pytest.mark.gpu
M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
NAMES = {"DEL": SVT_DEL, "INS": SVT_INS}
INT_STATS = tuple(J.JUNCTION_ZERO)
U64 = np.uint64


def same(got, want):
    assert got.dtype == CALL_DTYPE and want.dtype == CALL_DTYPE
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(want)} records differ; first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


def check(eng, pl, table, link=None, min_support=None, types=("DEL", "INS"), P=0, G=0, m=20, load=True):
    """Engine.call(junctions=True) == the model, every stat too; returns (calls, call stats, junction stats)."""
    if load:
        eng.load_pileup(pl)
        eng.load_junctions(*table)
    want, wst, wsp, wmg, wjs = J.call(pl, table, 10 if link is None else link, 3 if min_support is None else min_support,
                                      tuple(NAMES[t] for t in types), P, G, m)
    got = eng.call(link=link, min_support=min_support, types=types, len_permille=P, merge_gap=G or None, merge_min=m if G else None,
                   junctions=True)
    same(got, want)
    st, js, ms = eng.call_stats(), eng.call_junction_stats(), eng.call_merge_stats()
    assert {k: st[k] for k in wst} == wst
    assert eng.call_split_stats() == wsp
    assert {k: ms[k] for k in wmg} == wmg
    assert {k: js[k] for k in INT_STATS} == wjs
    assert js["build_ms"] > 0
    return got, st, js


def rec(c):
    return tuple(int(c[f]) for f in ("type", "pos", "end", "len", "support"))


def world(n_targets, reads, sa, flags=None):
    """(pileup, table) of reads given in (tid, pos) order -- a read's list index is its pileup index -- and
    sa = {read: [(tid, 1-based pos, strand, CIGAR), ...]}."""
    assert [(t, p) for t, p, _ in reads] == sorted((t, p) for t, p, _ in reads)
    pl = from_reads(n_targets, reads, clip={})
    pl.flag = np.array(flags if flags is not None else [0] * len(reads), dtype=np.uint16)
    return pl, J.segments(pl, sa)


def halves(x, ln, n=1, ins=False, tid=0, strand="+", left=1000, right=500):
    """n reads whose left record ends at x and whose SA entry stands for a deletion (an insertion) of ln:
    (reads, the SA entry of each)."""
    reads = [(tid, x - left, [(M, left), (S, right + (ln if ins else 0))])] * n
    entry = (tid, x + (0 if ins else ln) + 1, strand, [(S, left + (ln if ins else 0)), (M, right)])
    return reads, entry


def left_world(specs, n_targets=1, **kw):
    """world() of halves(*spec) for every spec, in spec order (ascending x)."""
    reads, sa = [], {}
    for spec in specs:
        rs, entry = halves(*spec) if isinstance(spec, tuple) else halves(**spec)
        for r in rs:
            sa[len(reads)] = [entry]
            reads.append(r)
    return world(n_targets, reads, sa, **kw)


@pytest.fixture(scope="module")
def eng():
    with Engine(Params(), device=0) as e:
        assert has_junctions(e.lib)
        yield e


def test_four_reads_cut_at_one_deletion(eng):
    whole = from_reads(1, [(0, 1000, [(M, 1000), (D, 300), (M, 1700)])] * 4, clip={})
    pl, table, _ = J.cut(whole, [(r, 1) for r in range(4)])
    got, st, js = check(eng, pl, table, min_support=3)
    assert [rec(c) for c in got] == [(SVT_DEL, 2000, 2301, 300, 4)] and int(got[0]["depth"]) == 0
    assert {k: js[k] for k in INT_STATS} == {"records": 8, "segments": 16, "junctions": 4, "del_items": 4, "ins_items": 0,
                                             "other": 0, "skipped": 0}
    assert len(eng.call()) == 0 and eng.call_stats()["events"] == 0            # the plain scan sees nothing
    assert eng.call_junction_stats() == {**J.JUNCTION_ZERO, "build_ms": 0.0}


THRESHOLDS = [(51, 0), (50, 0), (52, 1), (51, 1), (1, -50), (0, -51), (0, 50), (0, 49), (-50, 1), (-51, 1), (-50, 0), (-60, 0),
              (300, 40), (10, 400)]
WANT = [(SVT_DEL, 51), None, (SVT_DEL, 51), None, (SVT_DEL, 51), None, (SVT_INS, 50), None, (SVT_INS, 51), None, None, None,
        (SVT_DEL, 260), (SVT_INS, 390)]


@pytest.mark.parametrize("strand", [0, 1])
def test_every_threshold_pair_on_both_strands(eng, strand):
    """Three records per (dr, dq) pair, 10 kb apart; on the reverse strand the pileup record is the RIGHT
    segment on the reference (the query-first one) and the SA entry the left one."""
    reads, sa, xs = [], {}, []
    for k, (dr, dq) in enumerate(THRESHOLDS):
        base = 10000 * (k + 1)
        for _ in range(3):
            if strand == 0:   # own: [base, base + 1000) q [10, 1010); SA: r_beg = base + 1000 + dr, q_beg = 1010 + dq
                sa[len(reads)] = [(0, base + 1000 + dr + 1, "+", [(S, 1010 + dq), (M, 1000), (S, 10)])]
                reads.append((0, base, [(S, 10), (M, 1000), (S, 1010 + dq)]))
            else:             # own: [base, base + 1000) q_beg = its trailing clip 10; SA: r_end = base - dr, q_beg = 1010 + dq
                sa[len(reads)] = [(0, base - dr - 1000 + 1, "-", [(S, 10), (M, 1000), (S, 1010 + dq)])]
                reads.append((0, base, [(S, 1010 + dq), (M, 1000), (S, 10)]))
        xs.append(base + 1000 if strand == 0 else base - dr)
    pl, table = world(1, reads, sa, flags=[strand << 4] * len(reads))
    got, st, js = check(eng, pl, table)
    want = sorted((x, ty, ln) for x, w in zip(xs, WANT) if w for ty, ln in [w])
    assert [(int(c["pos"]), int(c["type"]), int(c["len"]), int(c["support"])) for c in got] == [(x, ty, ln, 3) for x, ty, ln in want]
    assert js["junctions"] == 3 * len(THRESHOLDS) and js["other"] == 3 and js["del_items"] == 12 and js["ins_items"] == 9


def test_chain_shuffled_sa_other_none_and_many_rows(eng):
    a, b, c = [(M, 1000), (S, 2100)], [(S, 1000), (M, 1000), (S, 1100)], [(S, 2100), (M, 1000)]
    ea, eb, ec = (0, 1001, "+", a), (0, 2301, "+", b), (0, 3301, "+", c)
    reads, sa = [], {}
    for k in range(3):                                       # a three-segment chain: 300 DEL at 2000, 100 INS at 3300
        sa[len(reads)] = [eb, ec] if k != 1 else [ec, eb]    # (shuffled SA order)
        reads.append((0, 1000, a))
    for k in range(3):
        sa[len(reads)] = [ea, ec] if k != 1 else [ec, ea]
        reads.append((0, 2300, b))
    for k in range(3):                                       # the query-last segment's records: no junction
        sa[len(reads)] = [ea, eb]
        reads.append((0, 3300, c))
    for k in range(3):                                       # other strand, other contig: other
        sa[len(reads)] = [(0, 20001, "-", b)] if k else [(1, 20001, "+", b)]
        reads.append((0, 18000, a))
    sa[len(reads)] = [(0, 30001, "+", a)]                    # an equal tuple: no junction
    reads.append((0, 30000, a))
    # a record of 200 rows: 198 decoys before A or far later in the query, the true B in the middle of them
    far = [(0, 50000 + 7 * k, "+", [(S, 5000 + k), (M, 100)]) for k in range(99)]
    early = [(0, 60000 + k, "+", [(M, 10 + k), (S, 5000)]) for k in range(99)]
    for _ in range(3):
        sa[len(reads)] = far + [(0, 41501, "+", [(S, 1000), (M, 500)])] + early
        reads.append((0, 40000, [(M, 1000), (S, 6000)]))
    reads.append((1, 5, [(M, 50)]))
    pl, table = world(2, reads, sa)
    got, st, js = check(eng, pl, table)
    assert [rec(c) for c in got] == [(SVT_DEL, 2000, 2301, 300, 3), (SVT_INS, 3300, 3301, 100, 3), (SVT_DEL, 41000, 41501, 500, 3)]
    assert js["junctions"] == 12 and js["other"] == 3 and js["records"] == 16 and js["segments"] == 3 * 200 + 9 * 3 + 3 * 2 + 2


def test_junction_items_cluster_with_cigar_and_merged_items(eng):
    whole = [(0, 1000, [(M, 1000), (D, 300), (M, 1700)])] * 2                       # 300D in the CIGAR at 2000
    frag = [(0, 1000, [(M, 1003), (D, 180), (M, 5), (D, 120), (M, 1500)])] * 2      # 180D 5M 120D at 2003
    hreads, entry = halves(2000, 300, n=2)                                           # junction items at the CIGAR items' own x
    reads = whole + frag + hreads                                                    # (all at pos 1000)
    pl, table = world(1, reads, {4: [entry], 5: [entry]})
    got, _, _ = check(eng, pl, table, min_support=1)
    assert [rec(c)[1:] for c in got] == [(2001, 2262, 260, 6), (2188, 2309, 120, 2)]
    got, _, _ = check(eng, pl, table, G=50, load=False)
    assert [rec(c) for c in got] == [(SVT_DEL, 2001, 2302, 300, 6)]
    got, _, _ = check(eng, pl, table, load=False)                                    # back on the plain base view
    assert [rec(c)[1:] for c in got] == [(2001, 2262, 260, 6)]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_records_on_both_sides_of_a_wave_boundary(eng, n):
    pl, table = left_world([(5000 + 40 * k, 100 + k) for k in range(n)])
    got, _, js = check(eng, pl, table, min_support=1)
    assert len(got) == n and js["del_items"] == n


def test_bucket_edge_both_strands_and_an_empty_contig(eng):
    """A cluster over the bucket edge at 1024; junctions of contig 3 behind the empty contig 2, its last ones from
    reverse-strand records (the SA entry is the LEFT segment there and x its end)."""
    reads, sa = [], {}
    for spec in [(1020, 300, 2), (1026, 300, 2), dict(x=900, ln=200, n=3, tid=2, left=500), dict(x=9000, ln=80, n=3, ins=True, tid=2)]:
        rs, entry = halves(*spec) if isinstance(spec, tuple) else halves(**spec)
        for r in rs:
            sa[len(reads)] = [entry]
            reads.append(r)
    flags = [0] * len(reads)
    for _ in range(3):
        sa[len(reads)] = [(2, 19201, "-", [(M, 500), (S, 500)])]                    # [19200, 19700), query-last
        reads.append((2, 20000, [(S, 500), (M, 500)]))
        flags.append(16)
    pl, table = world(3, reads, sa, flags=flags)
    got, st, js = check(eng, pl, table)
    assert [(int(c["chrom"]), *rec(c)) for c in got] == [(1, SVT_DEL, 1023, 1324, 300, 4), (3, SVT_DEL, 900, 1101, 200, 3),
                                                          (3, SVT_INS, 9000, 9001, 80, 3), (3, SVT_DEL, 19700, 20001, 300, 3)]
    assert js["junctions"] == 13 and js["other"] == 0 and js["del_items"] == 10
    assert len(check(eng, pl, table, link=5, load=False)[0]) == 3


def test_big_buckets(eng):
    """3 000 junction items at one x (more than a tile: the counting sort), and 2 500 CIGAR items in a contig's
    last bucket copied into the union beside that contig's junction items.  (A junction x never lies past its
    contig's reads by more than 50, so no junction item reaches a last bucket: H ops put the CIGAR items there.)"""
    rng = np.random.default_rng(5)
    lens = rng.integers(51, 5000, size=3000)
    reads, sa = [], {}
    for ln in lens:
        sa[len(reads)] = [(0, 50500 + int(ln) + 1, "+", [(S, 1000), (M, 10)])]
        reads.append((0, 49500, [(M, 1000), (S, 10)]))
    reads += [(0, 60000, [(M, 100)])]
    reads += [(1, 100, [(H, 300000 + 97 * (k % 500)), (D, 80), (M, 5)]) for k in range(2500)]
    for _ in range(3):
        sa[len(reads)] = [(1, 150 + 70 + 1, "+", [(S, 50), (M, 10)])]
        reads.append((1, 100, [(M, 50), (S, 10)]))
    pl, table = world(2, reads, sa)
    got, st, js = check(eng, pl, table)
    assert st["big_buckets"] == 2 and js["del_items"] == 3003
    assert int(got[0]["support"]) == 3000 and (int(got[0]["len_lo"]), int(got[0]["len_hi"])) == (int(lens.min()), int(lens.max()))
    assert len(got) == 502 and rec(got[1]) == (SVT_DEL, 150, 221, 70, 3) and (got["support"][2:] == 5).all()


def test_x_at_2_30(eng):
    sat, big = 1 << 30, (1 << 28) - 1
    reads, sa = [], {}
    for x in (sat - 1, sat):
        for _ in range(3):
            sa[len(reads)] = [(0, x + 300 + 1, "+", [(S, 100), (M, 50)])]
            reads.append((0, 10, [(M, 100)] + [(N, big)] * 3 + [(N, x - 110 - 3 * big)] + [(S, 50)]))
    pl, table = world(1, reads, sa)
    got, st, js = check(eng, pl, table)
    assert [rec(c) for c in got] == [(SVT_DEL, sat - 1, sat + 300, 300, 3)]
    assert st["skipped"] == 3 and js["skipped"] == 3 and js["del_items"] == 6


def test_len_permille_with_an_allele_seen_only_as_junctions(eng):
    whole = [(0, 1000, [(M, 1000), (D, 300), (M, 1700)])] * 3
    hreads, entry = halves(2000, 5000, n=3)
    pl, table = world(1, whole + hreads, {3: [entry], 4: [entry], 5: [entry]})
    got, _, _ = check(eng, pl, table, P=100)
    assert [rec(c) for c in got] == [(SVT_DEL, 2000, 2301, 300, 3), (SVT_DEL, 2000, 7001, 5000, 3)]
    got, _, _ = check(eng, pl, table, load=False)
    assert [rec(c) for c in got] == [(SVT_DEL, 2000, 4651, 2650, 6)]


def test_empty_table_reindex_rebuilds_and_the_plain_scan(eng):
    whole = [(0, 1000 + 7 * k, [(M, 1000), (D, 300 + k), (M, 1700)]) for k in range(40)]
    whole += [(0, 5000, [(M, 1000), (D, 180), (M, 5), (D, 120), (M, 500)])] * 4   # two plain items a read, one merged item
    hreads, entry = halves(2500, 300, n=4)
    reads = sorted(whole + hreads, key=lambda r: (r[0], r[1]))
    idx = [k for k, r in enumerate(reads) if r[2][-1][0] == S]
    pl, table = world(1, reads, {k: [entry] for k in idx})
    empty = (np.zeros(0, dtype=U64), np.zeros(1, dtype=U64), np.zeros(0, dtype=JUNCTION_SEG_DTYPE))
    with Engine(Params(), device=0) as fresh:
        fresh.load_pileup(pl)
        plain, plain_st = fresh.call(min_support=1), fresh.call_stats()
    # n = 0: the base scan record for record
    got, st, js = check(eng, pl, empty, min_support=1)
    same(got, plain)
    assert {k: st[k] for k in ("events", "skipped", "clusters", "calls", "big_buckets")} == \
        {k: plain_st[k] for k in ("events", "skipped", "clusters", "calls", "big_buckets")}
    # another table replaces it and the index is rebuilt
    eng.load_junctions(*table)
    full, _, js = check(eng, pl, table, min_support=1, load=False)
    assert len(full) == len(plain) + 1 and js["del_items"] == 4
    # cached: the second scan does not build (the build's time is the first one's)
    t0 = js["build_ms"]
    assert check(eng, pl, table, min_support=1, load=False)[2]["build_ms"] == t0
    # the same records after svt_reindex
    eng.reindex()
    same(check(eng, pl, table, min_support=1, load=False)[0], full)
    # a change of merge_gap rebuilds on the merged view (the 180D 5M 120D reads are one item there), and back
    merged = check(eng, pl, table, min_support=1, G=50, load=False)[0]
    assert len(merged) == len(full) - 1 and eng.call_stats()["events"] == 44 + 4
    same(check(eng, pl, table, min_support=1, load=False)[0], full)
    assert eng.call_stats()["events"] == 48 + 4
    # a plain scan after a junction scan is the fresh context's
    same(eng.call(min_support=1), plain)
    st = eng.call_stats()
    assert {k: st[k] for k in ("events", "clusters", "calls")} == {k: plain_st[k] for k in ("events", "clusters", "calls")}
    assert eng.call_junction_stats() == {**J.JUNCTION_ZERO, "build_ms": 0.0}


def gt(g):
    return tuple(int(g[f]) for f in ("alt", "ref", "span", "alt_all", "gt"))


def test_genotype_calls_on_split_reads(eng):
    # 4 split + 4 spanning reference reads: 0/1, DV 4, DR 4
    whole = from_reads(1, [(0, 1000, [(M, 3000)])] * 4 + [(0, 1000, [(M, 1000), (D, 300), (M, 1700)])] * 4, clip={})
    pl, table, _ = J.cut(whole, [(r, 1) for r in range(4, 8)])
    calls, _, _ = check(eng, pl, table)
    g = eng.genotype_calls()
    assert np.array_equal(g, J.genotype(pl, table, calls))
    assert [gt(x) for x in g] == [(4, 4, 4, 4, 1)]
    # the batch entry point keeps the plain view: no ALT item there
    b = eng.genotype(calls_to_sites(calls))
    assert np.array_equal(b, genotype_ref.genotype(pl, calls_to_sites(calls)))
    assert [gt(x) for x in b] == [(0, 4, 4, 0, 0)]
    # 2 CIGAR + 2 split ALT reads, 4 reference reads
    pl, table, _ = J.cut(whole, [(6, 1), (7, 1)])
    calls, _, _ = check(eng, pl, table)
    g = eng.genotype_calls()
    assert np.array_equal(g, J.genotype(pl, table, calls))
    assert [gt(x) for x in g] == [(4, 4, 6, 4, 1)]
    assert (g["alt_all"] == calls["support"]).all()
    # ... and after a merged junction scan
    calls, _, _ = check(eng, pl, table, G=50, load=False)
    assert np.array_equal(eng.genotype_calls(), J.genotype(pl, table, calls, merge_gap=50))


def test_status_codes(eng):
    whole = from_reads(2, [(0, 1000, [(M, 1000), (D, 300), (M, 1700)])] * 4 + [(1, 5, [(M, 50)])], clip={})
    pl, (read, off, seg), _ = J.cut(whole, [(r, 1) for r in range(4)])

    def code(fn, *a, **kw):
        with pytest.raises(SvtError) as e:
            fn(*a, **kw)
        return e.value.code

    with Engine(Params(), device=0) as e:
        assert code(e.load_junctions, read, off, seg) == SVT_ESTATE               # before svt_load_pileup
        e.load_pileup(pl)
        assert code(e.call, junctions=True) == SVT_ESTATE                         # no table
        e.load_junctions(read, off, seg)
        assert len(e.call(junctions=True)) == 1
        assert code(e.call_consensus) == SVT_ESTATE                               # no inserted bases for junction calls
        bad = read.copy(); bad[1] = bad[0]
        assert code(e.load_junctions, bad, off, seg) == SVT_EINVAL                # not strictly ascending
        bad = read.copy(); bad[-1] = pl.n_reads
        assert code(e.load_junctions, bad, off, seg) == SVT_EINVAL                # past the pileup
        bad = off.copy(); bad[1] = bad[2]
        assert code(e.load_junctions, read, bad, seg) == SVT_EINVAL               # a record with no row
        bad = off.copy(); bad[1], bad[2] = bad[2], bad[1]
        assert code(e.load_junctions, read, bad, seg) == SVT_EINVAL               # not monotone
        for field, k, v in (("strand", 1, 2), ("r_end", 1, 0), ("q_end", 1, 0), ("tid", 1, 2), ("tid", 1, -1),
                            ("tid", 0, 1), ("r_beg", 0, int(seg[0]["r_beg"]) + 1), ("r_end", 0, int(seg[0]["r_end"]) + 1)):
            bad = seg.copy()
            bad[k][field] = v
            assert code(e.load_junctions, read, off, bad) == SVT_EINVAL, (field, k, v)
        assert len(e.call(junctions=True)) == 1                                   # the table before is still in place
        import ctypes as C
        from svtrek_amd._lib import SvtCallParams
        prm, n = SvtCallParams(), C.c_uint64(0)
        e.lib.svt_call_default_params(e._h, C.byref(prm))
        assert prm.junctions == 0
        prm.junctions = 2
        assert e.lib.svt_call_scan(e._h, C.byref(prm), C.byref(n)) == SVT_EINVAL
        # a record without a reference base (endpos = pos + 1): its own segment ends at pos, nowhere else
        zero = from_reads(1, [(0, 5, [(S, 10)]), (0, 7, [(M, 1)])], clip={})
        e.load_pileup(zero)
        for k, r_end, ok in ((0, 5, True), (0, 6, True), (0, 1000000, False), (1, 8, True), (1, 7, True), (1, 9, False), (1, 1000000, False)):
            one = (np.array([k], dtype=U64), np.array([0, 1], dtype=U64),
                   np.array([(0, 0, 5 + 2 * k, r_end, 0, 1)], dtype=JUNCTION_SEG_DTYPE))
            if ok:
                e.load_junctions(*one)
            else:
                assert code(e.load_junctions, *one) == SVT_EINVAL, (k, r_end)
        e.load_pileup(pl)                                                         # a new pileup drops the table
        assert code(e.call, junctions=True) == SVT_ESTATE
        assert len(e.call()) == 0


@pytest.mark.parametrize("inflate", ["cpu", "gpu"])
def test_cli_split_reads(tmp_path, inflate):
    """`svtrek call --split-reads [--genotype]` on a BAM with SA tags against the model's VCF."""
    import os
    import subprocess

    from svtrek_amd import host

    import test_junction_ingest as T
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svtrek_amd", "svtrek")
    raws = [T.rec(0, 1000, [(M, 3000)]) for _ in range(4)]                                       # reference reads
    raws += [T.rec(0, 1000, [(M, 1000), (D, 300), (M, 1700)]) for _ in range(2)]                 # the 300D in the CIGAR
    raws += [T.rec(0, 1000, [(M, 1000), (S, 1700)], aux=T.sa_tag([(0, 2301, "+", "1000S1700M")])) for _ in range(2)]
    raws += [T.rec(0, 2300, [(S, 1000), (M, 1700)], flag=2048, aux=T.sa_tag([(0, 1001, "+", "1000M1700S")])) for _ in range(2)]
    raws += [T.rec(1, 900, [(S, 480), (M, 600)], flag=16, aux=T.sa_tag([(1, 501, "-", "400M680S")])) for _ in range(3)]   # 80 bp INS, strand -
    bam, vcf = T.write(tmp_path / "s.bam", raws), str(tmp_path / "c.vcf")
    pl, info, table = host.read_bam(bam, junctions=True)
    pl.flag = np.array([0] * 10 + [16] * 3, dtype=np.uint16)
    want = J.call(pl, table)[0]
    assert [rec(c) for c in want] == [(SVT_DEL, 2000, 2301, 300, 4), (SVT_INS, 900, 901, 80, 3)]
    names = [n.decode() for n in T.NAMES]

    def run(*args):
        return subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    p = run("call", "-b", bam, "-o", vcf, "--inflate", inflate, "--split-reads", "--verbose")
    assert p.returncode == 0 and p.stdout == "" and "calls 2" in p.stderr, p.stderr
    assert "split-reads  records 7  segments 14  junctions 5  DEL items 2  INS items 3  other 0  skipped 0  malformed SA 0" in p.stderr, p.stderr
    with open(vcf) as f:
        assert f.read() == host.format_calls(want, names)
    p = run("call", "-b", bam, "--inflate", inflate, "--split-reads", "--genotype")
    assert p.returncode == 0 and p.stdout == host.format_calls(want, names, genotypes=J.genotype(pl, table, want)), p.stderr
    p = run("call", "-b", bam, "--inflate", inflate, "--split-reads", "--merge-gap", "50", "--len-permille", "100")
    assert p.returncode == 0 and p.stdout == host.format_calls(J.call(pl, table, len_permille=100, merge_gap=50)[0], names), p.stderr
    p = run("call", "-b", bam, "--inflate", inflate)                      # without the flag: the CIGAR ops alone
    assert p.returncode == 0 and p.stdout == host.format_calls(call_ref.call(pl)[0], names)
    p = run("call", "-b", bam, "--split-reads", "--ins-seq")
    assert p.returncode != 0 and "--split-reads" in p.stderr and "--ins-seq" in p.stderr
