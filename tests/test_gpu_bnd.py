"""svt_call_params.bnd on the HIP engine (include/svtrek_bnd.h): Engine.call(breakends=True) against the model
(tests/bnd_ref.py, pinned by tests/test_bnd_model.py) record for record, with call_stats, the split, merge,
junction and rearr stats and every bnd stat, on tables built to reach every path of svt_bnd.inc: the four
orientations from both read strands, records on both sides of a wave boundary (the append's ballot ranks), a
record of many rows, a contig without a pileup record, both clamps, one big group, many groups in one start
cluster, many classes, link 0 and 2^20; then the combined scan and its order, the list's lifecycle,
genotype_calls, the status codes and the CLI.  (bnd = 1 with 2^30 - 1 targets or more is SVT_ESTATE by a
host-side comparison; a pileup of that many contigs is not built here.)"""
import numpy as np
import pytest

from svtrek_amd import Engine, Params, SvtError
from svtrek_amd._lib import (JUNCTION_SEG_DTYPE, SVT_BND, SVT_DEL, SVT_DUP, SVT_EINVAL, SVT_ESTATE, SVT_INS, SVT_INV,
                             call_mate, has_bnd)

import bnd_ref as B
import call_ref
import junction_ref as J
import rearr_ref as R
from test_bnd_model import bnd, recs, world
from test_gpu_rearr import build, dup, inv, plain, same

pytestmark = pytest.mark.gpu
M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
NAMES = {"DEL": SVT_DEL, "INS": SVT_INS, "DUP": SVT_DUP, "INV": SVT_INV}
JN_STATS, RR_STATS, BND_STATS = tuple(J.JUNCTION_ZERO), tuple(R.REARR_ZERO), tuple(B.BND_ZERO)
CALL_STATS = ("events", "skipped", "clusters", "calls", "big_buckets")
BND_NONE = {**B.BND_ZERO, "build_ms": 0.0}
SAT = 1 << 30
U64 = np.uint64


def check(eng, pl, table, link=None, min_support=None, types=("DEL", "INS"), rearr=(), P=0, G=0, m=20, junctions=False,
          breakends=True, load=True):
    """Engine.call(breakends=...) == the model, every stat too; returns (calls, call stats, bnd stats)."""
    if load:
        eng.load_pileup(pl)
        eng.load_junctions(*table)
    want, wst, wsp, wmg, wjs, wrs, wbs = B.call(pl, table, 10 if link is None else link, 3 if min_support is None else min_support,
                                                tuple(NAMES[t] for t in types), tuple(NAMES[t] for t in rearr), P, G, m, junctions,
                                                breakends)
    got = eng.call(link=link, min_support=min_support, types=types, len_permille=P, merge_gap=G or None, merge_min=m if G else None,
                   junctions=junctions, rearrangements=rearr, breakends=breakends)
    same(got, want)
    st, js, ms, rs, bs = eng.call_stats(), eng.call_junction_stats(), eng.call_merge_stats(), eng.call_rearr_stats(), eng.call_bnd_stats()
    assert {k: st[k] for k in wst} == wst
    assert eng.call_split_stats() == wsp
    assert {k: ms[k] for k in wmg} == wmg
    assert {k: js[k] for k in JN_STATS} == wjs
    assert {k: rs[k] for k in RR_STATS} == wrs
    assert {k: bs[k] for k in BND_STATS} == wbs
    assert (bs["build_ms"] > 0) == bool(breakends)
    return got, st, bs


def bnd_rev(x, y, tid=0, mate=1, o=1):
    """bnd()'s junction as the read of the OTHER strand has it: the own segment is on `mate`, the SA entry on `tid`."""
    sa, sb = o >> 1, o & 1
    own = (mate, y, [(S, 500), (M, 500)]) if sb else (mate, y - 500, [(M, 500), (S, 500)])
    b = (tid, x + 1, "+", [(S, 500), (M, 500)]) if sa else (tid, x - 500 + 1, "-", [(M, 500), (S, 500)])
    return own, b, 16 if sb else 0


@pytest.fixture(scope="module")
def eng():
    with Engine(Params(), device=0) as e:
        assert has_bnd(e.lib)
        yield e


# ---- classification ------------------------------------------------------------------------------------
def test_four_orientations_from_both_read_strands(eng):
    specs = []
    for o in range(4):
        specs += [bnd(2000 + 3000 * o, 7000, o=o)] * 2 + [bnd_rev(2000 + 3000 * o, 7000, o=o)] * 2
    specs += [bnd_rev(40000, 900, tid=1, mate=2, o=2)] * 3          # A.tid > B.tid alone
    pl, table = build(specs, n_targets=3)
    got, st, bs = check(eng, pl, table)
    assert recs(got) == [(1, 2000, 2, 7000, 0, 4), (1, 5000, 2, 7000, 1, 4), (1, 8000, 2, 7000, 2, 4), (1, 11000, 2, 7000, 3, 4),
                         (2, 40000, 3, 900, 2, 3)]
    assert (got["type"] == SVT_BND).all() and not got["len"].any() and bs["classes"] == 5
    assert eng.call_junction_stats() == {**J.JUNCTION_ZERO, "build_ms": 0.0}        # junctions = 0: all zero
    check(eng, pl, table, junctions=True, load=False)
    assert eng.call_junction_stats()["other"] == 19                                  # ... and its meaning kept with it


def hand_world():
    """tests/test_bnd_model.py's classes / groups / min_support world, plus records without an item."""
    specs = [bnd(2000, 7000)] * 3 + [bnd(2000, 7000, mate=2)] * 3 + [bnd(2000, 7000, o=0)] * 3
    specs += [bnd(30000 + k, 9000) for k in (0, 1, 2)] + [bnd(30000 + k, 9011 + k) for k in (3, 4, 5)]
    specs += [bnd(50000 + 10 * k, 4000 + 10 * k) for k in range(6)]
    specs += [bnd(70000, 100)] * 3 + [bnd(70001, 200)] * 2
    specs += [dup(90000, 300)] * 3 + [inv(95000, 600, 1)] * 3                                    # B.tid == A.tid: no item
    specs += [((0, 99000, [(M, 500), (S, 500)]), (0, 99001, "+", [(M, 500), (S, 500)]), 0)] * 3      # an equal tuple: no B
    return build(specs, n_targets=3)


def test_classes_groups_min_support_and_link(eng):
    pl, table = hand_world()
    got, st, bs = check(eng, pl, table, types=())
    assert recs(got) == [(1, 2000, 2, 7000, 0, 3), (1, 2000, 2, 7000, 1, 3), (1, 2000, 3, 7000, 1, 3),
                         (1, 30001, 2, 9000, 1, 3), (1, 30004, 2, 9015, 1, 3), (1, 50025, 2, 4025, 1, 6), (1, 70000, 2, 100, 1, 3)]
    assert {k: bs[k] for k in BND_STATS} == {"items": 26, "skipped": 0, "classes": 3, "clusters": 6, "groups": 8, "calls": 7}
    for kw in (dict(link=9), dict(min_support=2), dict(min_support=1), dict(link=0), dict(link=1 << 20), dict(link=0, min_support=1),
               dict(link=1 << 20, min_support=1), dict(rearr=("DUP", "INV")), dict(types=("DEL",), P=100, G=50, junctions=True)):
        check(eng, pl, table, load=False, **kw)
    assert check(eng, pl, table, load=False, link=1 << 20, min_support=1)[2]["groups"] == 3      # one group a class


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_records_on_both_sides_of_a_wave_boundary(eng, n):
    """Every third record has no item, so the lanes' ranks in the append are not their lane numbers."""
    specs = [dup(5000 + 40 * k, 100 + k, k & 1) if k % 3 == 2 else (bnd if k & 4 else bnd_rev)(5000 + 40 * k, 1000 + 7 * k, o=k & 3)
             for k in range(n)]
    pl, table = build(specs, n_targets=2)
    got, _, bs = check(eng, pl, table, min_support=1, types=())
    assert len(got) == n - n // 3 == bs["items"]


def test_a_record_of_200_rows(eng):
    own = (0, 40000, [(M, 1000), (S, 6000)])
    far = [(1, 50000 + 7 * k, "+", [(S, 5000 + k), (M, 100)]) for k in range(99)]       # later in the query than B
    early = [(2, 60000 + k, "-", [(S, 5000), (M, 10 + k)]) for k in range(99)]           # q_beg 0, q_end < A's: before A
    b = (2, 43000 - 500 + 1, "-", [(M, 500), (S, 1000)])                                 # B: contig 3, strand -, ends at 43000
    pl, table = build([(own, far + [b] + early, 0)] * 3, n_targets=3)
    got, _, bs = check(eng, pl, table)
    assert recs(got) == [(1, 41000, 3, 43000, 0, 3)] and eng.call_junction_stats()["segments"] == 0
    assert bs["items"] == 3


def test_a_lo_contig_without_a_pileup_record(eng):
    """The own segments are on contig 3, the partners on contig 1, which no read touches: the calls are contig 1's, depth 0."""
    specs = [bnd_rev(2000, 7000, tid=0, mate=2, o=o) for o in (1, 1, 1, 3, 3, 3)]
    pl, table = build(specs, n_targets=4)
    assert pl.tid_off[1] == pl.tid_off[0] == 0
    got, _, _ = check(eng, pl, table, types=())
    assert recs(got) == [(1, 2000, 3, 7000, 1, 3), (1, 2000, 3, 7000, 3, 3)] and not got["depth"].any()
    specs = [bnd(2000, 7000, tid=1, mate=3)] * 3 + [plain((1, 1900, [(M, 500)]))] * 2   # ... and a depth where there are reads
    pl, table = build(specs, n_targets=4)
    assert [int(d) for d in check(eng, pl, table, types=())[0]["depth"]] == [2]


def test_x_and_y_at_2_30(eng):
    """2^30 - 1 is called, 2^30 dropped and counted, in x (N ops carry the own segment's end there) and in y."""
    big = (1 << 28) - 1
    reads, sa = [], {}
    for x, y in ((SAT - 1, 500), (SAT, 500), (5000, SAT - 1), (5000, SAT)):
        for _ in range(3):
            sa[len(reads)] = [(1, y + 1, "+", [(S, 100), (M, 50)])]
            reads.append((0, 10, [(M, 100)] + [(N, big)] * 3 + [(N, x - 110 - 3 * big)] + [(S, 50)]) if x > 5000 else
                         (0, x - 100, [(M, 100), (S, 50)]))
    order = sorted(range(len(reads)), key=lambda i: reads[i][:2])
    pl, table = world(2, [reads[i] for i in order], {k: sa[i] for k, i in enumerate(order)})
    got, st, bs = check(eng, pl, table, types=())
    assert recs(got) == [(1, 5000, 2, SAT - 1, 1, 3), (1, SAT - 1, 2, 500, 1, 3)]
    assert st["skipped"] == 6 and bs["skipped"] == 6 and bs["items"] == 12 and st["events"] == 12


# ---- sizes ---------------------------------------------------------------------------------------------
def test_5000_items_of_one_class_at_one_place(eng):
    pl, table = build([bnd(50500, 7000)] * 5000 + [bnd(50500, 7000, o=3)] * 3, n_targets=2)
    got, _, bs = check(eng, pl, table)
    assert recs(got) == [(1, 50500, 2, 7000, 1, 5000), (1, 50500, 2, 7000, 3, 3)] and bs["groups"] == 2


def test_5000_items_of_one_start_cluster_in_50_groups(eng):
    specs = [bnd(20000 + k % 7, 1000 * (k % 50) + k % 5) for k in range(5000)]
    pl, table = build(specs, n_targets=2)
    got, _, bs = check(eng, pl, table)
    assert len(got) == 50 and (got["support"] == 100).all() and bs["clusters"] == 1 and bs["groups"] == 50
    check(eng, pl, table, link=0, load=False)
    check(eng, pl, table, link=1 << 20, min_support=1, load=False)


def test_40_contigs_with_every_pair_a_class(eng):
    specs = []
    for a in range(40):
        for b in range(a + 1, 40):
            for o in range(4):
                f = bnd if (a + b + o) & 1 else bnd_rev
                specs += [f(1000 + 13 * b + o, 2000 + 17 * a, tid=a, mate=b, o=o) for _ in range(3)]
    pl, table = build(specs, n_targets=40)
    got, _, bs = check(eng, pl, table, types=())
    assert len(got) == 780 * 4 and bs["classes"] == 780 * 4 and bs["items"] == 780 * 12
    mc, o = call_mate(got)
    assert set(zip(got["chrom"].tolist(), mc.tolist())) == {(a + 1, b + 1) for a in range(40) for b in range(a + 1, 40)}
    check(eng, pl, table, link=1 << 20, min_support=1, load=False)


# ---- the combined scan ---------------------------------------------------------------------------------
def test_one_scan_of_all_five_types(eng):
    extra = [bnd(2000, 500, mate=2)] * 3 + [bnd(2000, 9000, mate=1)] * 3 + [bnd(2000, 600, mate=1)] * 3 + [bnd(2000, 9000, mate=1, o=0)] * 3
    extra += [bnd_rev(300, 800, tid=1, mate=2, o=2)] * 4
    specs = []                                              # test_gpu_rearr.combined()'s records: all four other types at 2000
    for _ in range(3):
        specs += [plain((0, 1000, [(M, 1000), (D, 300), (M, 700)])), plain((0, 1000, [(M, 1000), (I, 80), (M, 700)]))]
    for _ in range(2):
        specs += [((0, 1000, [(M, 1000), (S, 500)]), (0, 2300 + 1, "+", [(S, 1000), (M, 500)]), 0)]
    for _ in range(3):
        specs += [((0, 4000, [(M, 1000), (S, 590)]), (0, 5000 + 1, "+", [(S, 1090), (M, 500)]), 0)]
    for ln in (400, 400, 400, 900, 900, 900):
        specs += [((0, 1000, [(M, ln + 1000), (S, 500)]), (0, 2000 + 1, "+", [(S, ln + 1000), (M, 500)]), 0)]
    for kind in (0, 2, 3):
        specs += [inv(2000, 600, kind)]
    pl, table = build(specs + extra, n_targets=3)
    kw = dict(junctions=True, rearr=("DUP", "INV"), P=100, G=50)
    got, st, bs = check(eng, pl, table, **kw)
    assert [int(t) for t in got["type"]][:6] == [SVT_INS, SVT_DEL, SVT_INV, SVT_DUP, SVT_DUP] + [SVT_BND]
    at = got[(got["pos"] == 2000) & (got["type"] == SVT_BND)]
    assert recs(at) == [(1, 2000, 2, 9000, 0, 3), (1, 2000, 2, 600, 1, 3), (1, 2000, 2, 9000, 1, 3), (1, 2000, 3, 500, 1, 3)]
    assert recs(got[-1:]) == [(2, 300, 3, 800, 2, 4)] and bs["calls"] == 5
    # the same scan without bnd: the present engine's list, which is this list without its BND records
    base, bst, none = check(eng, pl, table, breakends=False, load=False, **kw)
    assert none == BND_NONE
    same(base, got[got["type"] != SVT_BND])
    for k in ("events", "clusters", "calls"):
        assert st[k] - bst[k] == bs[{"events": "items"}.get(k, k)]
    # two scans of the same inputs give identical lists
    again, _, _ = check(eng, pl, table, load=False, **kw)
    assert np.array_equal(again, got)
    # types = () with bnd = 1, with and without rearrangements
    only, _, _ = check(eng, pl, table, types=(), load=False)
    same(only, got[got["type"] == SVT_BND])
    check(eng, pl, table, types=(), rearr=("INV",), load=False)


# ---- lifecycle -----------------------------------------------------------------------------------------
def test_the_list_is_built_once_dropped_with_its_table_and_leaves_plain_scans_alone(eng):
    pl, table = hand_world()
    pl2, table2 = build([bnd(2000, 7000)] * 3 + [bnd(2000, 7000, mate=2)] * 3 + [bnd(2000, 7000, o=0)] * 3 +
                      [bnd(30000 + k, 9000, mate=2) for k in (0, 1, 2)] + [bnd(30000 + k, 9011 + k) for k in (3, 4, 5)] +
                      [bnd(50000 + 10 * k, 4000 + 10 * k) for k in range(6)] + [bnd(70000, 100)] * 3 + [bnd(70001, 200)] * 2 +
                      [dup(90000, 300)] * 3 + [inv(95000, 600, 1)] * 3 +
                      [((0, 99000, [(M, 500), (S, 500)]), (0, 99001, "+", [(M, 500), (S, 500)]), 0)] * 3, n_targets=3)
    assert np.array_equal(pl2.pos, pl.pos) and np.array_equal(pl2.cigar, pl.cigar)    # the same pileup, other SA entries
    with Engine(Params(), device=0) as fresh:
        fresh.load_pileup(pl)
        plain_calls, plain_st = fresh.call(min_support=1), fresh.call_stats()
        assert fresh.call_bnd_stats() == BND_NONE
    eng.load_pileup(pl)
    eng.load_junctions(*table)
    same(eng.call(min_support=1), plain_calls)                       # a plain scan before ...
    full, _, bs = check(eng, pl, table, min_support=1, load=False)
    t0 = bs["build_ms"]
    same(eng.call(min_support=1), plain_calls)                       # ... and after: the fresh context's records and stats
    st = eng.call_stats()
    assert {k: st[k] for k in CALL_STATS} == {k: plain_st[k] for k in CALL_STATS}
    assert eng.call_bnd_stats() == BND_NONE and eng.call_rearr_stats() == {**R.REARR_ZERO, "build_ms": 0.0}
    # built once: another link, other passes beside it -- the build's time stays the first one's
    assert check(eng, pl, table, link=9, load=False)[2]["build_ms"] == t0
    assert check(eng, pl, table, link=1 << 20, min_support=2, rearr=("DUP",), junctions=True, load=False)[2]["build_ms"] == t0
    eng.reindex()                                                    # untouched by svt_reindex
    got, _, bs = check(eng, pl, table, min_support=1, load=False)
    same(got, full)
    assert bs["build_ms"] == t0
    eng.load_junctions(*table2)                                      # dropped with its table: the new table's calls
    got2, _, bs2 = check(eng, pl, table2, min_support=1, load=False)
    assert not np.array_equal(got2, full) and (1, 30001, 3, 9000, 1, 3) in recs(got2) and (1, 30001, 3, 9000, 1, 3) not in recs(full)
    empty = (np.zeros(0, dtype=U64), np.zeros(1, dtype=U64), np.zeros(0, dtype=JUNCTION_SEG_DTYPE))
    eng.load_junctions(*empty)
    got, _, bs = check(eng, pl, empty, min_support=1, load=False)
    same(got, plain_calls)
    assert bs["items"] == 0
    eng.load_pileup(pl)                                              # a new pileup drops table and list
    with pytest.raises(SvtError) as e:
        eng.call(breakends=True)
    assert e.value.code == SVT_ESTATE
    eng.load_junctions(*table)
    same(check(eng, pl, table, min_support=1, load=False)[0], full)


# ---- genotypes and status codes ------------------------------------------------------------------------
def test_genotype_calls(eng):
    pl, table = build([plain((0, 1000, [(M, 1000), (D, 300), (M, 700)]))] * 3 + [plain((0, 1000, [(M, 1000), (I, 80), (M, 700)]))] * 3 +
                      [dup(2000, 400)] * 3 + [bnd(2000, 500, mate=2)] * 3 + [bnd(2000, 9000)] * 3, n_targets=3)
    for junctions in (False, True):
        calls, _, _ = check(eng, pl, table, junctions=junctions, rearr=("DUP",))
        g = eng.genotype_calls()
        assert np.array_equal(g, B.genotype(pl, table, calls, junctions=junctions))
        bb = calls["type"] == SVT_BND
        assert bb.sum() == 2 and (g["gt"][bb] == -1).all() and (g["gt"][:2] >= 0).all()
        for f in ("alt", "ref", "span", "alt_all", "gq"):
            assert not g[f][bb].any()
        assert not g["pl"][bb].any()
        base = eng.call(junctions=junctions, rearrangements=("DUP",))     # the other calls: the same scan's without bnd
        assert np.array_equal(eng.genotype_calls(), g[~bb]) and np.array_equal(base, calls[~bb])


def test_status_codes(eng):
    import ctypes as C

    from svtrek_amd._lib import SvtCallParams
    pl, table = build([plain((0, 1000, [(M, 1000), (D, 300), (M, 700)]))] * 3 + [bnd(2000, 9000)] * 3, n_targets=2)

    def code(fn, *a, **kw):
        with pytest.raises(SvtError) as e:
            fn(*a, **kw)
        return e.value.code

    with Engine(Params(), device=0) as e:
        e.load_pileup(pl)
        assert code(e.call, breakends=True) == SVT_ESTATE                        # no table for the loaded pileup
        assert len(e.call()) == 1
        e.load_junctions(*table)
        assert len(e.call(breakends=True)) == 2
        assert code(e.call_consensus) == SVT_ESTATE                              # no consensus after such a scan
        assert code(e.call, types=()) == SVT_EINVAL                              # no DEL / INS bit and nothing else
        assert len(e.call(types=(), breakends=True)) == 1
        prm, n = SvtCallParams(), C.c_uint64(0)
        e.lib.svt_call_default_params(e._h, C.byref(prm))
        assert prm.bnd == 0 and prm.rearr == 0
        for bad in (2, 3, 1 << SVT_BND, 1 << 31):
            prm.bnd = bad
            assert e.lib.svt_call_scan(e._h, C.byref(prm), C.byref(n)) == SVT_EINVAL, bad
        prm.bnd = 1
        assert e.lib.svt_call_scan(e._h, C.byref(prm), C.byref(n)) == 0 and n.value == 2
        prm.types = 0
        assert e.lib.svt_call_scan(e._h, C.byref(prm), C.byref(n)) == 0 and n.value == 1
        prm.bnd = 0
        assert e.lib.svt_call_scan(e._h, C.byref(prm), C.byref(n)) == SVT_EINVAL
        e.load_pileup(pl)                                                         # a new pileup drops the table
        assert code(e.call, breakends=True) == SVT_ESTATE
        assert len(e.call()) == 1


# ---- the CLI -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflate", ["cpu", "gpu"])
def test_cli_breakends(tmp_path, inflate):
    """`svtrek call --breakends [--split-reads] [--rearrangements] [--genotype]` on a BAM with SA tags: one translocation
    seen from both contigs and both strands, one tandem duplication and one CIGAR deletion against the model's VCF,
    byte for byte."""
    import os
    import subprocess

    from svtrek_amd import host

    import test_junction_ingest as T
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svtrek_amd", "svtrek")
    raws = [T.rec(0, 1000, [(M, 1500)]) for _ in range(2)]                                               # reference reads
    raws += [T.rec(0, 1000, [(M, 500), (D, 300), (M, 400)]) for _ in range(3)]                           # 300D at 1500
    raws += [T.rec(0, 1500, [(M, 500), (S, 400)], aux=T.sa_tag([(1, 7001, "+", "500S400M")])) for _ in range(3)]          # chr1:2000 | chr2:7000
    raws += [T.rec(1, 700, [(M, 500), (S, 300)], aux=T.sa_tag([(1, 801, "+", "500S300M")])) for _ in range(3)]   # DUP [800, 1200) of chr2
    raws += [T.rec(1, 7000, [(S, 500), (M, 400)], flag=16, aux=T.sa_tag([(0, 1501, "-", "500M400S")])) for _ in range(2)]  # ... from the other strand
    bam, vcf = T.write(tmp_path / "b.bam", raws), str(tmp_path / "c.vcf")
    pl, info, table = host.read_bam(bam, junctions=True)
    pl.flag = np.array([0] * 11 + [16] * 2, dtype=np.uint16)
    want = B.call(pl, table)[0]
    assert [(int(c["type"]), *r) for c, r in zip(want, recs(want))] == [(SVT_DEL, 1, 1500, 0, 1801, 0, 3), (SVT_BND, 1, 2000, 2, 7000, 1, 5)]
    names = [n.decode() for n in T.NAMES]

    def run(*args):
        return subprocess.run([cli, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    p = run("call", "-b", bam, "-o", vcf, "--inflate", inflate, "--breakends", "--verbose")
    assert p.returncode == 0 and p.stdout == "" and "calls 2" in p.stderr, p.stderr
    assert "breakends  items 5  skipped 0  classes 1  clusters 1  groups 1  calls 1  build " in p.stderr, p.stderr
    with open(vcf) as f:
        text = f.read()
    assert text == host.format_calls(want, names, breakends=True)
    assert "chr1\t2000\tsvtrek.BND.1\tN\tN[chr2:7000[\t.\tPASS\tSVTYPE=BND;CHR2=chr2;POS2=7000;SUPPORT=5;DEPTH=5;XRANGE=2000,2000;X2RANGE=7000,7000\n" in text
    p = run("call", "-b", bam, "--inflate", inflate, "--breakends", "--rearrangements", "DUP", "--split-reads", "--genotype")
    w = B.call(pl, table, rearrangements=(SVT_DUP,), junctions=True)[0]
    assert [int(t) for t in w["type"]] == [SVT_DEL, SVT_BND, SVT_DUP]
    assert p.returncode == 0 and p.stdout == host.format_calls(w, names, genotypes=B.genotype(pl, table, w, junctions=True),
                                                               rearrangements=("DUP",), breakends=True), p.stderr
    assert p.stdout.count("\t./.:0:0:0:0,0,0\n") == 2 and "##INFO=<ID=CHR2" in p.stdout
    p = run("call", "-b", bam, "--inflate", inflate)                      # without the flag: today's output
    assert p.returncode == 0 and p.stdout == host.format_calls(call_ref.call(pl)[0], names) and "BND" not in p.stdout and "CHR2" not in p.stdout
    p = run("call", "-b", bam, "--breakends", "--ins-seq")
    assert p.returncode != 0 and "--breakends" in p.stderr and "--ins-seq" in p.stderr and p.stdout == ""
