"""svt_call_params.len_permille on the CPU: the numpy model (tests/call_split_ref.py) with the answers
written out -- the worked example of include/svtrek_call.h, the gap thresholds, single linkage,
min_support per group, the candidate rule -- the model against the unsplit calls and the simulator's
truth, and the VCF text of split calls through svth_parse_line."""
import functools
from dataclasses import replace

import numpy as np

from svtrek_amd import from_reads, host, sim
from svtrek_amd._lib import SVT_DEL, SVT_INS

import call_ref
import call_split_ref

M, I, D = 0, 1, 2


def d_at(x, ln=100, tid=0, lead=200, op=D, tail=60):
    return (tid, x - lead, [(M, lead), (op, ln), (M, tail)])


def rec(c):
    return tuple(int(c[f]) for f in ("pos", "end", "len", "support"))


def worked_reads():
    return [d_at(x, 300, lead=50) for x in (100, 100, 100, 110)] + [d_at(104, 500, lead=50)] * 3


def test_worked_example():
    pl = from_reads(1, worked_reads(), clip={})
    calls, st, sp = call_split_ref.call(pl, link=10, len_permille=0)
    assert [rec(c) for c in calls] == [(103, 490, 386, 7)] and sp == call_split_ref.SPLIT_ZERO
    assert (int(calls[0]["len_lo"]), int(calls[0]["len_hi"])) == (300, 500)
    calls, st, sp = call_split_ref.call(pl, link=10, len_permille=100)
    assert [rec(c) for c in calls] == [(103, 404, 300, 4), (104, 605, 500, 3)]
    assert [tuple(int(c[f]) for f in ("x_lo", "x_hi", "len_lo", "len_hi", "depth")) for c in calls] == \
        [(100, 110, 300, 300, 7), (104, 104, 500, 500, 7)]
    assert st == {"events": 7, "skipped": 0, "clusters": 1, "calls": 2}
    assert sp == {"candidates": 1, "split": 1, "groups": 2, "big": 0}


def test_len_permille_zero_is_call_ref():
    pl = from_reads(1, worked_reads() + [d_at(900, 80, op=I)] * 4, clip={})
    for kw in ({}, {"link": 3, "min_support": 1}, {"types": (SVT_INS,)}):
        got, st, sp = call_split_ref.call(pl, len_permille=0, **kw)
        want, wst = call_ref.call(pl, **kw)
        assert np.array_equal(got, want) and st == wst and sp == call_split_ref.SPLIT_ZERO


def pair(a, b, link=10, permille=100, n=3):
    pl = from_reads(1, [d_at(1000, a)] * n + [d_at(1000, b)] * n, clip={})
    return call_split_ref.call(pl, link=link, len_permille=permille)


def test_gap_thresholds():
    calls, _, sp = pair(300, 330)            # 30 == 300 * 100 // 1000: no cut
    assert [rec(c)[2:] for c in calls] == [(315, 6)] and sp == call_split_ref.SPLIT_ZERO
    calls, _, sp = pair(300, 331)
    assert [rec(c)[2:] for c in calls] == [(300, 3), (331, 3)] and sp == {"candidates": 1, "split": 1, "groups": 2, "big": 0}
    calls, _, sp = pair(60, 70)              # 60 * 100 // 1000 = 6 < link = 10: the floor decides
    assert [rec(c)[2:] for c in calls] == [(65, 6)] and sp["candidates"] == 0
    calls, _, sp = pair(60, 71)
    assert [rec(c)[2:] for c in calls] == [(60, 3), (71, 3)] and sp["split"] == 1
    calls, _, _ = pair(309, 339)             # integer division: 309 * 100 // 1000 = 30 < 30.9
    assert len(calls) == 1
    calls, _, _ = pair(309, 340)
    assert len(calls) == 2
    calls, _, _ = pair(300, 600, permille=1000)
    assert len(calls) == 1
    calls, _, _ = pair(300, 601, permille=1000)
    assert len(calls) == 2


def test_single_linkage_keeps_a_chain_together():
    pl = from_reads(1, [d_at(1000, ln) for ln in (300, 320, 340, 360)], clip={})
    calls, _, sp = call_split_ref.call(pl, len_permille=100)
    assert [rec(c)[2:] for c in calls] == [(330, 4)]
    # 360 - 300 = 60 > 30: a candidate by its range, not split
    assert sp == {"candidates": 1, "split": 0, "groups": 1, "big": 0}


def test_min_support_applies_per_group():
    pl = from_reads(1, [d_at(1000, 300)] * 3 + [d_at(1001, 500)] * 2, clip={})
    calls, st, sp = call_split_ref.call(pl, min_support=3, len_permille=100)
    assert [rec(c) for c in calls] == [(1000, 1301, 300, 3)]
    assert st["clusters"] == 1 and sp == {"candidates": 1, "split": 1, "groups": 2, "big": 0}
    pl = from_reads(1, [d_at(1000, 300)] * 2 + [d_at(1001, 500)] * 2 + [d_at(1002, 900)], clip={})
    calls, st, sp = call_split_ref.call(pl, min_support=3, len_permille=100)
    assert len(calls) == 0 and st["calls"] == 0 and sp == {"candidates": 1, "split": 1, "groups": 3, "big": 0}
    assert len(call_split_ref.call(pl, min_support=3, len_permille=0)[0]) == 1


def test_candidate_rule():
    # below min_support: two lengths, no candidate; the range rule alone for the rest
    reads = [d_at(1000, 300), d_at(1000, 500)] + [d_at(5000, 300)] * 3 + [d_at(9000, 300)] * 2 + [d_at(9001, 330)] * 2
    reads += [d_at(13000, 100 + 40 * k) for k in range(5)]
    pl = from_reads(1, reads, clip={})
    calls, st, sp = call_split_ref.call(pl, min_support=3, len_permille=100)
    assert st["clusters"] == 4 and sp == {"candidates": 1, "split": 1, "groups": 5, "big": 0}
    assert [rec(c)[2:] for c in calls] == [(300, 3), (315, 4)]
    calls, st, sp = call_split_ref.call(pl, min_support=1, len_permille=100)
    assert sp == {"candidates": 2, "split": 2, "groups": 7, "big": 0} and len(calls) == 2 + 1 + 1 + 5


def test_order_by_pos_then_len_inside_a_cluster():
    # len order 300 < 500 < 900, pos order reversed; then two groups with one pos
    pl = from_reads(1, [d_at(1008, 300)] * 3 + [d_at(1004, 500)] * 3 + [d_at(1000, 900)] * 3, clip={})
    calls, _, _ = call_split_ref.call(pl, len_permille=100)
    assert [rec(c)[::2] for c in calls] == [(1000, 900), (1004, 500), (1008, 300)]
    pl = from_reads(1, [d_at(1000, 900)] * 3 + [d_at(1000, 300)] * 3, clip={})
    calls, _, _ = call_split_ref.call(pl, len_permille=100)
    assert [rec(c)[::2] for c in calls] == [(1000, 300), (1000, 900)]


@functools.lru_cache(maxsize=None)
def sim_case():
    """tests/test_call_model.py's recipe."""
    r = sim.generate(replace(sim.WORKLOADS["cfg4_1m_delins_30x_hifi"], n_loci=2000, n_targets=2))
    return r, call_ref.call(r.pileup)[0]


def test_split_calls_against_the_unsplit_calls_and_the_truth():
    r, base = sim_case()
    n_truth = len(r.loci)
    counts = []
    for P in (20, 50, 100, 200, 500):
        calls, st, sp = call_split_ref.call(r.pileup, len_permille=P)
        counts.append(len(calls))
        print(f"P = {P}: {len(calls)} split calls, {len(base)} unsplit, truth {n_truth}, split stats {sp}")
        for ty in (SVT_DEL, SVT_INS):
            for chrom in (1, 2):
                mine = np.sort(calls["pos"][(calls["type"] == ty) & (calls["chrom"] == chrom)].astype(np.int64))
                b = base[(base["type"] == ty) & (base["chrom"] == chrom)]
                lo = np.searchsorted(mine, b["x_lo"].astype(np.int64), side="left")
                hi = np.searchsorted(mine, b["x_hi"].astype(np.int64), side="right")
                assert (hi > lo).all(), f"P = {P}: an unsplit call without a split call inside its x range"
        assert len(calls) <= 1.01 * n_truth
        assert st["clusters"] == call_ref.call(r.pileup)[1]["clusters"]
    assert counts == [2003, 2002, 2001, 2000, 2000] and len(base) == 2000


def test_format_of_split_calls_parses_back():
    pl = from_reads(1, worked_reads() + [d_at(900, 80, op=I)] * 3 + [d_at(900, 800, op=I)] * 3, clip={})
    calls = np.concatenate([call_split_ref.call(pl, len_permille=100)[0],
                            call_split_ref.call(sim_case()[0].pileup, len_permille=20)[0][:200]])
    body = [ln for ln in host.format_calls(calls, ["1", "2"]).splitlines() if not ln.startswith("#")]
    assert len(body) == len(calls) and len({ln.split("\t")[2] for ln in body}) == len(body)   # the IDs stay unique
    for ln, c in zip(body, calls):
        act, got, err = host.parse_line(ln)
        assert act == 1 and err == "" and got == tuple(int(c[f]) for f in ("type", "chrom", "pos", "end")), ln
    assert "SVLEN=-300;SUPPORT=4;" in body[0] and "LENRANGE=300,300" in body[0]
    assert "SVLEN=-500;SUPPORT=3;" in body[1] and "END=605;" in body[1]
