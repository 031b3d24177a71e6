"""Numpy model of include/svtrek_call.h with svt_call_params.len_permille (a helper, not a test),
built on call_ref.items: it knows nothing of the engine's buckets.

    start cluster   call_ref's cluster: per (contig, type) a maximal run of sorted x whose
                    neighbours differ by <= link
    allele group    inside one start cluster the items sorted by len; between sorted neighbours
                    lo <= hi a cut iff hi - lo > max(link, lo * P // 1000); a group is a maximal run
                    without a cut (single linkage)
    call            a group of c >= min_support items: call_ref's record over the group's items
    order           (chrom, pos, type code, len)
    candidate       a start cluster of >= min_support items with
                    len_hi - len_lo > max(link, len_lo * P // 1000)

len_permille = 0 is call_ref.call itself, with every split stat zero.
"""
from __future__ import annotations

import numpy as np

from svtrek_amd._lib import CALL_DTYPE, SVT_DEL, SVT_INS

import call_ref

SAT = call_ref.SAT
SPLIT_ZERO = {"candidates": 0, "split": 0, "groups": 0, "big": 0}
CALL_TILE = 2048   # svt_call.inc's: a candidate of more items is "big"


def gap(lo, link: int, permille: int):
    """The largest step from len lo that is no cut (Python / int64 arithmetic: no overflow)."""
    return np.maximum(link, lo * permille // 1000)


def groups(ln: np.ndarray, link: int, permille: int):
    """The sorted order of ln and the group bounds [b0, b1, ...] in it."""
    o = np.argsort(ln, kind="stable")
    s = ln[o].astype(np.int64)
    cut = np.nonzero(np.diff(s) > gap(s[:-1], link, permille))[0] + 1
    return o, np.concatenate([[0], cut, [len(s)]])


def call(pl, link: int = 10, min_support: int = 3, types=(SVT_DEL, SVT_INS), len_permille: int = 0):
    """(CALL_DTYPE records in order, call stats {events, skipped, clusters, calls},
    split stats {candidates, split, groups, big})."""
    if len_permille == 0:
        calls, st = call_ref.call(pl, link, min_support, types)
        return calls, st, dict(SPLIT_ZERO)
    rows = []
    st = {"events": 0, "skipped": 0, "clusters": 0, "calls": 0}
    sp = dict(SPLIT_ZERO)
    for tid in range(pl.n_targets):
        a, b = int(pl.tid_off[tid]), int(pl.tid_off[tid + 1])
        if a == b:
            continue
        pos, endpos = pl.pos[a:b].astype(np.int64), pl.endpos[a:b].astype(np.int64)
        it = call_ref.items(pl, tid)
        for ty in types:
            x, ln = it[ty]
            st["events"] += len(x)
            st["skipped"] += int((x >= SAT).sum())
            x, ln = x[x < SAT], ln[x < SAT]
            if not len(x):
                continue
            o = np.argsort(x, kind="stable")
            x, ln = x[o], ln[o]
            head = np.concatenate([[0], np.nonzero(np.diff(x) > link)[0] + 1])
            st["clusters"] += len(head)
            for h0, h1 in zip(head, np.concatenate([head[1:], [len(x)]])):
                cx, cl = x[h0:h1], ln[h0:h1]
                lo, hi = int(cl.min()), int(cl.max())
                cand = len(cx) >= min_support and hi - lo > max(link, lo * len_permille // 1000)
                go, gb = groups(cl, link, len_permille)
                if cand:
                    sp["candidates"] += 1
                    sp["split"] += 1 if len(gb) > 2 else 0
                    sp["groups"] += len(gb) - 1
                    sp["big"] += 1 if len(cx) > CALL_TILE else 0
                else:
                    assert len(gb) == 2 or len(cx) < min_support   # no other cluster holds a cut that matters
                for g0, g1 in zip(gb[:-1], gb[1:]):
                    c = int(g1 - g0)
                    if c < min_support:
                        continue
                    gx, gl = cx[go[g0:g1]], cl[go[g0:g1]]
                    p = (int(gx.sum()) + c // 2) // c
                    end = (int((gx + gl + 1).sum()) + c // 2) // c if ty == SVT_DEL else p + 1
                    depth = int(((pos <= p) & (endpos > p)).sum())
                    rows.append((ty, tid + 1, p, end, c, depth, (int(gl.sum()) + c // 2) // c, int(gl.min()), int(gl.max()),
                                 int(gx.min()), int(gx.max()), 0))
    rows.sort(key=lambda r: (r[1], r[2], r[0], r[6]))
    st["calls"] = len(rows)
    return np.array(rows, dtype=CALL_DTYPE), st, sp
