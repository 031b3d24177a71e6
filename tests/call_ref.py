"""Numpy model of include/svtrek_call.h (a helper, not a test), from the pileup's columns alone:
pos, endpos and the CIGAR stream.  It knows nothing of the engine's buckets.

    items     D ops with len > 50 / I ops with len >= 50 as (x, len), x = the read's pos plus the
              lengths of every earlier op except I and S (H, P, N and the codes 9-15 advance x),
              saturated at 2^30; items with x >= 2^30 are dropped (stats "skipped")
    cluster   per (contig, type) a maximal run of sorted x whose neighbours differ by <= link
    call      a cluster of c >= min_support items: the rounded means (sum + c // 2) // c, the
              ranges, depth = reads with pos <= call.pos < endpos
    order     (chrom, pos, type code)
"""
from __future__ import annotations

import numpy as np

from svtrek_amd._lib import CALL_DTYPE, SVT_DEL, SVT_INS

SAT = 1 << 30


def items(pl, tid: int):
    """{SVT_DEL: (x, len), SVT_INS: (x, len)} of contig tid, int64, x saturated, in read order."""
    a, b = int(pl.tid_off[tid]), int(pl.tid_off[tid + 1])
    o0, o1 = int(pl.cig_off[a]), int(pl.cig_off[b])
    words = pl.cigar[o0:o1].astype(np.int64)
    op, ln = words & 15, words >> 4
    nops = np.diff(pl.cig_off[a:b + 1].astype(np.int64))
    first = pl.cig_off[a:b].astype(np.int64) - o0
    adv = np.where((op == 1) | (op == 4), 0, ln)
    csum = np.cumsum(adv)
    base = np.where(first > 0, csum[np.maximum(first, 1) - 1], 0) if len(csum) else np.zeros(b - a, dtype=np.int64)
    read_of = np.repeat(np.arange(b - a), nops)
    x = np.minimum(pl.pos[a:b].astype(np.int64)[read_of] + (csum - adv) - base[read_of], SAT)
    d, i = (op == 2) & (ln > 50), (op == 1) & (ln >= 50)
    return {SVT_DEL: (x[d], ln[d]), SVT_INS: (x[i], ln[i])}


def call(pl, link: int = 10, min_support: int = 3, types=(SVT_DEL, SVT_INS)):
    """(CALL_DTYPE records in order, stats {events, skipped, clusters, calls})."""
    rows = []
    st = {"events": 0, "skipped": 0, "clusters": 0, "calls": 0}
    for tid in range(pl.n_targets):
        a, b = int(pl.tid_off[tid]), int(pl.tid_off[tid + 1])
        if a == b:
            continue
        pos, endpos = pl.pos[a:b].astype(np.int64), pl.endpos[a:b].astype(np.int64)
        it = items(pl, tid)
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
                c = int(h1 - h0)
                if c < min_support:
                    continue
                cx, cl = x[h0:h1], ln[h0:h1]
                p = (int(cx.sum()) + c // 2) // c
                end = (int((cx + cl + 1).sum()) + c // 2) // c if ty == SVT_DEL else p + 1
                depth = int(((pos <= p) & (endpos > p)).sum())
                rows.append((ty, tid + 1, p, end, c, depth, (int(cl.sum()) + c // 2) // c, int(cl.min()), int(cl.max()),
                             int(cx.min()), int(cx.max()), 0))
    rows.sort(key=lambda r: (r[1], r[2], r[0]))
    st["calls"] = len(rows)
    return np.array(rows, dtype=CALL_DTYPE), st
