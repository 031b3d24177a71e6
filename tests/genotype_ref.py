"""Numpy model of include/svtrek_genotype.h (a helper, not a test), from the pileup's columns alone:
pos, endpos and the CIGAR stream.  It knows nothing of the engine's buckets or events: every item
is derived here together with the index of the read that carries it.

    items     D ops with len > 50 / I ops with len >= 50 as (x, len, read), x = the read's pos plus
              the lengths of every earlier op except I and S, saturated at 2^30 (x >= 2^30: no item)
    a, b      max(pos - flank, 0), end + flank
    span      reads of the contig with pos <= a and endpos > b
    alt_all   items of the site's type with x_lo <= x <= min(x_hi, 2^30 - 1), len_lo <= len <= len_hi
    alt       those whose read spans;  ref = max(span - alt, 0)
    likelihood(alt, ref)  the integer PL arithmetic
"""
from __future__ import annotations

import numpy as np

from svtrek_amd._lib import GT_DTYPE, GT_SITE_DTYPE, SVT_DEL, SVT_INS

SAT = 1 << 30
REF_COST = (223, 3010, 13010)
ALT_COST = (13010, 3010, 223)
U64 = (1 << 64) - 1


def items(pl, tid: int):
    """{SVT_DEL: (x, len, read), SVT_INS: (x, len, read)} of contig tid, int64; read = the index in the
    contig's reads."""
    a, b = int(pl.tid_off[tid]), int(pl.tid_off[tid + 1])
    o0, o1 = int(pl.cig_off[a]), int(pl.cig_off[b])
    words = pl.cigar[o0:o1].astype(np.int64)
    op, ln = words & 15, words >> 4
    nops = np.diff(pl.cig_off[a:b + 1].astype(np.int64))
    read_of = np.repeat(np.arange(b - a), nops)
    adv = np.where((op == 1) | (op == 4), 0, ln)
    before = np.cumsum(adv) - adv                       # the advance of every earlier op of the stream
    first = pl.cig_off[a:b].astype(np.int64) - o0       # each read's first op
    base = np.zeros(b - a, dtype=np.int64)
    has = nops > 0
    base[has] = before[first[has]]
    x = np.minimum(pl.pos[a:b].astype(np.int64)[read_of] + before - base[read_of], SAT)
    d, i = (op == 2) & (ln > 50) & (x < SAT), (op == 1) & (ln >= 50) & (x < SAT)
    return {SVT_DEL: (x[d], ln[d], read_of[d]), SVT_INS: (x[i], ln[i], read_of[i])}


def likelihood(alt: int, ref: int, ref_cost=REF_COST, alt_cost=ALT_COST):
    """(gt, gq, [pl0, pl1, pl2]) of the counts."""
    if alt + ref == 0:
        return -1, 0, [0, 0, 0]
    L = [(ref * int(ref_cost[g]) + alt * int(alt_cost[g])) & U64 for g in range(3)]
    gt = min(range(3), key=lambda g: (L[g], g))
    pl = [min((L[g] - L[gt] + 500) // 1000, 65535) for g in range(3)]
    return gt, min(min(pl[g] for g in range(3) if g != gt), 99), pl


def genotype(pl, sites, flank: int = 50, costs=(REF_COST, ALT_COST)) -> np.ndarray:
    """GT_DTYPE records of GT_SITE_DTYPE sites (any array with a site's fields: calls too)."""
    out = np.zeros(len(sites), dtype=GT_DTYPE)
    out["gt"] = -1
    cache = {}
    for k, s in enumerate(sites):
        ty, chrom = int(s["type"]), int(s["chrom"])
        x_lo, x_hi, len_lo, len_hi = (int(s[f]) for f in ("x_lo", "x_hi", "len_lo", "len_hi"))
        if ty not in (SVT_DEL, SVT_INS) or not 1 <= chrom <= pl.n_targets or x_lo > x_hi or len_lo > len_hi:
            continue
        r0, r1 = int(pl.tid_off[chrom - 1]), int(pl.tid_off[chrom])
        if r0 == r1:
            continue
        if chrom not in cache:
            cache[chrom] = (pl.pos[r0:r1].astype(np.int64), pl.endpos[r0:r1].astype(np.int64), items(pl, chrom - 1))
        pos, endpos, it = cache[chrom]
        a, b = max(int(s["pos"]) - flank, 0), int(s["end"]) + flank
        spans = (pos <= a) & (endpos > b)
        x, ln, read = it[ty]
        m = (x >= x_lo) & (x <= min(x_hi, SAT - 1)) & (ln >= len_lo) & (ln <= len_hi)
        span, alt_all, alt = int(spans.sum()), int(m.sum()), int(spans[read[m]].sum())
        ref = max(span - alt, 0)
        gt, gq, p = likelihood(alt, ref, *costs)
        out[k] = (alt, ref, span, alt_all, gt, gq, p, 0)
    return out


def sites(rows) -> np.ndarray:
    """[(type, chrom, pos, end, x_lo, x_hi, len_lo, len_hi), ...] -> GT_SITE_DTYPE."""
    return np.array([tuple(r) for r in rows], dtype=GT_SITE_DTYPE).reshape(len(rows))
