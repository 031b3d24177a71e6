"""Pure-Python / numpy model of include/svtrek_bnd.h (a helper, not a test): the BND items of a segment
table, svt_call_scan with svt_call_params.bnd and svt_genotype_calls after it.  Built on junction_ref
(segments, the junction's A and B) and rearr_ref.call (the calls of the other types); it knows nothing of
the engine's sorts.

    junction  A = the own segment, B = the smallest tuple strictly greater than A's (junction_ref); an item
              iff there is a B and B.tid != A.tid -- no length threshold
    breakend  a = (A.tid, p, A.strand), p = A.r_end on strand + / A.r_beg on -;
              b = (B.tid, q, 1 - B.strand), q = B.r_beg on strand + / B.r_end on -
    item      lo = the breakend of the smaller tid, hi the other: (tid_lo, x, tid_hi, y, o = 2 s_lo + s_hi);
              dropped and counted in skipped when x or y >= 2^30
    calls     per class (tid_lo, tid_hi, o): start clusters by x (neighbours <= link apart), each cut by y
              (neighbours > link apart) into groups; a group of c >= min_support items is a call of type
              SVT_BND: pos / end the rounded means of x / y, len 0, x_lo / x_hi and len_lo / len_hi the
              ranges of x and y, pad = (tid_hi + 1) << 2 | o, depth the reads of tid_lo over pos
    order     (chrom, pos, type code, len) over all the scan's calls, BND ties by (mate chrom, o, end)
    genotype  the other calls as rearr_ref gives them, BND calls the invalid record
"""
from __future__ import annotations

import numpy as np

from svtrek_amd._lib import CALL_DTYPE, SVT_BND, SVT_DEL, SVT_INS

import junction_ref
import rearr_ref

SAT = 1 << 30
BND_ZERO = {"items": 0, "skipped": 0, "classes": 0, "clusters": 0, "groups": 0, "calls": 0}


def breakend(rows):
    """The record's BND item from its rows (own segment first): None or (tid_lo, x, tid_hi, y, o), unclamped."""
    A = rows[0]
    later = [s for s in rows if junction_ref._key(s) > junction_ref._key(A)]
    if not later:
        return None
    B = min(later, key=junction_ref._key)
    if int(B["tid"]) == int(A["tid"]):
        return None
    sa, sb = int(A["strand"]), 1 - int(B["strand"])
    a = (int(A["tid"]), int(A["r_beg"]) if int(A["strand"]) else int(A["r_end"]), sa)
    b = (int(B["tid"]), int(B["r_end"]) if int(B["strand"]) else int(B["r_beg"]), sb)
    lo, hi = (a, b) if a[0] < b[0] else (b, a)
    return (lo[0], lo[1], hi[0], hi[1], 2 * lo[2] + hi[2])


def items(table):
    """([(tid_lo, x, tid_hi, y, o), ...] of the kept items in table order, {items, skipped}) of a table
    (read, off, seg)."""
    read, off, seg = table
    kept, n, skipped = [], 0, 0
    for k in range(len(read)):
        it = breakend(seg[int(off[k]):int(off[k + 1])])
        if it is None:
            continue
        n += 1
        if it[1] >= SAT or it[3] >= SAT:
            skipped += 1
        else:
            kept.append(it)
    return kept, {"items": n, "skipped": skipped}


def _runs(vals, link):
    """The maximal runs of sorted vals whose neighbours differ by <= link, as index ranges."""
    cuts = [0] + [i for i in range(1, len(vals)) if vals[i] - vals[i - 1] > link] + [len(vals)]
    return list(zip(cuts[:-1], cuts[1:]))


def bnd_calls(pl, table, link: int = 10, min_support: int = 3):
    """(CALL_DTYPE records of the BND calls, unordered; svt_call_bnd_stats' counts)."""
    kept, st = items(table)
    st = {**BND_ZERO, **st}
    by_class: dict = {}
    for t_lo, x, t_hi, y, o in kept:
        by_class.setdefault((t_lo, t_hi, o), []).append((x, y))
    st["classes"] = len(by_class)
    out = []
    for (t_lo, t_hi, o), its in by_class.items():
        its.sort()
        for a, b in _runs([x for x, _ in its], link):
            st["clusters"] += 1
            cl = sorted(its[a:b], key=lambda r: r[1])
            for g0, g1 in _runs([y for _, y in cl], link):
                st["groups"] += 1
                grp = cl[g0:g1]
                c = len(grp)
                if c < min_support:
                    continue
                st["calls"] += 1
                xs, ys = [x for x, _ in grp], [y for _, y in grp]
                pos, end = (sum(xs) + c // 2) // c, (sum(ys) + c // 2) // c
                r0, r1 = int(pl.tid_off[t_lo]), int(pl.tid_off[t_lo + 1])
                depth = int(((pl.pos[r0:r1].astype(np.int64) <= pos) & (pl.endpos[r0:r1].astype(np.int64) > pos)).sum())
                out.append((SVT_BND, t_lo + 1, pos, end, c, depth, 0, min(ys), max(ys), min(xs), max(xs), (t_hi + 1) << 2 | o))
    return np.array(out, dtype=CALL_DTYPE).reshape(len(out)), st


def order_key(c):
    """The engine's total order: (chrom, pos, type code, len), BND ties by (mate chrom, o, end)."""
    bnd = int(c["type"]) == SVT_BND
    return (int(c["chrom"]), int(c["pos"]), int(c["type"]), int(c["len"]),
            int(c["pad"]) >> 2 if bnd else 0, int(c["pad"]) & 3 if bnd else 0, int(c["end"]) if bnd else 0)


def call(pl, table, link: int = 10, min_support: int = 3, types=(SVT_DEL, SVT_INS), rearrangements=(), len_permille: int = 0,
         merge_gap: int = 0, merge_min: int = 20, junctions: bool = False, breakends: bool = True):
    """(CALL_DTYPE records in order, call stats, split stats, merge stats, junction stats, rearr stats, bnd stats)
    of a scan with bnd = breakends: rearr_ref.call's calls and stats, plus the BND calls."""
    base, st, sp, mg, jst, rst = rearr_ref.call(pl, table, link, min_support, tuple(types), tuple(rearrangements), len_permille,
                                                merge_gap, merge_min, junctions)
    st = dict(st)
    bst = dict(BND_ZERO)
    lists = [np.array(base, dtype=CALL_DTYPE).reshape(len(base))]
    if breakends:
        calls, bst = bnd_calls(pl, table, link, min_support)
        lists.append(calls)
        st["events"] += bst["items"]
        st["skipped"] += bst["skipped"]
        st["clusters"] += bst["clusters"]
        st["calls"] += bst["calls"]
    out = np.concatenate(lists)
    order = sorted(range(len(out)), key=lambda i: order_key(out[i]))
    return out[order], st, sp, mg, jst, rst, bst


def genotype(pl, table, calls, junctions: bool = False, merge_gap: int = 0, merge_min: int = 20, flank: int = 50):
    """GT_DTYPE records of svt_genotype_calls after a scan with bnd = 1: BND calls invalid (gt = -1, all zero),
    the others as after the same scan without breakends."""
    return rearr_ref.genotype(pl, table, calls, junctions, merge_gap, merge_min, flank)   # (type 6: invalid there too)
