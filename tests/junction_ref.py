"""Pure-Python / numpy model of include/svtrek_junction.h (a helper, not a test): the segment table, the
junction items, and svt_call_scan / svt_genotype_calls on the union of the base items and the junction
items.  It knows nothing of the engine's buckets or events.

    segment   {tid, strand, r_beg, r_end, q_beg, q_end} of one alignment: cl / ct = the leading / trailing
              run of S and H ops, qlen = sum of M I = X, rlen = sum of M D N = X, r_end = r_beg + rlen,
              strand +: q_beg = cl; strand -: q_beg = ct; q_end = q_beg + qlen
    table     one record per pileup record with SA entries, ascending read index: the own segment (from
              the pileup's CIGAR and flag 0x10), then the SA entries in tag order
    junction  A = the own segment, B = the segment with the smallest tuple (q_beg, q_end, tid, r_beg,
              strand) strictly greater than A's; qualifies iff same tid and strand; (Lf, Rt) = (A, B) on
              strand +, (B, A) on -; dr = Rt.r_beg - Lf.r_end, dq = B.q_beg - A.q_end, d = dr - dq
    item      DEL iff d > 50 and dr > 0: (Lf.r_end, d); INS iff -d >= 50 and dq > 0 and dr >= -50:
              (Lf.r_end, -d); -d >= 50 and dq > 0 and dr < -50 counts in other; len clamped to 2^28 - 1,
              x saturated at 2^30 (the scan drops and counts those); extent (min r_beg, max r_end)
    genotype  alt_all / alt count junction items too (an item spans by its extent), span is the pileup's,
              ref = max(span - (alt - alt_j), 0)
"""
from __future__ import annotations

import contextlib
import re

import numpy as np

from svtrek_amd._lib import GT_DTYPE, JUNCTION_SEG_DTYPE, SVT_DEL, SVT_INS
from svtrek_amd.pileup import Pileup, endpos_of

import call_merge_ref
import call_ref
import call_split_ref
import genotype_ref

SAT = call_ref.SAT
LEN_MAX = (1 << 28) - 1
JUNCTION_ZERO = {"records": 0, "segments": 0, "junctions": 0, "del_items": 0, "ins_items": 0, "other": 0, "skipped": 0}
OPS = "MIDNSHP=X"
Q_OPS, R_OPS, CLIP_OPS = (0, 1, 7, 8), (0, 2, 3, 7, 8), (4, 5)


def parse_cigar(cig) -> list[tuple[int, int]]:
    """[(op, len), ...] of a CIGAR string, a list of such pairs, or an array of BAM words."""
    if isinstance(cig, str):
        return [(OPS.index(c), int(n)) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", cig)]
    if isinstance(cig, np.ndarray):
        return [(int(w) & 15, int(w) >> 4) for w in cig]
    return [(int(op), int(ln)) for op, ln in cig]


def seg_of(tid: int, strand: int, r_beg: int, cig) -> tuple:
    """One segment row (tid, strand, r_beg, r_end, q_beg, q_end)."""
    ops = parse_cigar(cig)
    cl = ct = 0
    for op, ln in ops:
        if op not in CLIP_OPS:
            break
        cl += ln
    for op, ln in reversed(ops):
        if op not in CLIP_OPS:
            break
        ct += ln
    qlen = sum(ln for op, ln in ops if op in Q_OPS)
    rlen = sum(ln for op, ln in ops if op in R_OPS)
    q_beg = ct if strand else cl
    return (tid, strand, r_beg, r_beg + rlen, q_beg, q_beg + qlen)


def strand_of(pl, r: int) -> int:
    return int(pl.flag[r] >> 4) & 1 if pl.flag is not None else 0


def contig_of(pl, r: int) -> int:
    return int(np.searchsorted(pl.tid_off, r, side="right")) - 1


def segments(pl, sa: dict):
    """(read uint64 [n], off uint64 [n + 1], seg JUNCTION_SEG_DTYPE) of sa = {pileup read index: [(tid, 1-based
    pos, '+' / '-', CIGAR), ...]}: the records in ascending read index, the own segment first."""
    read, off, rows = [], [0], []
    for r in sorted(sa):
        own = seg_of(contig_of(pl, r), strand_of(pl, r), int(pl.pos[r]), pl.read_cigar(r))
        if pl.flag is not None and int(pl.flag[r]) & 4:   # (bam_endpos: an unmapped record covers no reference base)
            own = own[:3] + (own[2],) + own[4:]
        rows.append(own)
        for tid, pos1, st, cig in sa[r]:
            rows.append(seg_of(int(tid), 1 if st in ("-", 1) else 0, int(pos1) - 1, cig))
        read.append(r)
        off.append(len(rows))
    return (np.array(read, dtype=np.uint64), np.array(off, dtype=np.uint64),
            np.array(rows, dtype=JUNCTION_SEG_DTYPE).reshape(len(rows)))


def _key(s):
    return (int(s["q_beg"]), int(s["q_end"]), int(s["tid"]), int(s["r_beg"]), int(s["strand"]))


def junction(rows):
    """The record's junction from its rows (own segment first): None, ("other",), ("none",) or
    (type, tid, x, len, lo, hi) with x and len unclamped."""
    A = rows[0]
    later = [s for s in rows if _key(s) > _key(A)]
    if not later:
        return None
    B = min(later, key=_key)
    if int(B["tid"]) != int(A["tid"]) or int(B["strand"]) != int(A["strand"]):
        return ("other",)
    Lf, Rt = (B, A) if int(A["strand"]) else (A, B)
    dr = int(Rt["r_beg"]) - int(Lf["r_end"])
    dq = int(B["q_beg"]) - int(A["q_end"])
    d = dr - dq
    ext = (min(int(Lf["r_beg"]), int(Rt["r_beg"])), max(int(Lf["r_end"]), int(Rt["r_end"])))
    if d > 50 and dr > 0:
        return (SVT_DEL, int(A["tid"]), int(Lf["r_end"]), d, *ext)
    if -d >= 50 and dq > 0:
        if dr >= -50:
            return (SVT_INS, int(A["tid"]), int(Lf["r_end"]), -d, *ext)
        return ("other",)
    return ("none",)


def items(pl, table):
    """({tid: {SVT_DEL: (x, len, lo, hi), SVT_INS: ...}} int64 arrays, x saturated at 2^30 and len clamped,
    svt_call_junction_stats' counts) of a table (read, off, seg)."""
    read, off, seg = table
    st = dict(JUNCTION_ZERO)
    st["records"], st["segments"] = len(read), len(seg)
    acc: dict = {}
    for k in range(len(read)):
        j = junction(seg[int(off[k]):int(off[k + 1])])
        if j is None:
            continue
        st["junctions"] += 1
        if j[0] == "other":
            st["other"] += 1
        if j[0] in ("other", "none"):
            continue
        ty, tid, x, ln, lo, hi = j
        st["del_items" if ty == SVT_DEL else "ins_items"] += 1
        st["skipped"] += 1 if x >= SAT else 0
        acc.setdefault(tid, {SVT_DEL: [], SVT_INS: []})[ty].append((min(x, SAT), min(ln, LEN_MAX), lo, hi))
    out = {}
    for tid, by in acc.items():
        out[tid] = {ty: tuple(np.array([r[q] for r in rows], dtype=np.int64) for q in range(4)) for ty, rows in by.items()}
    return out, st


def _base_items(pl, tid: int, merge_gap: int, merge_min: int):
    """{type: (x, len, read)} of the base view, x saturated (not dropped)."""
    if merge_gap:
        return call_merge_ref.merged_items(pl, tid, merge_gap, merge_min)
    op, ln, read_of, x = call_merge_ref.walk(pl, tid)
    d, i = (op == 2) & (ln > 50), (op == 1) & (ln >= 50)
    x = np.minimum(x, SAT)
    return {SVT_DEL: (x[d], ln[d], read_of[d]), SVT_INS: (x[i], ln[i], read_of[i])}


@contextlib.contextmanager
def _items_are(pl, jit, merge_gap: int, merge_min: int):
    """call_ref.items replaced by the union of pl's base items and the junction items while the block runs."""
    z = np.zeros(0, dtype=np.int64)

    def call_items(p, tid):
        assert p is pl
        base = _base_items(pl, tid, merge_gap, merge_min)
        j = jit.get(tid, {})
        return {ty: (np.concatenate([base[ty][0], j.get(ty, (z, z))[0]]), np.concatenate([base[ty][1], j.get(ty, (z, z))[1]]))
                for ty in (SVT_DEL, SVT_INS)}
    keep = call_ref.items
    call_ref.items = call_items
    try:
        yield
    finally:
        call_ref.items = keep


def call(pl, table, link: int = 10, min_support: int = 3, types=(SVT_DEL, SVT_INS), len_permille: int = 0,
         merge_gap: int = 0, merge_min: int = 20):
    """(CALL_DTYPE records in order, call stats, split stats, merge stats, junction stats) of a scan with
    junctions = 1: call_ref / call_split_ref on the union of the base items and the junction items."""
    jit, jst = items(pl, table)
    with _items_are(pl, jit, merge_gap, merge_min):
        calls, st, sp = call_split_ref.call(pl, link, min_support, types, len_permille)
    mg = call_merge_ref.merge_stats(pl, merge_gap, merge_min) if merge_gap else dict(call_merge_ref.MERGE_ZERO)
    return calls, st, sp, mg, jst


def genotype(pl, table, sites, merge_gap: int = 0, merge_min: int = 20, flank: int = 50,
             costs=(genotype_ref.REF_COST, genotype_ref.ALT_COST)) -> np.ndarray:
    """GT_DTYPE records of svt_genotype_calls after a scan with junctions = 1."""
    jit, _ = items(pl, table)
    out = np.zeros(len(sites), dtype=GT_DTYPE)
    out["gt"] = -1
    for k, s in enumerate(sites):
        ty, chrom = int(s["type"]), int(s["chrom"])
        x_lo, x_hi, len_lo, len_hi = (int(s[f]) for f in ("x_lo", "x_hi", "len_lo", "len_hi"))
        if ty not in (SVT_DEL, SVT_INS) or not 1 <= chrom <= pl.n_targets or x_lo > x_hi or len_lo > len_hi:
            continue
        r0, r1 = int(pl.tid_off[chrom - 1]), int(pl.tid_off[chrom])
        if r0 == r1:
            continue
        pos, endpos = pl.pos[r0:r1].astype(np.int64), pl.endpos[r0:r1].astype(np.int64)
        a, b = max(int(s["pos"]) - flank, 0), int(s["end"]) + flank
        spans = (pos <= a) & (endpos > b)
        span = int(spans.sum())
        x, ln, rd = _base_items(pl, chrom - 1, merge_gap, merge_min)[ty]
        m = (x >= x_lo) & (x <= min(x_hi, SAT - 1)) & (ln >= len_lo) & (ln <= len_hi)
        alt_all, alt_r = int(m.sum()), int(spans[rd[m]].sum())
        alt_j = 0
        if chrom - 1 in jit and len(jit[chrom - 1][ty][0]):
            jx, jl, lo, hi = jit[chrom - 1][ty]
            jm = (jx >= x_lo) & (jx <= min(x_hi, SAT - 1)) & (jl >= len_lo) & (jl <= len_hi)
            alt_all += int(jm.sum())
            alt_j = int((jm & (lo <= a) & (hi > b)).sum())
        alt = alt_r + alt_j
        ref = max(span - alt_r, 0)
        gt, gq, p = genotype_ref.likelihood(alt, ref, *costs)
        out[k] = (alt, ref, span, alt_all, gt, gq, p, 0)
    return out


def _clip_len(ops) -> int:
    """What a clip standing for `ops` is long: their M I S H = X."""
    return sum(ln for op, ln in ops if op in Q_OPS or op in CLIP_OPS)


def cuttable(ops, j: int) -> bool:
    """Can the read be cut at op j: a D or an I with an aligned base (M = X) on either side?"""
    return ops[j][0] in (1, 2) and any(o in (0, 7, 8) for o, _ in ops[:j]) and any(o in (0, 7, 8) for o, _ in ops[j + 1:])


def cut(pl, which):
    """(pileup, table, index) with every read r of which = [(r, j), ...] (at most one entry a read) replaced by
    two records cut at its op j, a D or an I: the left record keeps the ops before the op plus a trailing S over
    everything after it (the inserted bases of an I included), the right record starts behind the op with a
    leading S over everything before it.  Both carry the strand of r; the CIGARs are in reference orientation,
    so on the reverse strand the right record is the query-first one (cl and ct swap roles).  Each record's SA
    entry names the other.  index[r] is the new read index of an uncut read r (-1 for a cut one)."""
    at = {int(r): int(j) for r, j in which}
    recs = []   # (tid, pos, ops, flag, old read or -1, partner key or None)
    for r in range(pl.n_reads):
        tid, pos, fl = contig_of(pl, r), int(pl.pos[r]), int(pl.flag[r]) if pl.flag is not None else 0
        ops = parse_cigar(pl.read_cigar(r))
        if r not in at:
            recs.append((tid, pos, ops, fl, r, None))
            continue
        j = at[r]
        op, ln = ops[j]
        assert op in (1, 2), "cut at a D or an I op"
        pre, post = ops[:j], ops[j + 1:]
        assert cuttable(ops, j), "both records need an aligned base"
        ins = ln if op == 1 else 0
        left = pre + [(4, ins + _clip_len(post))]
        right = [(4, _clip_len(pre) + ins)] + post
        rpos = pos + sum(n for o, n in pre if o in R_OPS) + (ln if op == 2 else 0)
        recs.append((tid, pos, left, fl, -1, (r, 1)))
        recs.append((tid, rpos, right, fl | 0x800, -1, (r, 0)))
    order = sorted(range(len(recs)), key=lambda i: (recs[i][0], recs[i][1]))   # (stable)
    tid_off = np.zeros(pl.n_targets + 1, dtype=np.int64)
    pos_l, end_l, off_l, cig_l, flag_l = [], [], [0], [], []
    index = np.full(pl.n_reads, -1, dtype=np.int64)
    where = {}
    for new, i in enumerate(order):
        tid, pos, ops, fl, old, partner = recs[i]
        words = np.array([(n << 4) | o for o, n in ops], dtype=np.uint32)
        tid_off[tid + 1] += 1
        pos_l.append(pos)
        end_l.append(endpos_of(pos, words))
        cig_l.extend(int(w) for w in words)
        off_l.append(len(cig_l))
        flag_l.append(fl)
        if old >= 0:
            index[old] = new
        else:
            where[(partner[0], 1 - partner[1])] = new   # this record's own key: (read, 0 left / 1 right)
    out = Pileup(tid_off=np.cumsum(tid_off), pos=np.array(pos_l, dtype=np.int32), endpos=np.array(end_l, dtype=np.int32),
                 cig_off=np.array(off_l, dtype=np.uint64), cigar=np.array(cig_l, dtype=np.uint32),
                 flag=np.array(flag_l, dtype=np.uint16))
    sa = {}
    for (r, side), new in where.items():
        other = where[(r, 1 - side)]
        sa[new] = [(contig_of(out, other), int(out.pos[other]) + 1, "-" if strand_of(out, other) else "+", out.read_cigar(other))]
    return out, segments(out, sa), index
