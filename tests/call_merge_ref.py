"""Numpy model of include/svtrek_call.h with svt_call_params.merge_gap / merge_min (a helper, not a
test), from the pileup's columns alone: it knows nothing of the engine's merged index.

    walk position  x = the read's pos plus the lengths of every earlier op except I and S, in int64,
                   unsaturated
    fragment       a D (type DEL) / I (type INS) op with len >= m; tail = x + len (DEL), x (INS)
    join           fragment j+1 of a read and type joins fragment j iff x[j+1] - tail[j] <= G
    run            a maximal chain of joined fragments
    merged item    a run with L = sum len > 50 (DEL) / >= 50 (INS): (min(first x, 2^30), min(L, 2^28 - 1))

Everything downstream is call_ref's / call_split_ref's / genotype_ref's own code, run with the merged
items in place of their `items` (they look it up at every call).  merge_gap = 0 is those models
themselves with every merge stat zero.  `fragment` cuts a pileup's D > 50 / I >= 50 ops into pieces
that the merge joins again, without moving anything else.
"""
from __future__ import annotations

import contextlib

import numpy as np

from svtrek_amd._lib import SVT_DEL, SVT_INS
from svtrek_amd.pileup import Pileup

import call_ref
import call_split_ref
import genotype_ref

SAT = call_ref.SAT
LEN_MAX = (1 << 28) - 1
MERGE_ZERO = {"fragments": 0, "runs": 0, "joined_items": 0, "items": 0}
OPCODE = {SVT_DEL: 2, SVT_INS: 1}


def walk(pl, tid: int):
    """(op, len, read index in the contig, x) of every op of contig tid, int64, x unsaturated."""
    a, b = int(pl.tid_off[tid]), int(pl.tid_off[tid + 1])
    o0, o1 = int(pl.cig_off[a]), int(pl.cig_off[b])
    words = pl.cigar[o0:o1].astype(np.int64)
    op, ln = words & 15, words >> 4
    nops = np.diff(pl.cig_off[a:b + 1].astype(np.int64))
    read_of = np.repeat(np.arange(b - a), nops)
    adv = np.where((op == 1) | (op == 4), 0, ln)
    before = np.cumsum(adv) - adv
    first = pl.cig_off[a:b].astype(np.int64) - o0
    base = np.zeros(b - a, dtype=np.int64)
    has = nops > 0
    base[has] = before[first[has]]
    x = pl.pos[a:b].astype(np.int64)[read_of] + before - base[read_of]
    return op, ln, read_of, x


def runs(pl, tid: int, gap: int, min_len: int):
    """{type: (first x, L, read, fragments)} of every run of contig tid, unclamped, in read order."""
    op, ln, read_of, x = walk(pl, tid)
    out = {}
    for ty, code in OPCODE.items():
        f = (op == code) & (ln >= min_len)
        xf, lf, rf = x[f], ln[f], read_of[f]
        if not len(xf):
            z = np.zeros(0, dtype=np.int64)
            out[ty] = (z, z, z, z)
            continue
        tail = xf + lf if ty == SVT_DEL else xf
        head = np.ones(len(xf), dtype=bool)
        head[1:] = (rf[1:] != rf[:-1]) | (xf[1:] - tail[:-1] > gap)
        h = np.nonzero(head)[0]
        out[ty] = (xf[h], np.add.reduceat(lf, h), rf[h], np.diff(np.concatenate([h, [len(xf)]])))
    return out


def merged_items(pl, tid: int, gap: int, min_len: int):
    """{SVT_DEL: (x, len, read), SVT_INS: (x, len, read)} of contig tid: the merged items, int64, x
    clamped to 2^30 (not dropped: the scan counts those as skipped) and len to 2^28 - 1."""
    out = {}
    for ty, (fx, L, rd, _) in runs(pl, tid, gap, min_len).items():
        it = L > 50 if ty == SVT_DEL else L >= 50
        out[ty] = (np.minimum(fx[it], SAT), np.minimum(L[it], LEN_MAX), rd[it])
    return out


def merge_stats(pl, gap: int, min_len: int) -> dict:
    """svt_call_merge_stats' counts: of both types and every contig, whatever the scan's type bits."""
    st = dict(MERGE_ZERO)
    for tid in range(pl.n_targets):
        if int(pl.tid_off[tid]) == int(pl.tid_off[tid + 1]):
            continue
        for ty, (fx, L, rd, nf) in runs(pl, tid, gap, min_len).items():
            it = L > 50 if ty == SVT_DEL else L >= 50
            st["fragments"] += int(nf.sum())
            st["runs"] += len(fx)
            st["items"] += int(it.sum())
            st["joined_items"] += int((it & (nf >= 2)).sum())
    return st


@contextlib.contextmanager
def _items_are(pl, gap: int, min_len: int):
    """call_ref.items / genotype_ref.items replaced by the merged items of pl while the block runs."""
    def call_items(p, tid):
        assert p is pl
        return {ty: (x, ln) for ty, (x, ln, _) in merged_items(pl, tid, gap, min_len).items()}

    def gt_items(p, tid):
        assert p is pl
        return {ty: (x[x < SAT], ln[x < SAT], rd[x < SAT]) for ty, (x, ln, rd) in merged_items(pl, tid, gap, min_len).items()}
    keep = call_ref.items, genotype_ref.items
    call_ref.items, genotype_ref.items = call_items, gt_items
    try:
        yield
    finally:
        call_ref.items, genotype_ref.items = keep


def call(pl, link: int = 10, min_support: int = 3, types=(SVT_DEL, SVT_INS), len_permille: int = 0, merge_gap: int = 0,
         merge_min: int = 20):
    """(CALL_DTYPE records in order, call stats, split stats, merge stats {fragments, runs, joined_items, items})."""
    if merge_gap == 0:
        return (*call_split_ref.call(pl, link, min_support, types, len_permille), dict(MERGE_ZERO))
    with _items_are(pl, merge_gap, merge_min):
        calls, st, sp = call_split_ref.call(pl, link, min_support, types, len_permille)
    return calls, st, sp, merge_stats(pl, merge_gap, merge_min)


def genotype(pl, sites, merge_gap: int, merge_min: int = 20, flank: int = 50):
    """genotype_ref.genotype against the merged items (svt_genotype_calls after a merged scan)."""
    with _items_are(pl, merge_gap, merge_min):
        return genotype_ref.genotype(pl, sites, flank)


def fragment(pl, rng: np.random.Generator, gap: int, min_len: int = 20):
    """(a copy of pl with its D > 50 / I >= 50 ops cut into 2-4 pieces of >= min_len bases, eligible ops,
    fragmented ops).  The pieces are separated by 1-10 M bases taken from the FOLLOWING op, and an op is
    cut only when that op is an M of at least sum of gaps + gap + 1 bases: pos, endpos and every other
    op's x stay, the pieces lie within 10 <= gap of each other, and the rest of the M keeps the last
    piece more than gap from whatever follows, as the whole op was.  So
    merged_items(fragment(pl)) == merged_items(pl) for this gap and min_len."""
    assert gap >= 10 and 2 * min_len <= 50
    words = pl.cigar.astype(np.int64)
    op, ln = words & 15, words >> 4
    elig = np.nonzero(((op == 2) & (ln > 50)) | ((op == 1) & (ln >= 50)))[0]
    last = np.zeros(len(words), dtype=bool)                  # the last op of its read: nothing follows
    ends = pl.cig_off[1:].astype(np.int64)
    last[ends[ends > pl.cig_off[:-1].astype(np.int64)] - 1] = True
    parts, at, cut, added_at = [], 0, 0, []
    for j in elig:
        j = int(j)
        if last[j] or op[j + 1] != 0:
            continue
        k = int(rng.integers(2, min(4, int(ln[j]) // min_len) + 1))
        gaps = [int(g) for g in rng.integers(1, 11, size=k - 1)]
        while k > 2 and sum(gaps) + gap + 1 > ln[j + 1]:
            k -= 1
            gaps.pop()
        if sum(gaps) + gap + 1 > ln[j + 1]:
            gaps = [1]
        if sum(gaps) + gap + 1 > ln[j + 1]:
            continue
        # k pieces of >= min_len summing to ln[j]: the slack spread at random
        slack = int(ln[j]) - k * min_len
        cuts = np.sort(rng.integers(0, slack + 1, size=k - 1))
        piece = np.diff(np.concatenate([[0], cuts, [slack]])) + min_len
        new = []
        for i in range(k):
            new.append(int(piece[i]) << 4 | int(op[j]))
            if i < k - 1:
                new.append(gaps[i] << 4)
        new.append((int(ln[j + 1]) - sum(gaps)) << 4)
        parts.append(pl.cigar[at:j])
        parts.append(np.array(new, dtype=np.uint32))
        at = j + 2
        cut += 1
        added_at.append((j, len(new) - 2))
    parts.append(pl.cigar[at:])
    cigar = np.concatenate(parts).astype(np.uint32)
    grow = np.zeros(len(words) + 1, dtype=np.int64)
    for j, n in added_at:
        grow[j + 1] += n
    shift = np.cumsum(grow)                                    # ops added before stream offset o
    cig_off = (pl.cig_off.astype(np.int64) + shift[pl.cig_off.astype(np.int64)]).astype(np.uint64)
    out = Pileup(tid_off=pl.tid_off.copy(), pos=pl.pos.copy(), endpos=pl.endpos.copy(), cig_off=cig_off, cigar=cigar,
                 clip=None if pl.clip is None else pl.clip.copy())
    return out, len(elig), cut
