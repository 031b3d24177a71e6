"""Numpy model of include/svtrek_callseq.h (a helper, not a test), built on call_ref.items: it knows
nothing of the engine's item table, reach or gather.

    k             the sequence index of svt_load_insseq: the I >= 50 ops in (read, op) order
    items         of an INS call: the I >= 50 ops of contig chrom - 1 with x_lo <= x <= x_hi (x < 2^30)
                  and len_lo <= len <= len_hi
    support       the items with len <= max_len in ascending k; n_support their count, the first
                  max_support kept
    consensus     oracle_ffi.poa_consensus of the kept sequences (the first max_seqs that fit are fused)
    DEL call      {-1, 0, 0, 0}
"""
from __future__ import annotations

import numpy as np

from svtrek_amd._lib import POA_RESULT_DTYPE, SVT_INS

import call_ref

SAT = call_ref.SAT


def ins_items(pl):
    """Per contig (x, len, k, read pos) of its I >= 50 ops, int64, in (read, op) order."""
    out, k0 = [], 0
    for tid in range(pl.n_targets):
        a, b = int(pl.tid_off[tid]), int(pl.tid_off[tid + 1])
        if a == b:
            out.append(tuple(np.zeros(0, dtype=np.int64) for _ in range(4)))
            continue
        x, ln = call_ref.items(pl, tid)[SVT_INS]
        words = pl.cigar[int(pl.cig_off[a]):int(pl.cig_off[b])].astype(np.int64)
        is_i = ((words & 15) == 1) & ((words >> 4) >= 50)
        read_of = np.repeat(np.arange(a, b), np.diff(pl.cig_off[a:b + 1].astype(np.int64)))[is_i]
        out.append((x, ln, k0 + np.arange(len(x), dtype=np.int64), pl.pos[read_of].astype(np.int64)))
        k0 += len(x)
    return out


def reach(pl) -> int:
    """The largest x - read pos over the items with x < 2^30 (0: none)."""
    r = 0
    for x, _, _, pos in ins_items(pl):
        ok = x < SAT
        if ok.any():
            r = max(r, int((x[ok] - pos[ok]).max()))
    return r


def call_items(items, c) -> np.ndarray:
    """The k of an INS call's items, ascending."""
    x, ln, k, _ = items[int(c["chrom"]) - 1]
    m = (x >= int(c["x_lo"])) & (x <= int(c["x_hi"])) & (x < SAT) & (ln >= int(c["len_lo"])) & (ln <= int(c["len_hi"]))
    return k[m]


def call_support(items, c, max_len: int = 4000, max_support: int = 64):
    """(n_support, the kept k) of an INS call."""
    x, ln, k, _ = items[int(c["chrom"]) - 1]
    ks = call_items(items, c)
    k0 = int(k[0]) if len(k) else 0
    ks = ks[ln[ks - k0] <= max_len]
    return len(ks), ks[:max_support]


def consensus(pl, calls, off, bases, **poa_kw):
    """(POA_RESULT_DTYPE records, the full-length consensus of every call as a list of uint8 arrays)."""
    import oracle_ffi as O
    pp = dict(O.POA_DEFAULTS)
    pp.update(poa_kw)
    items = ins_items(pl)
    res = np.zeros(len(calls), dtype=POA_RESULT_DTYPE)
    seqs_out = []
    for j, c in enumerate(calls):
        if int(c["type"]) != SVT_INS:
            res[j] = (-1, 0, 0, 0)
            seqs_out.append(np.zeros(0, dtype=np.uint8))
            continue
        n, ks = call_support(items, c, pp["max_len"], pp["max_support"])
        want, used = O.poa_consensus([bases[int(off[k]):int(off[k + 1])] for k in ks], **poa_kw)
        res[j] = (len(want), n, used, 0)
        seqs_out.append(want)
    return res, seqs_out


def padded(seqs, cap: int) -> np.ndarray:
    """The [n, cap] bases array Engine.call_consensus returns for those consensus sequences."""
    out = np.zeros((len(seqs), cap), dtype=np.uint8)
    for j, s in enumerate(seqs):
        out[j, :min(len(s), cap)] = s[:cap]
    return out
