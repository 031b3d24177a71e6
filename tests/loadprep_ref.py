"""A numpy model of the load's host pass (svtrek_amd/csrc/svt_loadprep.h): what prep() and stream_prep() must
give, written from their contract, not from their loops.  A rejection raises Rejected(message)."""
import numpy as np


class Rejected(Exception):
    pass


# the engine's constants (svt_engine.hip / svt_index.inc), in the order tests/native/loadprep_shim.cpp takes them
LIMITS = dict(bkt_shift=12, ncig_mask=0x1FFFFFFF, op_soft=4, wave=64, rcap=128, t_min=2048, t_max=65536,
              ix_ranges=32768, group_ops=1 << 27, threads=16)


def _first(mask):
    k = np.flatnonzero(mask)
    return int(k[0]) if len(k) else None


def prep(lim, tid_off, pos, endpos, nc, soff):
    nt = len(tid_off) - 1 if len(tid_off) else 0
    nr = int(tid_off[nt]) if nt else 0
    nstream = int(soff[nr]) if nr > 0 else 0
    pos64, end64 = pos.astype(np.int64), endpos.astype(np.int64)
    emax = np.zeros(nr, np.int32)
    bkt, bkt_off, vtop, part = [], [0], [], []
    T = min(max(nstream // lim["ix_ranges"], lim["t_min"]), lim["t_max"])
    for t in range(nt):
        r0, r1 = int(tid_off[t]), int(tid_off[t + 1])
        p, e = pos64[r0:r1], end64[r0:r1]
        s0, s1 = soff[r0:r1].astype(object), soff[r0 + 1:r1 + 1].astype(object)
        n = (nc[r0:r1] & np.uint32(lim["ncig_mask"])).astype(object)
        checks = [  # per read, in the order the pass tests them
            ("reads not sorted by pos within a contig", np.r_[False, p[1:] < p[:-1]]),
            ("pos < 0 or endpos <= pos", (p < 0) | (e <= p)),
            ("bad cig_off", np.array([b < a or b > nstream or b - a != max(k, 1) for a, b, k in zip(s0, s1, n)], bool)),
        ]
        hits = [(k, i, m) for i, (m, bad) in enumerate(checks) if (k := _first(bad)) is not None]
        if hits:
            raise Rejected(min(hits)[2])
        emax[r0:r1] = np.maximum.accumulate(endpos[r0:r1]) if r1 > r0 else []
        top = int(max(p.max(), e.max())) if r1 > r0 else 0
        vtop.append(top)
        edges = np.arange((top >> lim["bkt_shift"]) + 2, dtype=np.int64) << lim["bkt_shift"]
        bkt.append(np.stack([np.searchsorted(p, edges, "left"), np.searchsorted(emax[r0:r1].astype(np.int64), edges, "left")], 1))
        bkt_off.append(bkt_off[-1] + len(edges))
        r = r0
        while r < r1:   # a range ends at the first read that starts T ops or rcap reads after its first, or at the contig's end
            part.append(r)
            by_ops = int(np.searchsorted(soff[:nr + 1], np.uint64(int(soff[r]) + T), "left"))
            r = min(r1, r + lim["rcap"], max(by_ops, r + 1))
    part.append(nr)
    if len(part) - 1 > 0x7FFFFFFF:
        raise Rejected("too many index ranges")
    W = lim["wave"]
    n_groups = (nr + W - 1) // W
    if any(int(soff[min(g + W, nr)]) - int(soff[g]) >= lim["group_ops"] for g in range(0, nr, W)):
        n_groups = 0
    rec = np.zeros((nr, 4), np.uint32)
    if nr:
        rec[:, 0], rec[:, 1], rec[:, 2] = pos.astype(np.uint32), endpos.astype(np.uint32), nc
        rec[:, 3] = np.repeat(np.arange(nt, dtype=np.uint32), np.diff(tid_off))
    clip8 = np.zeros(max(nr, 1), np.uint8)
    clip8[:nr] = nc >> np.uint32(30)
    return dict(emax=emax, rec=rec, clip8=clip8,
                bkt=(np.concatenate(bkt) if bkt else np.zeros((0, 2))).astype(np.uint32).reshape(-1, 2),
                bkt_off=np.array(bkt_off, np.int64), part=np.array(part, np.uint64), vtop=np.array(vtop, np.int64),
                n_ranges=len(part) - 1, n_groups=n_groups)


def stream_prep(lim, tid_off, pos, endpos, cig_off, cigar, clip):
    """-> nc, soff, words, nops.  tid_off may be None only with no contigs; the other arrays may be None."""
    nt = len(tid_off) - 1 if tid_off is not None and len(tid_off) else 0
    nr = int(tid_off[nt]) if nt else 0
    if nt and tid_off[0] != 0:
        raise Rejected("tid_off[0] != 0")
    if nt and (np.diff(tid_off) < 0).any():
        raise Rejected("tid_off not monotone")
    if nr > 0 and (pos is None or endpos is None or cig_off is None or (cigar is None and cig_off[nr] > 0)):
        raise Rejected("missing arrays")
    nops = int(cig_off[nr]) if nr > 0 else 0
    if nr > 0 and cig_off[0] != 0:
        raise Rejected("cig_off[0] != 0")
    o = [int(v) for v in cig_off[:nr + 1]] if nr else [0]
    if any(b < a or b > nops or b - a > lim["ncig_mask"] for a, b in zip(o[:-1], o[1:])):
        raise Rejected("bad cig_off")
    nc = np.zeros(nr, np.uint32)
    soff, words = [0], []
    for r in range(nr):
        w = cigar[o[r]:o[r + 1]]
        if clip is not None:
            c = int(clip[r]) & 3
        else:
            c = 0 if len(w) == 0 else int((w[-1] & 0xF) == lim["op_soft"]) | int((w[0] & 0xF) == lim["op_soft"]) << 1
        nc[r] = len(w) | c << 30
        words.extend(int(v) for v in w) if len(w) else words.append(0)
        soff.append(len(words))
    return nc, np.array(soff if nr else [], np.uint64), np.array(words, np.uint32), nops
