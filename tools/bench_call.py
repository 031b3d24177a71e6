"""DEL / INS discovery (include/svtrek_call.h) on a BASELINE workload.

Times svt_call_scan (its own HIP-event time, stats.scan_ms: the median of --repeat scans after a
warm-up) next to the same process's svt_reindex, and prices the scan's algorithmic bytes: 16 B per
event of the value-bucket arrays S and I read (the items and array S's trailing-S markers), 8 B per
key of the scratch written by the sort and 8 B read back by each of the two passes over it, 48 B
per call written.  Recall and extra calls
against the simulator's truth are reported for context: a truth breakpoint counts as found when a
call of its type and contig lies within --tol bp of bp1.  Prints one JSON line.

    python tools/bench_call.py [--workload cfg4_1m_delins_30x_hifi] [--repeat 20]

--hotspot N [--hotspot-last] times the scan on a synthetic hot spot instead: N reads with one D op
each, all starting in one 1-kb bucket (700 distinct starts: the counting sort of a big bucket) or,
with --hotspot-last, spread over 650 kb of the contig's last bucket (the in-memory bitonic sort).

--len-permille N scans with svt_call_params.len_permille = N (the start clusters split by length) and
adds the split statistics; the hot spot then gives every start two alternating lengths (D 60 + k % 50
and ten times that): the regular bucket's 700 neighbouring starts are one candidate holding every
item, the last bucket's starts, 13 apart, are one with --link 13 and 50 000 candidates without.

--merge-gap N [--merge-min M] scans with svt_call_params.merge_gap = N (a read's fragmented D / I ops
joined into merged items first) and adds the merge statistics, the build of the merged index
(build_ms: --merge-builds builds, each forced by a scan at N + 1 in between) and the same process's
plain scan (plain_scan_ms) next to the merged one.

--junctions SHARE cuts that share of the workload's D > 50 / I >= 50 ops into two records plus segment-table
rows with the model's cut helper (tests/junction_ref.py; the simulator writes no SA), scans with
svt_call_params.junctions = 1 and adds the junction statistics, the build of the union index (--merge-builds
builds, each forced by reloading the table) with its algorithmic bytes -- the base events copied once (16 B read
+ 16 B written), 24 B per segment row, 16 B per junction event -- the same process's plain scan and, for scale, the merged index's build at gap 50 on the side.  The cut is
pure Python, one read at a time: --loci N shrinks the workload to N loci for it.

--rearr SHARE cuts that share of the supporting reads the same way and then rewrites each cut read's second
alignment in the segment table, per 4-kb stretch of the reference either onto the other strand (an inverted
pair) or upstream of the first by the op's length + 100 (a duplicated pair), scans with svt_call_params.rearr =
DUP | INV (include/svtrek_rearr.h) and adds the rearrangement statistics, the build of the rearrangement index
(--merge-builds builds, each forced by reloading the table) with its algorithmic bytes -- 24 B per segment row
read twice, 16 B per event written -- and the same process's plain scan next to the two-pass one.

--bnd SHARE cuts that share of the supporting reads the same way and then rewrites each cut read's second
alignment in the segment table onto the next contig (the last one's onto the first), scans with
svt_call_params.bnd = 1 (include/svtrek_bnd.h) and adds the breakend statistics, the build of the item list
(--merge-builds builds, each forced by reloading the table) with its algorithmic bytes -- 24 B per segment row
read once, 16 B per item written -- and the same process's scan without bnd next to the one with it.  The cut
limits the workload as it does for --rearr: use the same --loci.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from svtrek_amd import SVT_DEL, SVT_INS, Engine, Params, sim, version  # noqa: E402


def recall(calls: np.ndarray, loci: np.ndarray, truth: np.ndarray, tol: int) -> dict:
    out = {}
    for name, ty in (("DEL", SVT_DEL), ("INS", SVT_INS)):
        sel = loci["type"] == ty
        mine = calls[calls["type"] == ty]
        found = 0
        for chrom in np.unique(loci["chrom"][sel]):
            cp = np.sort(mine["pos"][mine["chrom"] == chrom].astype(np.int64))
            bp = truth[sel & (loci["chrom"] == chrom), 0].astype(np.int64)
            if len(cp) == 0:
                continue
            j = np.clip(np.searchsorted(cp, bp), 1, max(len(cp) - 1, 1))
            near = np.abs(cp[np.minimum(j, len(cp) - 1)] - bp)
            near = np.minimum(near, np.abs(cp[j - 1] - bp))
            found += int((near <= tol).sum())
        out[name] = {"truth": int(sel.sum()), "found": found, "calls": int(len(mine))}
    return out


def hotspot_pileup(n: int, last: bool, two_lengths: bool = False):
    """n reads at pos 499 800 with [M | H] lead, D 60 + k % 50, M 60: the D ops start at 500 000 + k % 700
    (one regular bucket) or, behind an H op that endpos does not count, at 2 499 800 + 13 * (k % 50 000)."""
    from svtrek_amd import Pileup
    k = np.arange(n, dtype=np.int64)
    lead = 2_000_000 + 13 * (k % 50_000) if last else 200 + k % 700
    dlen = 60 + k % 50
    if two_lengths:   # the visits of one start alternate (700, 50 000 and 50 are even)
        dlen = np.where((k // (50_000 if last else 700)) % 2 == 1, 10 * dlen, dlen)
    cigar = np.stack([(lead << 4) | (5 if last else 0), (dlen << 4) | 2, np.full(n, (60 << 4) | 0)], axis=1)
    pos = np.full(n, 499_800, dtype=np.int32)
    endpos = pos + dlen + 60 + (0 if last else lead)
    return Pileup(tid_off=np.array([0, n], dtype=np.int64), pos=pos, endpos=endpos.astype(np.int32),
                  cig_off=(3 * np.arange(n + 1)).astype(np.uint64), cigar=cigar.reshape(-1).astype(np.uint32),
                  clip=np.zeros(n, dtype=np.uint8))


def hotspot(a) -> None:
    pl = hotspot_pileup(a.hotspot, a.hotspot_last, bool(a.len_permille))
    eng = Engine(Params(), device=0)
    eng.load_pileup(pl)
    ms = []
    for k in range(a.warmup + a.repeat):
        calls = eng.call(link=a.link, min_support=a.min_support, **split_kw(a))
        if k >= a.warmup:
            ms.append(eng.call_stats()["scan_ms"])
    st = eng.call_stats()
    print(json.dumps({
        "metric": "svt_call_scan ms on one hot bucket (1 GPU)", "value": round(float(np.median(ms)), 4), "unit": "ms",
        "bucket": "the contig's last (in-memory bitonic sort)" if a.hotspot_last else "regular (counting sort)",
        "items": a.hotspot, "scan_ms_all": [round(x, 4) for x in ms], "events": st["events"], "clusters": st["clusters"],
        "calls": int(len(calls)), "big_buckets": st["big_buckets"], **split_out(a, eng),
        "timing": f"svt_call_stats.scan_ms, median of {a.repeat} after {a.warmup} warm-up scans", "engine_version": version(),
    }))
    eng.close()


def split_kw(a) -> dict:
    """Engine.call's extra arguments: none without --len-permille / --merge-gap (an engine from before them runs too)."""
    kw = {"len_permille": a.len_permille} if a.len_permille else {}
    if a.merge_gap:
        kw.update(merge_gap=a.merge_gap, merge_min=a.merge_min)
    return kw


def merge_out(a, eng, r=None) -> dict:
    """The merge statistics, the build's time over --merge-builds builds and the plain scan beside it."""
    if not a.merge_gap:
        return {}
    out = {"merge_gap": a.merge_gap, "merge_min": a.merge_min, "merge_stats": eng.call_merge_stats()}
    kw = {k: v for k, v in split_kw(a).items() if k != "merge_gap"}
    build = []
    for _ in range(a.merge_builds):
        eng.call(link=a.link, min_support=a.min_support, merge_gap=a.merge_gap + 1, **kw)   # another gap: the index is dropped
        eng.call(link=a.link, min_support=a.min_support, merge_gap=a.merge_gap, **kw)
        build.append(eng.call_merge_stats()["build_ms"])
    plain = []
    kw.pop("merge_min")
    for k in range(a.warmup + a.repeat):
        eng.call(link=a.link, min_support=a.min_support, **kw)
        if k >= a.warmup:
            plain.append(eng.call_stats()["scan_ms"])
    out.update(build_ms=round(float(np.median(build)), 4), build_ms_all=[round(x, 4) for x in build],
               plain_scan_ms=round(float(np.median(plain)), 4), plain_events=eng.call_stats()["events"],
               plain_calls=eng.call_stats()["calls"])
    return out


def junction_cut(a, pl):
    """(pileup, table) with --junctions' share of the D > 50 / I >= 50 ops cut (at most one a read)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import junction_ref as J
    rng = np.random.default_rng(1)
    which = []
    for r in range(pl.n_reads):
        ops = J.parse_cigar(pl.read_cigar(r))
        cand = [j for j, (op, ln) in enumerate(ops) if ((op == 2 and ln > 50) or (op == 1 and ln >= 50)) and J.cuttable(ops, j)]
        if cand and rng.random() < a.junctions:
            which.append((r, cand[int(rng.integers(len(cand)))]))
    out, table, _ = J.cut(pl, which)
    out.clip = None
    return out, table


def junction_out(a, eng, table) -> dict:
    """The junction statistics, the union build's time over --merge-builds builds, its bytes, the plain scan beside it."""
    if not a.junctions:
        return {}
    js = eng.call_junction_stats()
    kw = split_kw(a)
    build = []
    for _ in range(a.merge_builds):
        eng.load_junctions(*table)   # the same table again: the index is dropped
        eng.call(link=a.link, min_support=a.min_support, junctions=True, **kw)
        build.append(eng.call_junction_stats()["build_ms"])
    plain = []
    for k in range(a.warmup + a.repeat):
        eng.call(link=a.link, min_support=a.min_support, **kw)
        if k >= a.warmup:
            plain.append(eng.call_stats()["scan_ms"])
    side = {}
    if not a.merge_gap:   # for scale: the merged index's build on the side (the union stays on the plain view)
        mb = []
        for _ in range(a.merge_builds):
            eng.call(link=a.link, min_support=a.min_support, merge_gap=51, merge_min=a.merge_min, **kw)   # another gap: the index is dropped
            eng.call(link=a.link, min_support=a.min_support, merge_gap=50, merge_min=a.merge_min, **kw)
            mb.append(eng.call_merge_stats()["build_ms"])
        side = {"merged_build_ms": round(float(np.median(mb)), 4), "merged_build_ms_all": [round(x, 4) for x in mb]}
    return {**side, "junctions": a.junctions, "junction_stats": js, "junction_build_ms": round(float(np.median(build)), 4),
            "junction_build_ms_all": [round(x, 4) for x in build], "plain_scan_ms": round(float(np.median(plain)), 4),
            "plain_events": eng.call_stats()["events"], "plain_calls": eng.call_stats()["calls"]}


def rearr_cut(a, pl):
    """(pileup, table) with --rearr's share of the supporting reads cut and their second alignments rewritten."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import junction_ref as J
    keep, a.junctions = a.junctions, a.rearr
    out, (read, off, seg) = junction_cut(a, pl)
    a.junctions = keep
    seg = seg.copy()
    for k in range(len(read)):
        r0, r1 = int(off[k]), int(off[k + 1])
        j = J.junction(seg[r0:r1])
        if r1 - r0 != 2 or j is None or j[0] in ("other", "none"):
            continue
        A, B, ln = seg[r0], seg[r0 + 1], int(j[3])
        if (int(j[2]) >> 12) & 1:                      # an inverted pair
            B["strand"] ^= 1
        elif int(A["strand"]) == 0:                    # a duplicated pair: Rt = B starts ln + 100 before Lf = A ends
            w = int(B["r_end"]) - int(B["r_beg"])
            B["r_beg"] = max(int(A["r_end"]) - ln - 100, 0)
            B["r_end"] = int(B["r_beg"]) + w
        else:                                          # ... on strand -: Lf = B ends ln + 100 behind the start of Rt = A
            w = int(B["r_end"]) - int(B["r_beg"])
            B["r_end"] = int(A["r_beg"]) + ln + 100
            B["r_beg"] = max(int(B["r_end"]) - w, 0)
    return out, (read, off, seg)


def rearr_out(a, eng, table) -> dict:
    """The rearrangement statistics, the index build's time over --merge-builds builds, its bytes, the plain scan beside it."""
    if not a.rearr:
        return {}
    rs = eng.call_rearr_stats()
    kw = split_kw(a)
    build = []
    for _ in range(a.merge_builds):
        eng.load_junctions(*table)   # the same table again: the index is dropped
        eng.call(link=a.link, min_support=a.min_support, rearrangements=("DUP", "INV"), **kw)
        build.append(eng.call_rearr_stats()["build_ms"])
    plain = []
    for k in range(a.warmup + a.repeat):
        eng.call(link=a.link, min_support=a.min_support, **kw)
        if k >= a.warmup:
            plain.append(eng.call_stats()["scan_ms"])
    return {"rearr": a.rearr, "rearr_stats": rs, "rearr_build_ms": round(float(np.median(build)), 4),
            "rearr_build_ms_all": [round(x, 4) for x in build],
            "rearr_build_alg_bytes": 2 * 24 * int(len(table[2])) + 16 * (rs["dup_items"] + rs["inv_items"]),
            "plain_scan_ms": round(float(np.median(plain)), 4), "plain_scan_ms_all": [round(x, 4) for x in plain],
            "plain_events": eng.call_stats()["events"], "plain_calls": eng.call_stats()["calls"]}


def bnd_cut(a, pl):
    """(pileup, table) with --bnd's share of the supporting reads cut and their second alignments moved to the next contig."""
    keep, a.junctions = a.junctions, a.bnd
    out, (read, off, seg) = junction_cut(a, pl)
    a.junctions = keep
    seg = seg.copy()
    nt = len(out.tid_off) - 1
    if nt < 2:
        raise SystemExit("--bnd needs a workload of two contigs or more")
    for k in range(len(read)):
        r0, r1 = int(off[k]), int(off[k + 1])
        if r1 - r0 == 2:
            seg[r0 + 1]["tid"] = (int(seg[r0 + 1]["tid"]) + 1) % nt
    return out, (read, off, seg)


def bnd_out(a, eng, table) -> dict:
    """The breakend statistics, the list build's time over --merge-builds builds, its bytes, the scan without bnd beside it."""
    if not a.bnd:
        return {}
    bs = eng.call_bnd_stats()
    kw = split_kw(a)
    build = []
    for _ in range(a.merge_builds):
        eng.load_junctions(*table)   # the same table again: the list is dropped
        eng.call(link=a.link, min_support=a.min_support, breakends=True, **kw)
        build.append(eng.call_bnd_stats()["build_ms"])
    plain = []
    for k in range(a.warmup + a.repeat):
        eng.call(link=a.link, min_support=a.min_support, **kw)
        if k >= a.warmup:
            plain.append(eng.call_stats()["scan_ms"])
    return {"bnd": a.bnd, "bnd_stats": bs, "bnd_build_ms": round(float(np.median(build)), 4),
            "bnd_build_ms_all": [round(x, 4) for x in build],
            "bnd_build_alg_bytes": 24 * int(len(table[2])) + 16 * bs["items"],
            "plain_scan_ms": round(float(np.median(plain)), 4), "plain_scan_ms_all": [round(x, 4) for x in plain],
            "plain_events": eng.call_stats()["events"], "plain_calls": eng.call_stats()["calls"]}


def split_out(a, eng) -> dict:
    return {"len_permille": a.len_permille, "split_stats": eng.call_split_stats()} if a.len_permille else {}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg4_1m_delins_30x_hifi")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--link", type=int, default=None)
    ap.add_argument("--min-support", type=int, default=None)
    ap.add_argument("--tol", type=int, default=10)
    ap.add_argument("--len-permille", type=int, default=0)
    ap.add_argument("--merge-gap", type=int, default=0)
    ap.add_argument("--merge-min", type=int, default=20)
    ap.add_argument("--merge-builds", type=int, default=5)
    ap.add_argument("--junctions", type=float, default=0.0)
    ap.add_argument("--rearr", type=float, default=0.0)
    ap.add_argument("--bnd", type=float, default=0.0)
    ap.add_argument("--loci", type=int, default=0)
    ap.add_argument("--hotspot", type=int, default=0)
    ap.add_argument("--hotspot-last", action="store_true")
    a = ap.parse_args()
    if a.hotspot:
        hotspot(a)
        return

    t0 = time.perf_counter()
    cfg = sim.WORKLOADS[a.workload]
    if a.loci:
        from dataclasses import replace
        cfg = replace(cfg, n_loci=a.loci)
    r = sim.generate(cfg)
    table = None
    if (a.junctions != 0) + (a.rearr != 0) + (a.bnd != 0) > 1:
        ap.error("--junctions, --rearr and --bnd each cut the workload: one at a time")
    if a.junctions:
        r.pileup, table = junction_cut(a, r.pileup)
    if a.rearr:
        r.pileup, table = rearr_cut(a, r.pileup)
    if a.bnd:
        r.pileup, table = bnd_cut(a, r.pileup)
    t_gen = time.perf_counter() - t0
    eng = Engine(Params(), device=0)
    eng.load_pileup(r.pileup)
    if table is not None:
        eng.load_junctions(*table)
    import torch
    s = torch.cuda.Stream()

    reindex_ms = []
    for k in range(a.warmup + a.repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        eng.reindex(s.cuda_stream)
        e1.record(s)
        e1.synchronize()
        if k >= a.warmup:
            reindex_ms.append(e0.elapsed_time(e1))
    scan_ms, wall_ms = [], []
    calls = None
    for k in range(a.warmup + a.repeat):
        t0 = time.perf_counter()
        calls = eng.call(link=a.link, min_support=a.min_support, **split_kw(a), **({"junctions": True} if a.junctions else {}),
                         **({"rearrangements": ("DUP", "INV")} if a.rearr else {}), **({"breakends": True} if a.bnd else {}))
        t1 = time.perf_counter()
        if k >= a.warmup:
            scan_ms.append(eng.call_stats()["scan_ms"])
            wall_ms.append((t1 - t0) * 1e3)
    st = eng.call_stats()
    med = float(np.median(scan_ms))
    # the events the scan reads: the items (D > 50 of array S, I >= 50 of array I) and the trailing-S
    # markers array S also holds, one per read whose CIGAR ends in S
    pl = r.pileup
    if pl.clip is not None:
        markers = int((pl.clip & 1).astype(bool).sum())
    else:
        nops = np.diff(pl.cig_off.astype(np.int64))
        last = pl.cig_off[1:].astype(np.int64)[nops > 0] - 1
        markers = int(((pl.cigar[last] & 15) == 4).sum())
    keys = st["events"] + (0 if a.merge_gap else markers)   # (the merged index holds items alone)
    if a.bnd:   # (the breakend items are no events of the buckets: the scan's bytes below are its passes over the buckets alone)
        keys -= eng.call_bnd_stats()["items"]
    jout = junction_out(a, eng, table)
    if jout:   # the union's build: the base events copied once, the table's rows read, the junction events written
        js = jout["junction_stats"]
        base = keys - js["del_items"] - js["ins_items"]
        jout["junction_build_alg_bytes"] = 32 * base + 24 * js["segments"] + 16 * (js["del_items"] + js["ins_items"])
    rout = {**rearr_out(a, eng, table), **bnd_out(a, eng, table)}
    alg = 16 * keys + 8 * keys + 2 * 8 * keys + 48 * st["calls"] + (48 * st["calls"] if a.rearr else 0)   # (the merge of the two lists)
    print(json.dumps({
        "metric": "svt_call_scan ms (1 GPU)", "value": round(med, 4), "unit": "ms",
        "workload": a.workload, "reads": int(r.pileup.n_reads), "cigar_ops": int(r.pileup.cig_off[-1]),
        "scan_ms": round(med, 4), "scan_ms_all": [round(x, 4) for x in scan_ms],
        "call_wall_ms": round(float(np.median(wall_ms)), 3),
        "reindex_ms": round(float(np.median(reindex_ms)), 4), "reindex_ms_all": [round(x, 4) for x in reindex_ms],
        "timing": f"scan: svt_call_stats.scan_ms (HIP events around the whole scan), median of "
                  f"{a.repeat} after {a.warmup} warm-up scans; call_wall: Engine.call with the fetch; reindex: HIP events "
                  "around svt_reindex on one stream",
        "events": st["events"], "skipped": st["skipped"], "clusters": st["clusters"], "calls": st["calls"],
        "big_buckets": st["big_buckets"], **split_out(a, eng), **merge_out(a, eng), **jout, **rout, "events_read": keys,
        "alg_bytes_per_scan": alg, "alg_gbs": round(alg / (med * 1e-3) / 1e9, 2),
        "alg": "per event of arrays S and I (items + trailing-S markers): 16 B read + 8 B key written + 2 x 8 B key read; "
               "48 B per call",
        "truth": recall(calls, r.loci, r.truth, a.tol), "tol": a.tol,
        "setup_s": {"generate": round(t_gen, 2)}, "engine_version": version(),
    }))
    eng.close()


if __name__ == "__main__":
    main()
