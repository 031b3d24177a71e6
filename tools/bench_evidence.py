"""Per-breakpoint evidence (include/svtrek_evidence.h) throughput on a BASELINE workload.

Times svt_evidence_device over every locus of the workload (device arrays in and out, HIP
events on one stream, the median of --repeat calls after a warm-up) next to the same
session's svt_refine_device, and prices the call's algorithmic bytes on the host: per
breakpoint with a refined value the two 4-B bucket offsets, 16 B per event of the 1 kb value
buckets covering [R - ci, R + ci], the region query's words (four 8-B bucket words + 4 B per
pos[] / emax[] entry its two searches read) and 4 B per endpos read for the depth; per
breakpoint 16 B of locus, 4 B of refined value in and 16 B of record out.  Prints one JSON line.

    python tools/bench_evidence.py [--workload cfg4_1m_delins_30x_hifi] [--repeat 20]
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

from svtrek_amd import EVIDENCE_DTYPE, RESULT_DTYPE, SVT_NA, Engine, Params, sim, version  # noqa: E402

BKS, BKT_SHIFT = 10, 12   # value buckets of 1 kb, read-start buckets of 4 kb (svt_engine.hip)


def algorithmic_bytes(pl, loci, refined, prm: Params) -> dict:
    """Host model of what one svt_evidence_device call has to read (see the module docstring)."""
    ci = max(prm.consensus_interval, 0)
    n = len(loci)
    R = np.stack([refined["start"], refined["end"]], axis=1).astype(np.int64)
    ok = R != SVT_NA
    tid = loci["chrom"].astype(np.int64) - 1
    # which event array a breakpoint reads: 0 S (DEL start), 1 E (DEL end), 2 I (INS)
    arr = np.where(loci["type"][:, None] == 1, 2, np.array([0, 1])[None, :])
    ev_total = probe = depth_reads = 0
    for t in range(pl.n_targets):
        a, b = int(pl.tid_off[t]), int(pl.tid_off[t + 1])
        sel = ok & (tid == t)[:, None]
        if a == b or not sel.any():
            continue
        pos, endpos = pl.pos[a:b].astype(np.int64), pl.endpos[a:b].astype(np.int64)
        o0, o1 = int(pl.cig_off[a]), int(pl.cig_off[b])
        words = pl.cigar[o0:o1]
        op, ln = (words & 15).astype(np.uint8), (words >> 4).astype(np.int64)
        nops = np.diff(pl.cig_off[a:b + 1].astype(np.int64))
        first = pl.cig_off[a:b].astype(np.int64) - o0
        adv = np.where((op == 1) | (op == 4), 0, ln)
        csum = np.cumsum(adv)
        base = np.where(first > 0, csum[np.maximum(first, 1) - 1], 0)           # advance before each read
        read_of = np.repeat(np.arange(b - a), nops)
        before = pos[read_of] + (csum - adv) - base[read_of]
        has = nops > 0
        last = first + nops - 1
        wend = pos.copy()
        wend[has] = pos[has] + csum[last[has]] - base[has]
        if pl.clip is not None:
            clip = pl.clip[a:b]
        else:
            clip = np.zeros(b - a, dtype=np.uint8)
            clip[has] = (op[last[has]] == 4) * 1 + (op[first[has]] == 4) * 2
        d, i = (op == 2) & (ln > 50), (op == 1) & (ln >= 50)
        vals = [np.concatenate([before[d], wend[(clip & 1) != 0]]),                   # S
                np.concatenate([before[d] + ln[d] + 1, wend[(clip & 2) != 0] + 1]),   # E
                before[i]]                                                            # I
        nb = int(max(int(endpos.max()), max((int(v.max()) for v in vals if len(v)), default=0)) >> BKS) + 2
        emax = np.maximum.accumulate(endpos)
        for A in range(3):
            m = sel & (arr == A)
            if not m.any():
                continue
            cnt = np.bincount(np.minimum(vals[A] >> BKS, nb - 1), minlength=nb)
            pre = np.concatenate([[0], np.cumsum(cnt)])
            r = R[m]
            b0 = np.minimum(np.maximum(r - ci, 0) >> BKS, nb - 1)
            b1 = np.minimum((r + ci) >> BKS, nb - 1)
            ev_total += int((pre[b1 + 1] - pre[b0]).sum())
        r = R[sel]
        # the one-base query [R, R + 1): hi = first pos >= R + 1 from its 4 kb bucket's start,
        # lo = first emax > R from the first emax >= the bucket's start
        h = np.searchsorted(pos, r + 1, side="left")
        hl = np.searchsorted(pos, ((r + 1) >> BKT_SHIFT) << BKT_SHIFT, side="left")
        lo = np.searchsorted(emax, r, side="right")
        ll = np.searchsorted(emax, (r >> BKT_SHIFT) << BKT_SHIFT, side="left")
        probe += int((h - hl + 1).sum() + (lo - ll + 1).sum())
        depth_reads += int(np.maximum(h - lo, 0).sum())
    nref = int(ok.sum())
    total = 2 * n * (16 + 4 + 16) + nref * (8 + 32) + 16 * ev_total + 4 * probe + 4 * depth_reads
    return {"refined_breakpoints": nref, "bucket_events": ev_total, "probe_entries": probe, "depth_reads": depth_reads,
            "bytes": total}


def main() -> None:
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg4_1m_delins_30x_hifi")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--alg-max-ops", type=int, default=1_000_000_000,
                    help="skip the host model of the algorithmic bytes for pileups with more CIGAR ops")
    a = ap.parse_args()

    cfg = sim.WORKLOADS[a.workload]
    t0 = time.perf_counter()
    r = sim.generate(cfg)
    t_gen = time.perf_counter() - t0
    prm = Params()
    eng = Engine(prm, device=0)
    eng.load_pileup(r.pileup)
    n = len(r.loci)
    d_loci = torch.from_numpy(r.loci.view(np.uint8).copy()).cuda()
    d_ref = torch.zeros(n * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(2 * n * EVIDENCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def timed(fn) -> list[float]:
        for _ in range(a.warmup):
            fn()
        eng.sync(s.cuda_stream)
        ms = []
        for _ in range(a.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        eng.sync(s.cuda_stream)
        return ms

    refine_ms = timed(lambda: eng.refine_device(d_loci.data_ptr(), n, d_ref.data_ptr(), s.cuda_stream))
    evid_ms = timed(lambda: eng.evidence_device(d_loci.data_ptr(), d_ref.data_ptr(), n, d_out.data_ptr(), s.cuda_stream))
    refined = d_ref.cpu().numpy().view(RESULT_DTYPE)
    ev = d_out.cpu().numpy().view(EVIDENCE_DTYPE).reshape(n, 2)
    t0 = time.perf_counter()
    n_ops = int(r.pileup.cig_off[-1])
    if n_ops <= a.alg_max_ops:
        alg = algorithmic_bytes(r.pileup, r.loci, refined, prm)
    else:   # the host model walks every CIGAR op in numpy: minutes and tens of GB past ~1 G ops
        alg = {"bytes": None, "not_computed": f"{n_ops} CIGAR ops > --alg-max-ops {a.alg_max_ops}"}
    t_alg = time.perf_counter() - t0
    R = np.stack([refined["start"], refined["end"]], axis=1)
    ok = R != SVT_NA
    med = float(np.median(evid_ms))
    print(json.dumps({
        "metric": "evidence breakpoints/sec (svt_evidence_device, 1 GPU)",
        "value": round(2 * n / (med * 1e-3), 1), "unit": "breakpoints/s",
        "workload": a.workload, "loci": n, "breakpoints": 2 * n, "refined_breakpoints": int(ok.sum()),
        "ms_per_call": round(med, 4), "ms_all": [round(x, 4) for x in evid_ms],
        "refine_ms_per_call": round(float(np.median(refine_ms)), 4), "refine_ms_all": [round(x, 4) for x in refine_ms],
        "timing": f"HIP events around one call on one stream, median of {a.repeat} after {a.warmup} warm-up calls; "
                  "refine = svt_refine_device alone (no index rebuild)",
        "alg_bytes_per_call": alg["bytes"],
        "alg_gbs": round(alg["bytes"] / (med * 1e-3) / 1e9, 1) if alg["bytes"] else None, "alg": alg,
        "support_mean": round(float(ev["support"][ok].mean()), 2) if ok.any() else None,
        "depth_mean": round(float(ev["depth"][ok].mean()), 2) if ok.any() else None,
        "setup_s": {"generate": round(t_gen, 2), "alg_bytes_model": round(t_alg, 2)}, "engine_version": version(),
    }))
    eng.close()


if __name__ == "__main__":
    main()
