"""Genotypes of the discovered calls (include/svtrek_genotype.h) on a BASELINE workload.

Scans the workload's pileup (svt_call_scan), then times one svt_genotype_device over the scan's
calls as sites: HIP events around the call on one stream, the median and range of --repeat calls
after --warmup.  The yardsticks come from the same process: the scan's own scan_ms and one
svt_evidence_device over the same calls as loci (their refined results computed once before).
Reports the mean alt / ref / span and the 0/0, 0/1, 1/1, no-call split.  Prints one JSON line.

    python tools/bench_genotype.py [--workload cfg4_1m_delins_30x_hifi] [--repeat 20]
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

from svtrek_amd import Engine, Params, calls_to_loci, calls_to_sites, sim, version  # noqa: E402
from svtrek_amd._lib import EVIDENCE_DTYPE, GT_DTYPE, RESULT_DTYPE  # noqa: E402


def main() -> None:
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg4_1m_delins_30x_hifi")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--flank", type=int, default=None)
    a = ap.parse_args()

    t0 = time.perf_counter()
    r = sim.generate(sim.WORKLOADS[a.workload])
    t_gen = time.perf_counter() - t0
    eng = Engine(Params(), device=0)
    eng.load_pileup(r.pileup)
    scan_ms = []
    calls = None
    for k in range(a.warmup + a.repeat):
        calls = eng.call()
        if k >= a.warmup:
            scan_ms.append(eng.call_stats()["scan_ms"])
    n = len(calls)
    d_sites = torch.from_numpy(calls_to_sites(calls).view(np.uint8).copy()).cuda()
    d_gt = torch.zeros(max(n, 1) * GT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_loci = torch.from_numpy(calls_to_loci(calls).view(np.uint8).copy()).cuda()
    d_ref = torch.zeros(max(n, 1) * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_ev = torch.zeros(2 * max(n, 1) * EVIDENCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

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

    gt_ms = timed(lambda: eng.genotype_device(d_sites.data_ptr(), n, d_gt.data_ptr(), flank=a.flank, stream=s.cuda_stream))
    eng.refine_device(d_loci.data_ptr(), n, d_ref.data_ptr(), s.cuda_stream)
    ev_ms = timed(lambda: eng.evidence_device(d_loci.data_ptr(), d_ref.data_ptr(), n, d_ev.data_ptr(), s.cuda_stream))
    gts = d_gt.cpu().numpy().view(GT_DTYPE)[:n]
    same = bool(np.array_equal(gts, eng.genotype_calls(flank=a.flank)))
    med = float(np.median(gt_ms))
    print(json.dumps({
        "metric": "svt_genotype_device ms over the scan's calls (1 GPU)", "value": round(med, 4), "unit": "ms",
        "workload": a.workload, "reads": int(r.pileup.n_reads), "calls": n,
        "genotype_ms": round(med, 4), "genotype_ms_range": [round(min(gt_ms), 4), round(max(gt_ms), 4)],
        "genotype_ms_all": [round(x, 4) for x in gt_ms], "sites_per_s": round(n / (med * 1e-3), 1) if n else None,
        "scan_ms": round(float(np.median(scan_ms)), 4), "scan_ms_range": [round(min(scan_ms), 4), round(max(scan_ms), 4)],
        "evidence_ms": round(float(np.median(ev_ms)), 4), "evidence_ms_range": [round(min(ev_ms), 4), round(max(ev_ms), 4)],
        "timing": f"genotype / evidence: HIP events around one call on one stream, median and range of {a.repeat} after "
                  f"{a.warmup} warm-up calls; scan: svt_call_stats.scan_ms of the same process, the same counts",
        "flank": 50 if a.flank is None else a.flank,
        "alt_mean": round(float(gts["alt"].mean()), 2) if n else None,
        "ref_mean": round(float(gts["ref"].mean()), 2) if n else None,
        "span_mean": round(float(gts["span"].mean()), 2) if n else None,
        "alt_all_equals_support": bool(np.array_equal(gts["alt_all"], calls["support"])),
        "genotype_calls_equal": same,
        "split": {"0/0": int((gts["gt"] == 0).sum()), "0/1": int((gts["gt"] == 1).sum()), "1/1": int((gts["gt"] == 2).sum()),
                  "no_call": int((gts["gt"] < 0).sum())},
        "setup_s": {"generate": round(t_gen, 2)}, "engine_version": version(),
    }))
    eng.close()


if __name__ == "__main__":
    main()
