"""Consensus inserted sequence of the discovered INS calls (include/svtrek_callseq.h) on a BASELINE workload.

Loads the workload's pileup and the simulator's inserted sequences (sim_insseq), scans it (svt_call_scan)
and runs svt_call_consensus over all the scan's calls in windows of --window calls (the consensus bases of a
window are n x cap bytes on both sides).  Every figure is the engine's own HIP-event time
(svt_call_consensus_stats): the item table's build (once per load: taken from a fresh load each repeat), the
support gather and the POA launches summed over the windows; the median and range of --repeat passes after
one warm-up pass (which allocates the POA slots).  Reports the reach, the items per candidate range (mean
and max), the bytes of inserted bases on the device and INS calls/s.  Prints one JSON line.

    python tools/bench_callseq.py [--workload cfg4_1m_delins_30x_hifi] [--repeat 3] [--out FILE]
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

from svtrek_amd import Engine, Params, sim, version  # noqa: E402
from svtrek_amd._lib import SVT_INS  # noqa: E402


def one_pass(eng, n: int, window: int, cap: int) -> dict:
    """svt_call_consensus over calls [0, n) in windows; the stats summed."""
    tot = {"gather_ms": 0.0, "poa_ms": 0.0, "window_items": 0, "window_max": 0, "ins_calls": 0, "deferred": 0,
           "with_consensus": 0, "fused": 0, "cons_bases": 0}
    t0 = time.perf_counter()
    for first in range(0, n, window):
        res, _ = eng.call_consensus(first, min(window, n - first), cap)
        st = eng.call_consensus_stats()
        for k in ("gather_ms", "poa_ms", "window_items", "ins_calls", "deferred"):
            tot[k] += st[k]
        tot["window_max"] = max(tot["window_max"], st["window_max"])
        tot["with_consensus"] += int((res["len"] > 0).sum())
        tot["fused"] += int(res["n_used"].sum())
        tot["cons_bases"] += int(np.maximum(res["len"], 0).sum())
        tot["table_ms"], tot["reach"], tot["items"] = st["table_ms"], st["reach"], st["items"]
    tot["wall_s"] = time.perf_counter() - t0
    return tot


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg4_1m_delins_30x_hifi")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--window", type=int, default=100000)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--err-permille", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    cfg = sim.WORKLOADS[a.workload]
    t0 = time.perf_counter()
    r = sim.generate(cfg, keep_handle=True)
    off, bases = sim.insertion_sequences(r, cfg, err_permille=a.err_permille)
    t_gen = time.perf_counter() - t0
    eng = Engine(Params(), device=0)
    passes = []
    n = n_ins_calls = 0
    scan_ms = []
    for k in range(1 + a.repeat):        # a fresh load each pass: the table is built once per load
        eng.load_pileup(r.pileup)
        eng.load_insseq(off, bases)
        calls = eng.call()
        n, n_ins_calls = len(calls), int((calls["type"] == SVT_INS).sum())
        scan_ms.append(eng.call_stats()["scan_ms"])
        p = one_pass(eng, n, a.window, a.cap)
        if k:
            passes.append(p)

    def med(key):
        v = [p[key] for p in passes]
        return round(float(np.median(v)), 4), [round(float(min(v)), 4), round(float(max(v)), 4)]
    last = passes[-1]
    poa_ms, poa_rng = med("poa_ms")
    gather_ms, gather_rng = med("gather_ms")
    table_ms, table_rng = med("table_ms")
    line = json.dumps({
        "metric": "INS calls/s of svt_call_consensus's POA launches (1 GPU)",
        "value": round(n_ins_calls / (poa_ms * 1e-3), 1) if poa_ms else None, "unit": "INS calls/s",
        "workload": a.workload, "reads": int(r.pileup.n_reads), "calls": n, "ins_calls": n_ins_calls,
        "table_ms": table_ms, "table_ms_range": table_rng, "gather_ms": gather_ms, "gather_ms_range": gather_rng,
        "poa_ms": poa_ms, "poa_ms_range": poa_rng,
        "ins_calls_per_s_gather_and_poa": round(n_ins_calls / ((poa_ms + gather_ms) * 1e-3), 1) if poa_ms else None,
        "wall_s": med("wall_s")[0], "scan_ms": round(float(np.median(scan_ms[1:])), 4),
        "timing": f"svt_call_consensus_stats (HIP events on the null stream), summed over windows of {a.window} calls; "
                  f"median and range of {a.repeat} passes, each after a fresh load, after one warm-up pass; poa_ms "
                  "includes the host's ordering of the calls and the copies of res and bases",
        "items": last["items"], "reach": last["reach"],
        "window_items_mean": round(last["window_items"] / max(last["ins_calls"], 1), 2), "window_items_max": last["window_max"],
        "insseq_device_bytes": int(off[-1]) + 8 * len(off), "insseq_bases": int(off[-1]),
        "table_device_bytes": 8 * last["items"],
        "with_consensus": last["with_consensus"], "sequences_fused": last["fused"], "consensus_bases": last["cons_bases"],
        "deferred_to_full_slots": last["deferred"], "cap": a.cap, "window": a.window,
        "setup_s": {"generate": round(t_gen, 2)}, "engine_version": version(),
    })
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
