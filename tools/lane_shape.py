"""CPU-side shape check for refine_lane_kernel's phase 2 (no GPU): the band sizes of a workload's
windows, the share of voted windows whose pass below pos + 25 returns early, and the per-wave
maximum band size -- which picks the sort network (8 / 16 / 32) and bounds the vote's trip count --
for waves of 32 and of 64 consecutive windows.

    python tools/lane_shape.py [--workload cfg4_1m_delins_30x_hifi] [--scale 0.004]

Candidates come from the reference walk's Python model (tests/evidence_ref.py, pinned to the oracle
by tests/test_evidence_model.py); the left pass is consensus_pos's (refinement.c:56-76).
"""
import argparse
import collections
import os
import sys
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from evidence_ref import Model, windows  # noqa: E402

from svtrek_amd import Params, sim  # noqa: E402

LV_CAP = 32


def left_pass_early(band, below, pos, ci, rng, min_count):
    """Does consensus_pos's first pass (from the last element <= pos + 25 downwards) return?"""
    nb = len(band)
    l0 = sum(1 for v in band if v <= pos + 25)
    p = 0 if (not below and l0 == 0) else (l0 - 1 if l0 else -1)
    best, dist = min_count - 1, 1 << 31
    for i in range(min(p, nb - 1), -1, -1):
        a = band[i]
        if abs(pos - a) >= rng:
            break
        k = i
        while k > 0 and band[k - 1] >= a - ci:
            k -= 1
        c = i - k + 1
        if c > best:
            co = (sum(band[k:i + 1]) + c // 2) // c
            d = abs(pos - co)
            if d < ci:
                return True
            if d < dist:
                best, dist = c, d
    return False


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg4_1m_delins_30x_hifi")
    ap.add_argument("--scale", type=float, default=0.004)
    a = ap.parse_args()
    cfg = sim.WORKLOADS[a.workload]
    cfg = replace(cfg, n_loci=max(1, int(cfg.n_loci * a.scale)))
    r = sim.generate(cfg)
    p = Params()
    prm = (p.wider_interval, p.median_interval, p.narrow_interval, p.consensus_interval_range, p.consensus_interval,
           p.consensus_min_count)
    bw = prm[3] + max(prm[4], 0)
    n = len(r.loci)
    m = Model(r.pileup)
    nb = np.full(2 * n, -1, dtype=np.int64)      # -1: no window
    early = np.zeros(2 * n, dtype=bool)
    for i, l in enumerate(r.loci):
        for k, kind, s, e, imp in windows(l, prm):
            c = m.candidates(kind, int(l["chrom"]), s, e)
            band = sorted(v for v in c if imp - bw < v < imp + bw)
            nb[k * n + i] = len(band)
            if prm[5] <= len(band) <= LV_CAP:
                early[k * n + i] = left_pass_early(band, any(v <= imp - bw for v in c), imp, prm[4], prm[3], prm[5])
    voted = (nb >= prm[5]) & (nb <= LV_CAP)
    print(f"{a.workload} x {a.scale}: {n} loci, {2 * n} windows: none {int((nb < 0).sum())}, "
          f"NA (band < {prm[5]}) {int(((nb >= 0) & (nb < prm[5])).sum())}, voted {int(voted.sum())}, "
          f"left over (band > {LV_CAP}) {int((nb > LV_CAP).sum())}")
    hist = collections.Counter()
    for v in nb[voted]:
        hist["<= 8" if v <= 8 else "9-16" if v <= 16 else "17-24" if v <= 24 else "25-32"] += 1
    print("band sizes of voted windows:", {k: f"{100 * hist[k] / voted.sum():.1f} %" for k in ("<= 8", "9-16", "17-24", "25-32")},
          f"median {int(np.median(nb[voted]))}, mean {nb[voted].mean():.1f}")
    print(f"left pass returns early: {100 * early[voted].mean():.1f} % of voted windows")
    lane_nb = np.where(voted, nb, 0)
    for w in (32, 64):
        nwv = (2 * n + w - 1) // w
        mx = np.array([lane_nb[j * w:(j + 1) * w].max() for j in range(nwv)])
        live = np.array([voted[j * w:(j + 1) * w].sum() for j in range(nwv)])
        act = mx > 0
        net = {8: int(((mx > 0) & (mx <= 8)).sum()), 16: int(((mx > 8) & (mx <= 16)).sum()), 32: int((mx > 16).sum())}
        print(f"{w} windows per wave: {nwv} waves, {int(act.sum())} vote; network 8 / 16 / 32: "
              f"{net[8]} / {net[16]} / {net[32]} ({100 * net[32] / max(1, act.sum()):.1f} % in the 32-network); "
              f"mean per-wave max band {mx[act].mean():.1f}; voting lanes per voting wave {live[act].mean():.1f}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
