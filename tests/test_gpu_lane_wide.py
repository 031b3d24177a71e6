"""refine_lane_kernel at 64 windows per wave (one window per lane on all 64 lanes of phase 2):
bit-exact against the oracle at the window counts, band sizes, lane positions and paths where a
wave's upper half can go wrong.  Every engine comes from the default engine_factory(), which
forces the lane kernel at these small sizes.

Window g < n is locus g's first window, window n + i locus i's second; wave j of the launch takes
windows 64 j .. 64 j + 63, window g in lane g % 64.  The inputs are built so that the intended
band sizes sit in the intended lanes, and each test first checks that they do with the reference
walk's Python model (tests/evidence_ref.py) -- a test must not pass by missing its case.
"""
import numpy as np
import oracle_ffi as O
import pytest
import torch

from svtrek_amd import Params, make_loci
from svtrek_amd._lib import RESULT_DTYPE
from svtrek_amd.pileup import from_reads

from evidence_ref import K_END, K_INS, K_START, Model, windows
from fuzz import random_loci, random_pileup

pytestmark = pytest.mark.gpu

T_INS, T_DEL, T_INV = 1, 2, 3
# locus i sits at BASE + i * STEP (one 1 kb value bucket holds its whole band: pos = 512 mod 1024,
# band half-width 505) and a DEL ends DEL_LEN later, so no window sees another's events
BASE, STEP, DEL_LEN = 1024 * 100 + 512, 1024 * 60, 1024 * 20
BW = 505   # range + ci of the default parameters


def _pos(i):
    return BASE + i * STEP


def _reads_for(kind, values):
    """One read per candidate value of a window of this kind (an 80-base I, or a 200-base D that
    starts at the value -- refine_start -- or ends just before it -- refine_end)."""
    rows = []
    for v in values:
        if kind == K_INS:
            rows.append((0, v - 1000, [(0, 1000), (1, 80), (0, 3000)]))
        elif kind == K_START:
            rows.append((0, v - 1000, [(0, 1000), (2, 200), (0, 3000)]))
        else:
            rows.append((0, v - 201 - 1000, [(0, 1000), (2, 200), (0, 3000)]))
    return rows


def _build(spec):
    """spec[i] = (type, first-window candidate offsets from pos, second-window offsets from end)
    -> pileup, loci."""
    rows, loci = [], []
    for i, (t, first, second) in enumerate(spec):
        pos, end = _pos(i), _pos(i) + DEL_LEN
        loci.append((t, 1, pos, end))
        if t == T_INS:
            rows += _reads_for(K_INS, [pos + d for d in first])
        elif t == T_DEL:
            rows += _reads_for(K_START, [pos + d for d in first])
            rows += _reads_for(K_END, [end + d for d in second])
    return from_reads(1, rows, clip={}), make_loci(loci)


def _bands(pl, loci, prm=None):
    """Per window g (first windows, then second): band members, or -1 for no window."""
    p = prm or Params()
    tup = (p.wider_interval, p.median_interval, p.narrow_interval, p.consensus_interval_range, p.consensus_interval,
           p.consensus_min_count)
    bw = p.consensus_interval_range + max(p.consensus_interval, 0)
    n = len(loci)
    out = np.full(2 * n, -1, dtype=np.int64)
    m = Model(pl)
    for i, l in enumerate(loci):
        for k, kind, s, e, imp in windows(l, tup):
            c = m.candidates(kind, int(l["chrom"]), s, e)
            out[k * n + i] = sum(1 for v in c if imp - bw < v < imp + bw)
    return out


def _same(got, want):
    bad = np.nonzero((got["start"] != want["start"]) | (got["end"] != want["end"]))[0]
    assert len(bad) == 0, f"{len(bad)} loci differ; first #{bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


def _cluster(m, rng=None):
    """m offsets within +-3 of the breakpoint: one cluster, all band members."""
    return [(j % 7) - 3 for j in range(m)]


@pytest.mark.parametrize("nwin", [2, 62, 64, 66, 126, 128, 130, 254, 256, 258, 510, 512, 514])
def test_window_count_edges(engine_factory, nwin):
    """A single short wave, the tail wave and the workgroup tail (4 waves x 64 windows): DEL, INS and
    INV loci mixed so that lanes without a window fall in both halves of a wave."""
    n = nwin // 2
    rng = np.random.default_rng(nwin)
    spec = []
    for i in range(n):
        t = int(rng.choice([T_DEL, T_DEL, T_INS, T_INS, T_INV]))
        spec.append((t, _cluster(int(rng.integers(0, 13))), _cluster(int(rng.integers(0, 13)))))
    pl, loci = _build(spec)
    none = np.array([s[0] == T_INV for s in spec] + [s[0] != T_DEL for s in spec])
    lane = np.arange(2 * n) % 64
    if nwin >= 64:
        assert none[lane < 32].any() and none[lane >= 32].any()
        assert (~none)[lane < 32].any() and (~none)[lane >= 32].any()
    eng = engine_factory()
    eng.load_pileup(pl)
    _same(eng.refine(loci), O.refine_batch(pl, loci))


SIZES = [0, 2, 3, 8, 9, 16, 17, 32, 33]   # min_count 3: 2 is NA, 33 is left over to refine_redo_kernel
LANES = [0, 31, 32, 33, 63]


def test_band_size_edges_in_the_upper_half(engine_factory):
    """Waves 0-8: lanes 0, 31, 32, 33 and 63 carry the nine band sizes, rotated by one per wave (every
    size in every one of the five lanes once), the other lanes bands of 0-8.  Wave 9: bands <= 8 but
    for 20 members in lane 63; wave 10: 12 members in lane 63 -- the wave's sort network is picked by
    lane 63 alone.  Both window kinds of the first-window half (DEL starts and INS) take part."""
    rng = np.random.default_rng(5)
    want_band = {}
    spec = []
    for wave in range(11):
        for ln in range(64):
            i = wave * 64 + ln
            m = int(rng.integers(0, 9))
            if wave < 9 and ln in LANES:
                m = SIZES[(LANES.index(ln) + wave) % 9]
                want_band[i] = m
            elif ln == 63:
                m = want_band[i] = 20 if wave == 9 else 12
            spec.append((T_DEL if (i + wave) % 2 else T_INS, _cluster(m), []))
    pl, loci = _build(spec)
    n = len(loci)
    bands = _bands(pl, loci)
    for i, m in want_band.items():
        assert bands[i] == m, (i, m, bands[i])
    for size in SIZES:   # every size at a lane >= 32
        assert any(m == size and i % 64 >= 32 for i, m in want_band.items())
    for wave, top in ((9, 20), (10, 12)):
        first = bands[wave * 64: wave * 64 + 64]
        assert first[63] == top and first[:63].max() <= 8
    assert (bands[n:] <= 0).all()   # the DEL ends see nothing
    eng = engine_factory()
    eng.load_pileup(pl)
    _same(eng.refine(loci), O.refine_batch(pl, loci))


def test_above_walks_from_upper_lanes(engine_factory):
    """min_count 1; windows whose candidates all lie at or above pos - 25, three at pos - 25 and one at
    pos - 21: the vote's pass above pos - 25 runs from the last band member (and its lone pos - 21 then
    wins over the cluster's mean) only when no candidate lies at or above the band's high end.  Every
    second such window has one, 1 300-1 800 bases up -- beyond the band's bucket, so only the ABOVE
    walk (bk_above) sees it.  All of them sit in lanes >= 32, between ordinary windows."""
    prm = Params(consensus_min_count=1)
    rng = np.random.default_rng(9)
    spec, probe = [], []
    for i in range(3 * 64):
        t = T_DEL if i % 3 else T_INS
        if i % 64 >= 32 and i % 2 == 0:
            far = [int(rng.integers(1300, 1800))] if (i // 2) % 2 else []
            spec.append((t, [-25, -25, -25, -21] + far, []))
            probe.append((i, bool(far)))
        else:
            spec.append((t, _cluster(int(rng.integers(0, 9))), []))
    pl, loci = _build(spec)
    want = O.refine_batch(pl, loci, prm)
    # the far candidate decides the answer (so a missed or misplaced ABOVE walk shows)
    with_far = {int(want["start"][i]) - _pos(i) for i, f in probe if f}
    without = {int(want["start"][i]) - _pos(i) for i, f in probe if not f}
    assert len(with_far) == 1 and len(without) == 1 and with_far != without, (with_far, without)
    assert {i % 64 for i, f in probe if f} >= {34, 62} and all(i % 64 >= 32 for i, _ in probe)
    eng = engine_factory(prm)
    eng.load_pileup(pl)
    _same(eng.refine(loci), want)


def test_windows_walked_alone_in_upper_lanes(engine_factory):
    """Windows whose band bucket holds more than 128 events (walked alone), pairs of windows with
    65-128 (walked two at a time) and one with 40 band members among 150 events (left over), all in
    lanes >= 32 next to packed windows: their flags reach phase 2 through the walking wave's
    registers, keyed by the window's lane."""
    spec = []
    heavy = {}
    for i in range(2 * 64):
        ln = i % 64
        t = T_DEL if i < 64 else T_INS
        m = (i * 5) % 9
        extra = []
        if ln in (33, 40, 63):
            extra = [506 + (j % 5) for j in range(150)]       # in the band's bucket, above the band
            heavy[i] = 150 + m
        elif ln in (36, 37, 50, 51):
            extra = [506 + (j % 5) for j in range(90)]
            heavy[i] = 90 + m
        if ln == 45:
            m, extra = 40, [506 + (j % 5) for j in range(110)]
            heavy[i] = 150
        spec.append((t, _cluster(m) + extra, []))
    pl, loci = _build(spec)
    bands = _bands(pl, loci)
    m = Model(pl)
    for i, ev in heavy.items():
        l = loci[i]
        kind = K_START if int(l["type"]) == T_DEL else K_INS
        s, e = windows(l, (20000, 10000, 2000, 500, 5, 3))[0][2:4]
        c = m.candidates(kind, 1, s, e)
        assert len(c) == ev and bands[i] == (40 if i % 64 == 45 else (i * 5) % 9), (i, len(c), bands[i])
        assert all((_pos(i) - BW) >> 10 == v >> 10 for v in c)   # one bucket holds them all
    eng = engine_factory()
    eng.load_pileup(pl)
    _same(eng.refine(loci), O.refine_batch(pl, loci))


def test_left_overs_in_upper_lanes_direct_and_replayed(engine_factory):
    """Every left-over window (a band of more than 32 members) in a lane >= 32, some in the launch's
    tail wave: a direct launch, a captured launch replayed three times, then a direct launch again
    give the oracle's results each time -- the left-over list and its direct / captured counters are
    the 32-wide kernel's protocol (the check of test_graph_replays_between_direct_lane_launches)."""
    spec = []
    big = []
    for i in range(3 * 64 + 40):
        m = (i * 7) % 11
        if i % 64 in (32, 39, 47, 63) or i == 3 * 64 + 37:
            m = 33 + i % 5
            big.append(i)
        spec.append((T_DEL if i % 2 else T_INS, _cluster(m), _cluster((i * 3) % 8)))
    pl, loci = _build(spec)
    n = len(loci)
    bands = _bands(pl, loci)
    left = np.nonzero(bands > 32)[0]
    assert list(left) == big and all(g % 64 >= 32 for g in left)
    want = O.refine_batch(pl, loci)
    eng = engine_factory()
    eng.load_pileup(pl)
    _same(eng.refine(loci), want)
    d_loci = torch.from_numpy(loci.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(n * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.refine_device(d_loci.data_ptr(), n, d_out.data_ptr(), s.cuda_stream)
    s.synchronize()
    _same(d_out.cpu().numpy().view(RESULT_DTYPE), want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        eng.refine_device(d_loci.data_ptr(), n, d_out.data_ptr(), s.cuda_stream)
    for _ in range(3):
        d_out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same(d_out.cpu().numpy().view(RESULT_DTYPE), want)
    _same(eng.refine(loci), want)
    _same(eng.refine(loci[: n // 2]), O.refine_batch(pl, loci[: n // 2]))


@pytest.mark.parametrize("env", [None, {"SVTREK_INDEX": "lists"}, {"SVTREK_LANE_WIDE": "0"}],
                         ids=["buckets", "lists", "buckets-32-per-wave"])
@pytest.mark.parametrize("seed", range(6))
def test_fuzz_both_index_paths(engine_factory, seed, env):
    """The fuzzed pileups of test_gpu_parity at ~300 loci through the value buckets and through the
    span lists (and, for the size pick's other side, through the 32-windows-per-wave kernel)."""
    rng = np.random.default_rng(4000 + seed)
    hot = [int(x) for x in rng.integers(5000, 55000, size=6)]
    pl = random_pileup(rng, n_targets=2, contig_len=60000, n_reads=int(rng.integers(50, 700)),
                       max_ops=int(rng.choice([3, 40, 150, 400])), hot=hot)
    prm = Params(consensus_interval=int(rng.choice([5, 0, 30])), consensus_min_count=int(rng.choice([1, 2, 3])))
    eng = engine_factory(prm, env=env)
    eng.load_pileup(pl)
    loci = random_loci(rng, 300, 2, 60000, hot)
    _same(eng.refine(loci), O.refine_batch(pl, loci, prm))
