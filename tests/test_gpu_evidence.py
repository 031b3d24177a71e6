"""include/svtrek_evidence.h on the HIP engine: Engine.evidence against the Python model
(tests/evidence_ref.py, pinned to the oracle by tests/test_evidence_model.py), the bucket path
against the span-list fallback (SVTREK_INDEX=lists), the sentinel windows that must take the
per-read walk, the API's shape, and `svtrek audt --evidence`."""
import functools
import os
import subprocess

import numpy as np
import oracle_ffi as O
import pytest

from svtrek_amd import Engine, Params, SvtError, from_reads, make_loci, sim
from svtrek_amd._lib import EVIDENCE_DTYPE, SVT_ESTATE, SVT_NA

import fuzz
from evidence_ref import Model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "svtrek_amd", "svtrek")

# (wider, median, narrow, range, ci, min_count)
PARAM_SETS = {"defaults": (20000, 10000, 2000, 500, 5, 3), "sentinel": (20000, 10000, 503, 500, 5, 1),
              "band_small": (3000, 1500, 600, 300, 20, 2), "ci0": (20000, 10000, 2000, 500, 0, 1)}
# (seed, n_reads, max_ops): two short-read pileups and one that takes the long-read filing path
PILEUPS = {"s901": (901, 400, 60), "s902": (902, 400, 60), "long905": (905, 120, 600)}
NA_REC = np.array([(0, 0, SVT_NA, SVT_NA)], dtype=EVIDENCE_DTYPE)[0]


@functools.lru_cache(maxsize=None)
def fuzz_case(name):
    seed, n_reads, max_ops = PILEUPS[name]
    rng = np.random.default_rng(seed)
    hot = [int(x) for x in rng.integers(5000, 55000, size=5)]
    pl = fuzz.random_pileup(rng, n_targets=2, contig_len=60000, n_reads=n_reads, max_ops=max_ops, hot=hot)
    loci = fuzz.random_loci(rng, 300, 2, 60000, hot)
    return pl, loci, Model(pl)


@functools.lru_cache(maxsize=None)
def fuzz_expected(name, pname):
    """The oracle's refined results and the model's evidence for them: computed once per case."""
    pl, loci, model = fuzz_case(name)
    prm = PARAM_SETS[pname]
    refined = O.refine_batch(pl, loci, Params(*prm))
    return refined, model.evidence(loci, refined, prm)


def first_diff(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} records differ; first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"


def same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), first_diff(got, want)


def open_engine(prm, monkeypatch, lists=False):
    """An engine on device 0; lists: without the value buckets (SVTREK_INDEX is read at svt_open)."""
    if lists:
        monkeypatch.setenv("SVTREK_INDEX", "lists")
    return Engine(Params(*prm), device=0)


@pytest.mark.parametrize("index", ["buckets", "lists"])
@pytest.mark.parametrize("pname", list(PARAM_SETS))
@pytest.mark.parametrize("name", list(PILEUPS))
def test_fuzz_parity_with_the_model(name, pname, index, monkeypatch):
    """Engine.evidence == the model for every breakpoint (random_loci supplies windows that wrap
    in uint32 and contigs out of range), through the value buckets and through the exact
    fallback of an engine without them; the refined results are the engine's own."""
    pl, loci, _ = fuzz_case(name)
    refined, want = fuzz_expected(name, pname)
    with open_engine(PARAM_SETS[pname], monkeypatch, lists=index == "lists") as eng:
        eng.load_pileup(pl)
        assert bool(eng.load_stats()["bucket_index"]) == (index == "buckets")
        got_ref = eng.refine(loci)
        assert np.array_equal(got_ref, refined)
        got = eng.evidence(loci, got_ref)
    n_win = int((loci["type"] == 1).sum() + 2 * (loci["type"] == 2).sum())
    n_ref = int((refined["start"] != SVT_NA).sum() + (refined["end"] != SVT_NA).sum())
    assert n_ref >= 0.10 * n_win, (n_ref, n_win)   # not a comparison of all-NA records
    same(got, want)


def sentinel_pileup(tail_ops):
    reads = [(0, 19000, [(0, 699), (2, 200), (0, 700)])]
    reads += [(0, 19000, [(0, v - 19101), (2, 100), (0, 50)]) for v in (20499, 20503, 20504)]
    reads += [(0, 20400, [(4, 10)] + tail_ops)]
    return from_reads(1, reads, clip={})


@pytest.mark.parametrize("tail_ops, want_end", [
    ([(0, 106)], (4, 5, 20499, 20507)),                # the stop's value 20507 = R + ci, past e + 2 = 20505
    ([(0, 107)], (3, 5, 20499, 20504)),                # 20508: outside the radius
    ([(0, 106), (0, 500)], (4, 5, 20499, 20507)),      # the value comes after the break op, not at the walk end
], ids=["L106", "L107", "L106+500"])
@pytest.mark.parametrize("index", ["buckets", "lists"])
def test_sentinel_windows_take_the_perread_walk(tail_ops, want_end, index, monkeypatch):
    """refine_end's leading-S read whose walk breaks past e: the events hold no exact value for
    it (the vote paths use e + 2), so a window with R + ci >= e + 2 is walked read by read."""
    prm = (20000, 10000, 503, 500, 5, 3)
    pl = sentinel_pileup(tail_ops)
    loci = make_loci([(2, 1, 10000, 20000)])
    refined = O.refine_batch(pl, loci, Params(*prm))
    assert int(refined[0]["end"]) == 20502
    want = Model(pl).evidence(loci, refined, prm)
    assert tuple(want[0, 1]) == want_end
    with open_engine(prm, monkeypatch, lists=index == "lists") as eng:
        eng.load_pileup(pl)
        assert np.array_equal(eng.refine(loci), refined)
        got = eng.evidence(loci, refined)
    same(got, want)


def test_api_shape(engine_factory):
    import torch
    pl, loci, _ = fuzz_case("s901")
    refined, want = fuzz_expected("s901", "defaults")
    with Engine(Params(), device=0) as e0:   # before load_pileup
        assert e0.evidence(loci[:0], refined[:0]).shape == (0, 2)
        with pytest.raises(SvtError) as ei:
            e0.evidence(loci, refined)
        assert ei.value.code == SVT_ESTATE
    eng = engine_factory()
    eng.load_pileup(pl)
    got = eng.evidence(loci, refined)
    assert got.shape == (len(loci), 2) and got.dtype == EVIDENCE_DTYPE
    same(got, want)
    assert eng.evidence(loci[:0], refined[:0]).shape == (0, 2)
    # INV, unknown types and the second slot of an INS: the NA record
    no_win = np.ones((len(loci), 2), dtype=bool)
    no_win[loci["type"] == 2] = False
    no_win[loci["type"] == 1, 0] = False
    assert no_win.sum() > 100 and (got[no_win] == NA_REC).all()
    # device buffers on a non-default stream
    n = len(loci)
    d_loci = torch.from_numpy(loci.view(np.uint8).copy()).cuda()
    d_ref = torch.from_numpy(refined.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(2 * n * EVIDENCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.evidence_device(d_loci.data_ptr(), d_ref.data_ptr(), n, d_out.data_ptr(), s.cuda_stream)
    eng.sync(s.cuda_stream)
    same(d_out.cpu().numpy().view(EVIDENCE_DTYPE).reshape(n, 2), want)
    # after a rebuild of the index, on another stream than the rebuild's
    eng.reindex(s.cuda_stream)
    same(eng.evidence(loci, refined), want)


def test_multi_device_context_splits_evidence():
    import torch
    pl, loci, _ = fuzz_case("s902")
    refined, want = fuzz_expected("s902", "defaults")
    ndev = torch.cuda.device_count()
    devices = list(range(min(ndev, 4))) if ndev > 1 else [0, 0]
    with Engine(Params(), devices=devices) as eng:
        eng.load_pileup(pl)
        same(eng.evidence(loci, refined), want)
        k = int(np.nonzero(refined["start"] != SVT_NA)[0][0])
        same(eng.evidence(loci[k:k + 3], refined[k:k + 3]), want[k:k + 3])   # fewer loci than 4 devices
        same(eng.evidence(loci[k:k + 1], refined[k:k + 1]), want[k:k + 1])   # ... and than 2


@functools.lru_cache(maxsize=None)
def sim_workload():
    return sim.generate(sim.SimConfig(n_targets=2, n_loci=2501, coverage=20, p_clip_ends=0.2))


def test_sim_workload_invariants_and_paths(monkeypatch):
    r = sim_workload()
    prm = PARAM_SETS["defaults"]
    with Engine(Params(), device=0) as eng:
        eng.load_pileup(r.pileup)
        refined = eng.refine(r.loci)
        ev = eng.evidence(r.loci, refined)
    with open_engine(prm, monkeypatch, lists=True) as eng:
        eng.load_pileup(r.pileup)
        same(eng.evidence(r.loci, refined), ev)
    R = np.stack([refined["start"], refined["end"]], axis=1)
    ok = R != SVT_NA
    assert ok.sum() > 1000
    assert (ev["support"][ok] >= prm[5]).all()
    assert (ev["lo"][ok] <= R[ok]).all() and (R[ok] <= ev["hi"][ok]).all()
    assert (ev["hi"][ok].astype(np.int64) - ev["lo"][ok] <= 2 * prm[4]).all()
    assert (ev[~ok] == NA_REC).all()
    # 200 sampled refined breakpoints against the model (the loci they belong to)
    rows = np.unique(np.argwhere(ok)[np.random.default_rng(5).choice(int(ok.sum()), 200, replace=False), 0])
    want = Model(r.pileup).evidence(r.loci[rows], refined[rows], prm)
    same(ev[rows], want)


def run_cli(*args):
    p = subprocess.run([CLI, "audt", *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    from svtrek_amd import host
    d = tmp_path_factory.mktemp("evidence_cli")
    r = sim.generate(sim.SimConfig(n_loci=300), keep_handle=True)
    bam, vcf = str(d / "x.bam"), d / "x.vcf"
    sim.write_bam(r, bam, with_seq=False)
    sim.write_vcf(r.loci, str(vcf))
    with open(vcf, "a") as f:   # records that reach the type switch without a window, and skipped lines
        f.write("1\t30000\tinv1\tN\t<INV>\t.\tPASS\tSVTYPE=INV;END=36000\n"
                "1\t40000\tdup1\tN\t<DUP>\t.\tPASS\tSVTYPE=DUP;END=46000\n"
                "9\t50000\tnocontig\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=60000\n"
                "onlyone\n")
    text = vcf.read_text()
    loci, _ = host.parse_vcf_text(text.encode("latin-1"))
    with Engine(Params(), device=0) as eng:
        eng.load_pileup(r.pileup)
        refined = eng.refine(loci)
        table = host.format_evidence(loci, refined, eng.evidence(loci, refined))
    plain = run_cli("-b", bam, "-v", str(vcf))
    assert plain.stdout == O.audit_text(text, r.pileup)
    return d, bam, str(vcf), plain, table, len(loci)


@pytest.mark.parametrize("extra", [(), ("--gpus", "2", "--devices", "0,0"), ("--batch", "17")],
                         ids=["one_gpu", "two_shards", "batch17"])
def test_cli_evidence_table(cli_case, extra):
    """stdout and stderr are the same bytes with and without --evidence; the file has one line
    per parsed record and its columns are Engine.refine + Engine.evidence on the same loci."""
    d, bam, vcf, plain, table, n = cli_case
    out = d / ("ev_" + "_".join(extra).replace(",", "").replace("-", "") + ".tsv")
    p = run_cli("-b", bam, "-v", vcf, "--evidence", str(out), *extra)
    assert p.stdout == plain.stdout and p.stderr == plain.stderr
    got = out.read_text()
    assert got.count("\n") == n + 1 and got.startswith("#row\ttype\tchrom\t")
    assert got == table
