"""CPU side of include/svtrek_evidence.h: the Python model (tests/evidence_ref.py) pinned to the
oracle, the host formatter of `svtrek audt --evidence`, and the backends without the entry
point.  The GPU side is tests/test_gpu_evidence.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import oracle_ffi as O
import pytest

from svtrek_amd import Engine, Params, SvtError, make_loci
from svtrek_amd._lib import EVIDENCE_DTYPE, EVIDENCE_SYMBOLS, RESULT_DTYPE, SVT_NA, bind_abi, has_evidence

import fuzz
from evidence_ref import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libsvtrek_cpu.so")
CPU_CLI = os.path.join(ROOT, "oracle", "_cpu", "svtrek_cpu")

# (wider, median, narrow, range, ci, min_count): the defaults, and the set where refine_end's
# sentinel value e + 2 can fall inside the support radius (narrow + 2 < range + ci)
PARAM_SETS = [(20000, 10000, 2000, 500, 5, 3), (20000, 10000, 503, 500, 5, 1)]


def fuzz_case(seed, n_reads=400, max_ops=60):
    rng = np.random.default_rng(seed)
    hot = [int(x) for x in rng.integers(5000, 55000, size=5)]
    pl = fuzz.random_pileup(rng, n_targets=2, contig_len=60000, n_reads=n_reads, max_ops=max_ops, hot=hot)
    return pl, fuzz.random_loci(rng, 300, 2, 60000, hot)


@pytest.mark.parametrize("prm", PARAM_SETS, ids=["defaults", "sentinel"])
@pytest.mark.parametrize("seed", [901, 902])
def test_model_candidates_vote_as_the_oracle(seed, prm):
    """consensus_pos on the model's candidates == O.refine_batch for every window, and the
    invariants of the header hold on every refined breakpoint."""
    pl, loci = fuzz_case(seed)
    m = Model(pl)
    want = O.refine_batch(pl, loci, Params(*prm))
    w = np.stack([want["start"], want["end"]], axis=1)
    assert np.array_equal(m.refine(loci, prm, O.consensus_pos), w)
    ev = m.evidence(loci, want, prm)
    r = w != SVT_NA
    n_win = int((loci["type"] == 1).sum() + 2 * (loci["type"] == 2).sum())
    assert r.sum() >= 0.10 * n_win   # the inputs refine (the oracle: 18 % of the windows or more)
    assert (ev["support"][r] >= prm[5]).all()
    assert (ev["lo"][r] <= w[r]).all() and (w[r] <= ev["hi"][r]).all()
    assert (ev["hi"][r].astype(np.int64) - ev["lo"][r] <= 2 * prm[4]).all()
    na = ev[~r]
    assert (na["support"] == 0).all() and (na["depth"] == 0).all() and (na["lo"] == SVT_NA).all() and (na["hi"] == SVT_NA).all()


def test_format_evidence_bytes():
    """svth_format_evidence on a hand-written batch: DEL, INS, INV, an unknown type, NA results
    and values that print as large unsigned numbers."""
    from svtrek_amd import host
    loci = make_loci([(2, 1, 10000, 20000), (1, 2, 5000, 5001), (3, 1, 700, 900), (4, -1, 0, 0xFFFFFFF0),
                      (2, 3, 100, 0xFFFFFFD8)])
    res = np.array([(10003, 20002), (4999, SVT_NA), (SVT_NA, SVT_NA), (SVT_NA, SVT_NA), (SVT_NA, 0xFFFFFFFE)],
                   dtype=RESULT_DTYPE)
    ev = np.array([[(12, 40, 10001, 10005), (4, 5, 20499, 20507)],
                   [(3, 0, 4999, 4999), (0, 0, SVT_NA, SVT_NA)],
                   [(0, 0, SVT_NA, SVT_NA), (0, 0, SVT_NA, SVT_NA)],
                   [(0, 0, SVT_NA, SVT_NA), (0, 0, SVT_NA, SVT_NA)],
                   [(0, 0, SVT_NA, SVT_NA), (1, 0, 0xFFFFFFFE, 0xFFFFFFFE)]], dtype=EVIDENCE_DTYPE)
    head = ("#row\ttype\tchrom\tpos\tend\tref_pos\tref_end\tsup_pos\tdepth_pos\tlo_pos\thi_pos\t"
            "sup_end\tdepth_end\tlo_end\thi_end\n")
    body = ("0\t2\t1\t10000\t20000\t10003\t20002\t12\t40\t10001\t10005\t4\t5\t20499\t20507\n"
            "1\t1\t2\t5000\t5001\t4999\tNA\t3\t0\t4999\t4999\t0\t0\tNA\tNA\n"
            "2\t3\t1\t700\t900\tNA\tNA\t0\t0\tNA\tNA\t0\t0\tNA\tNA\n"
            "3\t4\t-1\t0\t4294967280\tNA\tNA\t0\t0\tNA\tNA\t0\t0\tNA\tNA\n"
            "4\t2\t3\t100\t4294967256\tNA\t4294967294\t0\t0\tNA\tNA\t1\t0\t4294967294\t4294967294\n")
    assert host.format_evidence(loci, res, ev) == head + body
    assert host.format_evidence(loci, res, ev, header=False, threads=1) == body
    assert host.format_evidence(loci[:0], res[:0], ev[:0]) == head


def test_cpu_backend_binds_without_evidence(tmp_path):
    """The CPU restatement has no evidence entry point: bind_abi still binds it, Engine.evidence
    raises a clear error on it, and its CLI refuses --evidence."""
    lib = bind_abi(C.CDLL(CPU_LIB))
    assert not has_evidence(lib) and not any(hasattr(lib, s) for s in EVIDENCE_SYMBOLS)
    pl, loci = fuzz_case(901, n_reads=60)
    with Engine(Params(), device=0, lib=lib) as e:
        e.load_pileup(pl)
        refined = e.refine(loci[:8])
        with pytest.raises(SvtError, match="svtrek_evidence.h"):
            e.evidence(loci[:8], refined)
    bam, vcf = tmp_path / "x.bam", tmp_path / "x.vcf"
    bam.write_bytes(b"")
    vcf.write_text("")
    p = subprocess.run([CPU_CLI, "audt", "-b", str(bam), "-v", str(vcf), "--evidence", str(tmp_path / "e.tsv")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode != 0
    assert p.stderr.decode() == "[ERROR] --evidence: not supported by this backend\n"
    assert not (tmp_path / "e.tsv").exists()
