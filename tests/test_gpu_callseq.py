"""include/svtrek_callseq.h on the HIP engine: Engine.call_consensus against the numpy model
(tests/callseq_ref.py, pinned by tests/test_callseq_model.py; its consensus is oracle_ffi.poa_consensus on the
model's support list), record for record -- len, n_support, n_used and bases[:min(len, cap)] -- on pileups
built to reach every path of the item table and the support gather, the lifecycle of the table, the status
codes, and `svtrek call --ins-seq`."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest

from svtrek_amd import Engine, Params, SvtError, from_reads, host
from svtrek_amd._lib import SVT_DEL, SVT_EINVAL, SVT_ESTATE, SVT_INS, has_callseq

import bamfix
import call_ref
import call_split_ref
import callseq_ref
import fuzz
from test_insseq_ingest import header, with_seq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "svtrek_amd", "svtrek")
M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
NAMES = {"DEL": SVT_DEL, "INS": SVT_INS}
CODE = {0: 1, 1: 2, 2: 4, 3: 8, 4: 15}      # nt4 -> a SEQ nibble


@pytest.fixture(scope="module")
def eng():
    with Engine(Params(), device=0) as e:
        assert has_callseq(e.lib)
        yield e


def make_seqs(pl, rng, noise=0.03):
    """(off, bases, {len: allele}): every I >= 50 op, in (read, op) order, carries a noisy copy of its
    length's allele."""
    w = pl.cigar
    lens = (w[((w & 15) == 1) & ((w >> 4) >= 50)] >> 4).astype(np.int64)
    alleles, seqs = {}, []
    for L in lens.tolist():
        if L not in alleles:
            alleles[L] = rng.integers(0, 4, L).astype(np.uint8)
        s = alleles[L].copy()
        m = rng.random(L) < noise
        s[m] = (s[m] + rng.integers(1, 4, int(m.sum()))) & 3
        seqs.append(s)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return off, (np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)), alleles


def check(eng, pl, off, bases, cap=4096, first=0, n=None, P=0, link=None, min_support=None, types=("DEL", "INS"), **kw):
    """Scan, then Engine.call_consensus == the model; returns (calls, res, out)."""
    want_calls = call_split_ref.call(pl, 10 if link is None else link, 3 if min_support is None else min_support,
                                     tuple(NAMES[t] for t in types), P)[0]
    calls = eng.call(link=link, min_support=min_support, types=types, len_permille=P)
    assert np.array_equal(calls, want_calls)
    res, out = eng.call_consensus(first, n, cap, **kw)
    sub = calls[first:] if n is None else calls[first:first + n]
    wres, wseqs = callseq_ref.consensus(pl, sub, off, bases, **kw)
    assert len(res) == len(sub) and out.shape == (len(sub), cap)
    for j in range(len(sub)):
        assert tuple(int(v) for v in res[j]) == tuple(int(v) for v in wres[j]), (j, sub[j], res[j], wres[j])
        m = min(len(wseqs[j]), cap)
        assert np.array_equal(out[j, :m], wseqs[j][:m]), j
    assert np.array_equal(eng.call_fetch(0, len(calls)), calls)      # the scan's calls are as they were
    return calls, res, out


def load(eng, pl, rng, noise=0.03):
    off, bases, alleles = make_seqs(pl, rng, noise)
    eng.load_pileup(pl)
    assert eng.ins_count == len(off) - 1
    eng.load_insseq(off, bases)
    return off, bases, alleles


def ins_at(x, ln=60, tid=0, lead=200, tail=60):
    return (tid, x - lead, [(M, lead), (I, ln), (M, tail)])


def test_item_counts_around_max_support(eng):
    rng = np.random.default_rng(1)
    reads = []
    for i, c in enumerate((3, 63, 64, 65, 200)):
        reads += [ins_at(20000 * (i + 1) + int(rng.integers(0, 3)), 60, lead=int(rng.integers(50, 3000)))
                  for _ in range(c)]
    pl = from_reads(1, reads, clip={})
    off, bases, _ = load(eng, pl, rng, noise=0.0)       # identical sequences: every one aligns and is fused
    calls, res, _ = check(eng, pl, off, bases)
    assert calls["support"].tolist() == [3, 63, 64, 65, 200] and res["n_support"].tolist() == [3, 63, 64, 65, 200]
    assert res["n_used"].tolist() == [3, 32, 32, 32, 32]                                  # max_seqs fused
    st = eng.call_consensus_stats()
    assert st["items"] == 395 and st["ins_calls"] == 5 and st["reach"] == callseq_ref.reach(pl) and st["deferred"] == 0
    assert st["window_items"] >= 395 and st["window_max"] >= 200
    _, res, _ = check(eng, pl, off, bases, max_support=5)          # the 5 smallest k alone are fused
    assert res["n_support"].tolist() == [3, 63, 64, 65, 200] and res["n_used"].tolist() == [3, 5, 5, 5, 5]
    # The 64 smallest k are kept, no more: with the sequences of each call's first 40 k empty (an empty
    # sequence is passed over), 24 of the 65- and 200-item calls' kept 64 are left to fuse, 23 of the 63.
    items = callseq_ref.ins_items(pl)
    lens = np.diff(off.astype(np.int64))
    for c in calls[1:]:
        lens[callseq_ref.call_items(items, c)[:40]] = 0
    off2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    keep = np.repeat(np.diff(off2.astype(np.int64)) > 0, np.diff(off.astype(np.int64)))
    eng.load_insseq(off2, bases[keep])
    _, res, _ = check(eng, pl, off2, bases[keep])
    assert res["n_support"].tolist() == [3, 63, 64, 65, 200] and res["n_used"].tolist() == [3, 23, 24, 24, 24]


def test_items_straddle_chunk_edges_between_unrelated_ops(eng):
    """One candidate range of several hundred table entries: the call's own items (I 70 at X) sit between a
    second I >= 50 op of the same read (x outside the range), ops at the same x of another length and the
    items of a neighbouring cluster."""
    rng = np.random.default_rng(2)
    X, reads = 50000, []
    for i in range(150):
        lead = int(rng.integers(10, 4000))
        if i % 3 == 0:
            reads.append((0, X - lead, [(M, lead), (I, 70), (M, 500), (I, 80), (M, 20)]))      # same read, x + 500
        elif i % 3 == 1:
            reads.append((0, X - lead, [(M, lead), (I, 200 + 30 * i), (M, 20)]))                # same x, another length
        else:
            reads.append((0, X + 40 - lead, [(I, 55), (M, lead), (I, 70), (M, 20)]))           # the cluster next door
    pl = from_reads(1, reads, clip={})
    off, bases, _ = load(eng, pl, rng)
    calls, res, _ = check(eng, pl, off, bases, P=100)
    mine = [j for j, c in enumerate(calls) if int(c["pos"]) == X and int(c["len"]) == 70]
    assert len(mine) == 1 and int(res[mine[0]]["n_support"]) == 50
    assert eng.call_consensus_stats()["window_max"] > 128
    # the model's k of that call are spread over more than two 64-entry chunks of the range
    ks = callseq_ref.call_items(callseq_ref.ins_items(pl), calls[mine[0]])
    assert ks.max() - ks.min() > 128 and len(set((ks // 64).tolist())) >= 3
    check(eng, pl, off, bases, P=0)
    check(eng, pl, off, bases, P=100, min_support=1, max_support=7)


def test_two_alleles_of_one_start_two_contigs_and_a_del(eng):
    rng = np.random.default_rng(3)
    reads = [ins_at(7000, 300, lead=int(rng.integers(100, 900))) for _ in range(5)]
    reads += [ins_at(7000, 500, lead=int(rng.integers(100, 900))) for _ in range(5)]
    reads += [(0, 6500, [(M, 500), (D, 90), (M, 300)])] * 3                       # a DEL at the same pos
    reads += [ins_at(7000, 301, tid=1, lead=int(rng.integers(100, 900))) for _ in range(4)]    # the same x on contig 2
    pl = from_reads(2, reads, clip={})
    off, bases, alleles = load(eng, pl, rng, noise=0.0)
    calls, res, out = check(eng, pl, off, bases, P=100)
    assert [(int(c["type"]), int(c["chrom"]), int(c["len"])) for c in calls] == [
        (SVT_INS, 1, 300), (SVT_INS, 1, 500), (SVT_DEL, 1, 90), (SVT_INS, 2, 301)]
    assert [tuple(int(v) for v in r) for r in res] == [(300, 5, 5, 0), (500, 5, 5, 0), (-1, 0, 0, 0), (301, 4, 4, 0)]
    for j, L in ((0, 300), (1, 500), (3, 301)):                                    # each its own allele
        assert np.array_equal(out[j, :L], alleles[L])
    calls, res, _ = check(eng, pl, off, bases, P=0)                                # one call of both alleles
    assert res["n_support"].tolist() == [10, 0, 4] and res["len"].tolist()[1:] == [-1, 301]


def test_leading_h_past_endpos_and_reach_per_load(eng):
    rng = np.random.default_rng(4)
    far = [(0, 100, [(H, 5000), (I, 60), (M, 10)])] * 3          # x = 5100, endpos = 110
    near = [ins_at(90000, 64, lead=300)] * 3
    long_read = [(0, 50000, [(M, 40000), (I, 64), (M, 10)])]      # starts 40 kb before its item at 90000
    pl = from_reads(1, far + near + long_read, clip={})
    off, bases, _ = load(eng, pl, rng)
    calls, res, _ = check(eng, pl, off, bases)
    assert [(int(c["pos"]), int(c["support"])) for c in calls] == [(5100, 3), (90000, 4)]
    assert res["n_support"].tolist() == [3, 4] and eng.call_consensus_stats()["reach"] == 40000
    pl = from_reads(1, far + near, clip={})                      # without the long read: the reach is this load's
    off, bases, _ = load(eng, pl, rng)
    _, res, _ = check(eng, pl, off, bases)
    assert res["n_support"].tolist() == [3, 3] and eng.call_consensus_stats()["reach"] == 5000
    pl = from_reads(1, near, clip={})
    off, bases, _ = load(eng, pl, rng)
    check(eng, pl, off, bases)
    assert eng.call_consensus_stats()["reach"] == 300


def test_length_edges_and_saturated_items(eng):
    rng = np.random.default_rng(5)
    reads = [ins_at(3000, 100)] * 3 + [ins_at(3001, 101)] * 3                     # len == max_len kept, + 1 dropped
    reads += [(0, 8000, [(M, 100), (I, 49), (M, 5), (I, 50), (M, 5)])] * 3        # an I of exactly 50 (49 is no item)
    reads += [(0, 5, [(H, (1 << 28) - 1)] * 4 + [(M, 10), (I, 60), (M, 1)])] * 3  # x >= 2^30: items of no call
    pl = from_reads(1, reads, clip={})
    off, bases, _ = load(eng, pl, rng)
    calls, res, _ = check(eng, pl, off, bases, max_len=100)
    assert [(int(c["pos"]), int(c["support"])) for c in calls] == [(3001, 6), (8105, 3)]
    assert res["n_support"].tolist() == [3, 3] and res["n_used"].tolist() == [3, 3]
    assert eng.call_stats()["skipped"] == 3
    st = eng.call_consensus_stats()
    assert st["items"] == 12 and st["reach"] == 200
    _, res, _ = check(eng, pl, off, bases, max_len=99)
    assert tuple(int(v) for v in res[0]) == (0, 0, 0, 0) and int(res[1]["n_support"]) == 3
    check(eng, pl, off, bases, P=1000, min_support=1)


def test_empty_pileups_windows_and_cap(eng):
    rng = np.random.default_rng(6)
    pl = from_reads(2, [], clip={})
    off, bases, _ = load(eng, pl, rng)
    _, res, out = check(eng, pl, off, bases)
    assert len(res) == 0 and out.shape == (0, 4096)
    pl = from_reads(1, [(0, 400, [(M, 100), (D, 90), (M, 50)])] * 3, clip={})     # no I >= 50 op at all
    off, bases, _ = load(eng, pl, rng)
    _, res, _ = check(eng, pl, off, bases)
    assert [tuple(int(v) for v in r) for r in res] == [(-1, 0, 0, 0)] and eng.call_consensus_stats()["items"] == 0
    reads = [ins_at(4000 * (k + 1), 80 + 40 * k) for k in range(6) for _ in range(3)] + [(0, 400, [(M, 100), (D, 90), (M, 50)])] * 3
    pl = from_reads(1, reads, clip={})
    off, bases, _ = load(eng, pl, rng)
    _, res, _ = check(eng, pl, off, bases, types=("DEL",))                           # a scan without INS calls
    assert res["len"].tolist() == [-1] and eng.call_consensus_stats()["ins_calls"] == 0
    calls, full, fout = check(eng, pl, off, bases)
    assert len(calls) == 7
    eng.call_consensus(0, 0)                                                         # n = 0
    assert len(eng.call_consensus(7, 0)[0]) == 0 and len(eng.call_consensus(7)[0]) == 0
    for first, n in ((2, 3), (6, 1), (1, None)):
        _, res, out = check(eng, pl, off, bases, first=first, n=n)
        hi = len(calls) if n is None else first + n
        assert np.array_equal(res, full[first:hi])
        assert all(np.array_equal(out[j, :max(int(res[j]["len"]), 0)], fout[first + j, :max(int(res[j]["len"]), 0)])
                   for j in range(len(res)))
    _, res, out = check(eng, pl, off, bases, cap=10)                                 # cap smaller than the consensus
    assert np.array_equal(res, full) and out.shape == (7, 10) and int(res["len"].max()) >= 250
    _, res, out = check(eng, pl, off, bases, cap=0)
    assert np.array_equal(res, full)


def test_a_call_deferred_to_the_big_slots(eng, monkeypatch):
    rng = np.random.default_rng(7)
    reads = [ins_at(9000, 400, lead=int(rng.integers(100, 900))) for _ in range(12)] + [ins_at(30000, 70)] * 3
    pl = from_reads(1, reads, clip={})
    off, bases, _ = load(eng, pl, rng, noise=0.08)
    _, plain, pout = check(eng, pl, off, bases, max_len=500)
    assert eng.call_consensus_stats()["deferred"] == 0
    monkeypatch.setenv("SVTREK_POA_SMALL_NODES", "1")      # budget = max_len + 2 nodes: the noisy 400 bp graph outgrows it
    _, res, out = check(eng, pl, off, bases, max_len=500)
    assert eng.call_consensus_stats()["deferred"] >= 1 and (res["status"] == 0).all()
    assert np.array_equal(res, plain) and np.array_equal(out, pout)


@functools.lru_cache(maxsize=None)
def fuzz_pileup(seed, n_reads, max_ops):
    """tests/test_gpu_call.py's generator (a copy)."""
    rng = np.random.default_rng(seed)
    hot = [int(x) for x in rng.integers(5000, 55000, size=5)]
    return fuzz.random_pileup(rng, n_targets=2, contig_len=60000, n_reads=n_reads, max_ops=max_ops, hot=hot)


@pytest.mark.parametrize("seed, n_reads, max_ops", [(901, 400, 60), (905, 120, 600)], ids=["short901", "long905"])
def test_fuzz_pileups(eng, seed, n_reads, max_ops):
    pl = fuzz_pileup(seed, n_reads, max_ops)
    off, bases, _ = load(eng, pl, np.random.default_rng(seed), noise=0.05)
    _, res, _ = check(eng, pl, off, bases, P=0, min_support=3)
    assert (res["n_used"] > 1).sum() >= 3
    assert eng.call_consensus_stats()["reach"] == callseq_ref.reach(pl)
    check(eng, pl, off, bases, P=100, min_support=2, max_len=1000, max_support=6, max_seqs=4, cap=300)
    check(eng, pl, off, bases, P=50, link=200, min_support=1, max_len=400, cap=64)


def test_reindex_and_rescan(eng):
    pl = fuzz_pileup(901, 400, 60)
    off, bases, _ = load(eng, pl, np.random.default_rng(8))
    _, res, out = check(eng, pl, off, bases, P=100, min_support=2, max_len=600)
    table_ms = eng.call_consensus_stats()["table_ms"]
    eng.reindex()
    _, res2, out2 = check(eng, pl, off, bases, P=100, min_support=2, max_len=600)
    assert np.array_equal(res, res2) and np.array_equal(out, out2)
    assert eng.call_consensus_stats()["table_ms"] == table_ms         # the table is built once per load
    eng.call(min_support=2)                                           # another scan: the consensus follows it
    r3, _ = eng.call_consensus(max_len=600)
    assert len(r3) == len(eng.call_fetch(0, eng.call_device()[1]))
    check(eng, pl, off, bases, P=0, min_support=2, max_len=600)


def test_status_codes():
    rng = np.random.default_rng(9)
    pl = from_reads(1, [ins_at(3000, 70)] * 3, clip={})
    off, bases, _ = make_seqs(pl, rng)
    with Engine(Params(), device=0) as e:
        def code(first=0, n=1, cap=16, poa=None):
            """svt_call_consensus's status for a call that must fail."""
            res, out = np.zeros((4, 4), dtype=np.int32), np.zeros(4 * 16, dtype=np.uint8)
            p = e.poa_params(**(poa or {}))
            rc = e.lib.svt_call_consensus(e._h, C.byref(p), first, n, cap, out.ctypes.data, res.ctypes.data)
            assert rc != 0
            with pytest.raises(SvtError):
                e._check(rc)
            return rc
        assert code() == SVT_ESTATE                              # before svt_load_pileup
        e.load_pileup(pl)
        assert code() == SVT_ESTATE                              # before a scan
        assert code(n=0) == SVT_ESTATE
        assert len(e.call()) == 1
        assert code() == SVT_ESTATE                              # before svt_load_insseq
        e.load_insseq(off, bases)
        assert code(first=0, n=2) == SVT_EINVAL                  # past the scanned count
        assert code(first=2, n=0) == SVT_EINVAL
        assert code(poa={"band_b": 60}) == SVT_EINVAL            # svt_poa_consensus's limits
        assert code(poa={"max_seqs": 33}) == SVT_EINVAL
        assert code(poa={"max_len": 4097}) == SVT_EINVAL
        assert code(cap=-1) == SVT_EINVAL
        res, out = e.call_consensus(1, 0)                        # n == 0 at the end of the range: OK
        assert len(res) == 0
        res, out = e.call_consensus()
        assert tuple(int(v) for v in res[0]) == (70, 3, 3, 0)
        e.load_pileup(pl)                                        # a new load: scan and sequences are gone
        assert code() == SVT_ESTATE
        e.call()
        assert code() == SVT_ESTATE


# ---------------------------------------------------------------- the CLI
def cli_case(rng):
    """(reads, per read its SEQ as nt4) -- two alleles at one start, a long allele, a DEL and a singleton."""
    alleles = {L: rng.integers(0, 4, L).astype(np.uint8) for L in (60, 300, 500, 150)}
    spec = []
    for k in range(6):
        spec.append((100000, (300, 500)[k % 2], 700 + 150 * k))
    for k in range(4):
        spec.append((160000, 150, 300 + 90 * k))
    for k in range(3):
        spec.append((220000, 60, 500 + 10 * k))
    reads, seqs = [], []
    for x, L, lead in spec:
        ops = [(S, 5), (M, lead), (I, L), (M, 900)]
        s = alleles[L].copy()
        m = rng.random(L) < 0.02
        s[m] = (s[m] + 1) & 3
        reads.append((0, x - lead, ops))
        seqs.append(np.concatenate([rng.integers(0, 4, 5 + lead).astype(np.uint8), s, rng.integers(0, 5, 900).astype(np.uint8)]))
    for k in range(3):
        reads.append((0, 40000 - 100 * k, [(M, 400 + 100 * k), (D, 120), (M, 300)]))
        seqs.append(rng.integers(0, 4, 700 + 100 * k).astype(np.uint8))
    return reads, seqs


def write_seq_bam(path, reads, seqs):
    rnd = random.Random(1)
    order = sorted(range(len(reads)), key=lambda i: (reads[i][0], reads[i][1], i))
    raw = header(1)
    for k, i in enumerate(order):
        tid, pos, ops = reads[i]
        assert len(seqs[i]) == sum(ln for op, ln in ops if op in (0, 1, 4, 7, 8))
        rec = bamfix.record(tid, pos, b"r%d" % k, ops, 0, len(seqs[i]), b"", False, rnd)
        raw += with_seq(rec, [CODE[int(b)] for b in seqs[i]])
    with open(path, "wb") as f:
        f.write(bamfix.bgzf_blocks(raw))
    return [reads[i] for i in order], [seqs[i] for i in order]


@pytest.mark.parametrize("inflate", ["cpu", "gpu"])
def test_cli_ins_seq(tmp_path, inflate):
    reads, seqs = cli_case(np.random.default_rng(10))
    bam, vcf, vcf0 = str(tmp_path / "x.bam"), str(tmp_path / "c.vcf"), str(tmp_path / "c0.vcf")
    reads, seqs = write_seq_bam(bam, reads, seqs)
    pl = from_reads(1, reads, clip=None)
    ins = []
    for (tid, pos, ops), s in zip(reads, seqs):                      # the inserted bases, in (read, op) order
        q = 0
        for op, ln in ops:
            if op == I and ln >= 50:
                ins.append(s[q:q + ln])
            if op in (0, 1, 4, 7, 8):
                q += ln
    off = np.concatenate([[0], np.cumsum([len(s) for s in ins])]).astype(np.uint64)
    bases = np.concatenate(ins)
    want = call_split_ref.call(pl, len_permille=100)[0]
    assert [(int(c["type"]), int(c["len"]), int(c["support"])) for c in want] == [
        (SVT_DEL, 120, 3), (SVT_INS, 300, 3), (SVT_INS, 500, 3), (SVT_INS, 150, 4), (SVT_INS, 60, 3)]

    def run(*args):
        return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    for cap in (4096, 200):
        wres, wseqs = callseq_ref.consensus(pl, want, off, bases)
        text = host.format_calls(want, ["1"], consensus=(wres, callseq_ref.padded(wseqs, cap)))
        p = run("call", "-b", bam, "-o", vcf, "--inflate", inflate, "--len-permille", "100", "--ins-seq", "--ins-seq-cap", str(cap),
                "--verbose")
        assert p.returncode == 0 and p.stdout == "" and "ins-seq" in p.stderr and "INS calls 4" in p.stderr, p.stderr
        with open(vcf) as f:
            got = f.read()
        assert got == text
        alts = [ln.split("\t")[4] for ln in got.splitlines() if ln[0] != "#"]
        assert alts[0] == "<DEL>" and [a == "<INS>" for a in alts[1:]] == [not 1 <= len(w) <= cap for w in wseqs[1:]]
        assert [abs(len(w) - L) <= 5 for w, L in zip(wseqs[1:], (300, 500, 150, 60))] == [True] * 4
        assert all(a == "N" + "".join("ACGTN"[b] for b in w) for a, w in zip(alts[1:], wseqs[1:]) if a != "<INS>")
    p = run("call", "-b", bam, "-o", vcf0, "--inflate", inflate, "--len-permille", "100")
    assert p.returncode == 0
    with open(vcf0) as f:
        assert f.read() == host.format_calls(want, ["1"])             # without the flag: the bytes as they were
    a, a0 = run("audt", "-b", bam, "-v", vcf, "--inflate", inflate), run("audt", "-b", bam, "-v", vcf0, "--inflate", inflate)
    assert a.returncode == 0 and a0.returncode == 0 and a.stdout == a0.stdout, a.stderr
    assert len([ln for ln in a.stdout.splitlines() if ln.startswith("(INS)")]) >= 1
    p = run("call", "-b", bam, "--inflate", inflate)
    assert p.returncode == 0 and p.stdout == host.format_calls(call_ref.call(pl)[0], ["1"])
    import genotype_ref
    from svtrek_amd import calls_to_sites
    p = run("call", "-b", bam, "--inflate", inflate, "--len-permille", "100", "--genotype", "--ins-seq")
    wres, wseqs = callseq_ref.consensus(pl, want, off, bases)
    assert p.returncode == 0 and p.stdout == host.format_calls(
        want, ["1"], genotypes=genotype_ref.genotype(pl, calls_to_sites(want)), consensus=(wres, callseq_ref.padded(wseqs, 4096)))
    p = run("call", "-b", bam, "--ins-seq", "--ins-seq-cap", "0")
    assert p.returncode == 1 and "--ins-seq-cap" in p.stderr
