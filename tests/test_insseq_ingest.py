"""The host ingest's opt-in for inserted bases (svth_bam_read_seq / host.read_bam(insseq=True)): the
sequences of the kept reads' I >= 50 ops, in the final pileup's (read, op) order, against bases this test
decodes from the records' bytes itself.  No GPU."""
import random
import struct

import numpy as np
import pytest

from svtrek_amd import host

import bamfix

NT4 = {1: 0, 2: 1, 4: 2, 8: 3}
M, I, D, N, S, H, P, EQ, X = range(9)


def header(n_ref=1):
    text = b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:%d\tLN:1000000\n" % (t + 1) for t in range(n_ref))
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref)
    for t in range(n_ref):
        nm = b"%d\0" % (t + 1)
        raw += struct.pack("<i", len(nm)) + nm + struct.pack("<i", 1000000)
    return raw


def with_seq(raw: bytes, codes) -> bytes:
    """The record with its SEQ nibbles replaced by `codes` (len == l_seq)."""
    b = bytearray(raw)
    l_qname, n_cig, l_seq = b[4 + 8], struct.unpack_from("<H", b, 4 + 12)[0], struct.unpack_from("<i", b, 4 + 16)[0]
    assert len(codes) == l_seq
    at = 4 + 32 + l_qname + 4 * n_cig
    for i in range((l_seq + 1) // 2):
        hi = codes[2 * i]
        lo = codes[2 * i + 1] if 2 * i + 1 < l_seq else 0
        b[at + i] = hi << 4 | lo
    return bytes(b)


def decode(raw: bytes, ops) -> list[np.ndarray]:
    """The inserted sequences of one record from its bytes and the CIGAR the pileup keeps."""
    l_qname, n_cig, l_seq = raw[4 + 8], struct.unpack_from("<H", raw, 4 + 12)[0], struct.unpack_from("<i", raw, 4 + 16)[0]
    seq = raw[4 + 32 + l_qname + 4 * n_cig:]
    out, q = [], 0
    for op, ln in ops:
        if op == I and ln >= 50:
            if q + ln <= l_seq:
                out.append(np.array([NT4.get((seq[t >> 1] >> (0 if t & 1 else 4)) & 15, 4) for t in range(q, q + ln)], np.uint8))
            else:
                out.append(np.full(ln, 4, np.uint8))
        if op in (M, I, S, EQ, X):
            q += ln
    return out


def write(path, raws, n_ref=1):
    with open(path, "wb") as f:
        f.write(bamfix.bgzf_blocks(header(n_ref) + b"".join(raws)))


def check(path, want_seqs, **kw):
    pl, info, (off, bases) = host.read_bam(str(path), insseq=True, **kw)
    pl0, info0 = host.read_bam(str(path), **kw)
    for f in ("tid_off", "pos", "endpos", "cig_off", "cigar", "clip"):
        assert np.array_equal(getattr(pl, f), getattr(pl0, f)), f     # the pileup itself is the plain reader's
    ins = ((pl.cigar & 15) == 1) & ((pl.cigar >> 4) >= 50)
    assert len(off) == int(ins.sum()) + 1 and off[0] == 0              # = svt_pileup_ins_count() after a load
    assert np.array_equal(np.diff(off.astype(np.int64)), (pl.cigar[ins] >> 4).astype(np.int64))
    assert len(want_seqs) == len(off) - 1
    for k, s in enumerate(want_seqs):
        assert np.array_equal(bases[int(off[k]):int(off[k + 1])], s), k
    return pl, off, bases


def test_offsets_lengths_codes_and_clips(tmp_path):
    rng = random.Random(5)
    cases = [  # (ops, l_seq or None for the CIGAR's own)
        [(M, 10), (I, 50), (M, 5)],            # even offset, even length
        [(M, 11), (I, 51), (M, 5)],            # odd offset, odd length
        [(M, 11), (I, 50), (M, 4)],            # odd offset, even length
        [(M, 10), (I, 53), (M, 4)],            # even offset, odd length
        [(S, 7), (I, 60), (M, 9)],             # a leading S before the I
        [(H, 9), (I, 60), (M, 9)],             # a leading H: consumes no SEQ
        [(I, 64), (M, 20)],                    # I first
        [(M, 20), (I, 65)],                    # I last
        [(M, 3), (EQ, 2), (X, 2), (D, 70), (N, 5), (P, 1), (I, 49), (I, 50), (M, 1), (I, 77), (S, 3)],   # every op kind; I49 is no item
    ]
    raws, want = [], []
    for k, ops in enumerate(cases):
        l_seq = sum(ln for op, ln in ops if op in (M, I, S, EQ, X))
        raw = bamfix.record(0, 100 + k, b"r%d" % k, ops, 0, l_seq, b"", False, rng)
        codes = [(t + k) % 16 for t in range(l_seq)]                                   # all 16 SEQ codes
        raw = with_seq(raw, codes)
        raws.append(raw)
        want += decode(raw, ops)
    # the first case written out by hand: offset 10, codes (t + 0) % 16 for t = 10 .. 59
    assert want[0].tolist() == [NT4.get(t % 16, 4) for t in range(10, 60)]
    assert want[5].tolist() == [NT4.get((t + 5) % 16, 4) for t in range(0, 60)]       # leading H: offset 0
    assert want[4].tolist() == [NT4.get((t + 4) % 16, 4) for t in range(7, 67)]       # leading S: offset 7
    assert set(np.concatenate(want).tolist()) == {0, 1, 2, 3, 4}
    write(tmp_path / "a.bam", raws)
    check(tmp_path / "a.bam", want)
    check(tmp_path / "a.bam", want, threads=1)


def test_cg_restored_lseq_zero_and_short_seq(tmp_path):
    rng = random.Random(6)
    ops = [(S, 4), (M, 30), (I, 55), (M, 10), (I, 90), (M, 3)]
    l_seq = 4 + 30 + 55 + 10 + 90 + 3
    cg = with_seq(bamfix.record(0, 50, b"cg", ops, 0, l_seq, b"XAc\5", True, rng), [(3 * t) % 16 for t in range(l_seq)])
    nos = bamfix.record(0, 60, b"noseq", [(M, 5), (I, 58), (M, 5)], 0, 0, b"", False, rng)             # l_seq = 0
    short = bamfix.record(0, 70, b"short", [(M, 5), (I, 50), (M, 5), (I, 52), (M, 1)], 0, 80, b"", False, rng)  # 2nd op past l_seq
    short = with_seq(short, [1, 2, 4, 8] * 20)
    unplaced = bamfix.record(-1, -1, b"u", [], 4, 60, b"", False, rng)
    want = decode(cg, ops) + [np.full(58, 4, np.uint8)] + decode(short, [(M, 5), (I, 50), (M, 5), (I, 52), (M, 1)])
    assert want[0].tolist() == [NT4.get((3 * t) % 16, 4) for t in range(34, 89)]
    assert want[3].tolist() == [(t % 4) for t in range(5, 55)] and want[4].tolist() == [4] * 52
    write(tmp_path / "b.bam", [cg, nos, short, unplaced])
    pl, off, bases = check(tmp_path / "b.bam", want)
    assert host.read_bam(str(tmp_path / "b.bam"))[1]["cg_restored"] == 1 and len(pl.pos) == 3


def test_unsorted_file_is_reordered_with_its_sequences(tmp_path):
    rng = random.Random(7)
    spec = [(1, 500, [(M, 9), (I, 50), (M, 1)]), (0, 900, [(M, 3), (I, 61), (M, 1), (I, 70), (M, 2)]), (0, 100, [(M, 40)]),
            (0, 900, [(I, 52), (M, 8)]), (1, 20, [(M, 1), (I, 99), (M, 1)]), (0, 300, [(S, 2), (I, 57), (M, 8)])]
    raws, per = [], []
    for k, (tid, pos, ops) in enumerate(spec):
        l_seq = sum(ln for op, ln in ops if op in (M, I, S, EQ, X))
        raw = with_seq(bamfix.record(tid, pos, b"q%d" % k, ops, 0, l_seq, b"", False, rng),
                       [rng.choice([1, 2, 4, 8, 15]) for _ in range(l_seq)])
        raws.append(raw)
        per.append(decode(raw, ops))
    order = sorted(range(len(spec)), key=lambda k: (spec[k][0], spec[k][1], k))      # the stable (tid, pos) sort
    want = [s for k in order for s in per[k]]
    write(tmp_path / "c.bam", raws, n_ref=2)
    pl, off, bases = check(tmp_path / "c.bam", want)
    assert pl.pos.tolist() == [100, 300, 900, 900, 20, 500]


@pytest.mark.parametrize("seed", [11, 12])
def test_bamfix_files_with_seq(tmp_path, seed):
    raw, recs = bamfix.make_bam(seed, n_reads=1500, seq=True)
    path = tmp_path / "f.bam"
    with open(path, "wb") as f:
        f.write(bamfix.bgzf_blocks(raw))
    want = []
    n_cg = 0
    for r in recs:
        if not (0 <= r["tid"] < 3 and r["pos"] >= 0):
            continue
        ops = r["ops"]
        if r["cg"] and not bamfix.restored(r):     # the placeholder CIGAR stays: no I op
            ops = []
        n_cg += bool(r["cg"] and bamfix.restored(r) and any(op == I and ln >= 50 for op, ln in ops))
        want += decode(r["raw"], ops)
    assert len(want) > 500 and n_cg > 5
    check(path, want)
    pl, info, (off, bases) = host.read_bam(str(path), insseq=True)
    assert bases.max() <= 4 and len(set(bases.tolist())) == 5


def test_no_seq_in_the_file_and_the_plain_reader(tmp_path):
    raw, recs = bamfix.make_bam(13, n_reads=300, seq=False)
    path = tmp_path / "n.bam"
    with open(path, "wb") as f:
        f.write(bamfix.bgzf_blocks(raw))
    pl, info, (off, bases) = host.read_bam(str(path), insseq=True)
    assert len(off) > 10 and (bases == 4).all() and len(bases) == int(off[-1])
    assert len(host.read_bam(str(path))) == 2                     # without the opt-in: (pileup, info) as before
    import ctypes as C
    L = host.load_host()
    err = C.create_string_buffer(256)
    h = L.svth_bam_read(str(path).encode(), 1, err, 256)
    try:
        from svtrek_amd._lib import SvtInsseqView
        assert L.svth_bam_insseq(h, C.byref(SvtInsseqView())) == 0   # a pileup read without the sequences
    finally:
        L.svth_bam_free(h)
