"""svth_bam_read_sa / svth_bam_junctions (bam_ingest.cpp) through host.read_bam(junctions=True): the segment
table of BAMs written with tests/bamfix.record and hand-made aux bytes equals tests/junction_ref.segments --
SA before and after aux fields of every type and around a CG tag, 1-based positions, several entries, an
unsorted file, region reads, and every malformed shape (counted, the other records intact)."""
import random
import struct

import numpy as np

from svtrek_amd import host

import bamfix
import junction_ref as J

M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
NAMES = [b"chr1", b"chr2", b"chrUn_x"]
EVERY_TYPE = (b"XAAQ" + b"XbcA" + b"XcC\xff" + b"Xds\x01\x02" + b"XeS\x03\x04" + b"Xfi\x05\x06\x07\x08" + b"XgI\x09\x0a\x0b\x0c" +
              b"Xhf\x00\x00\x80\x3f" + b"XiZSA:Z:fake,1,+,5M,0,0;\0" + b"XjH1AE3\0" + b"XkBc\x02\x00\x00\x00\x01\x02" +
              b"XlBS\x01\x00\x00\x00\x01\x02" + b"XmBf\x01\x00\x00\x00\x00\x00\x80\x3f" + b"XnBI\x00\x00\x00\x00")


def sa_tag(entries) -> bytes:
    return b"SAZ" + b"".join(b"%s,%d,%s,%s,%d,%d;" % (NAMES[t], p, st.encode(), c.encode(), 60, 3) for t, p, st, c in entries) + b"\0"


def header(n_ref=3):
    text = b"@HD\tVN:1.6\n"
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref)
    for t in range(n_ref):
        nm = NAMES[t] + b"\0"
        hdr += struct.pack("<i", len(nm)) + nm + struct.pack("<i", 1 << 29)
    return hdr


def rec(tid, pos, ops, flag=0, aux=b"", cg=False, seed=1):
    l_seq = sum(ln for op, ln in ops if op in (M, I, S, 7, 8))
    return bamfix.record(tid, pos, b"r%d" % pos, ops, flag, l_seq, aux, cg, random.Random(seed))


def write(path, raws, n_ref=3):
    raw = header(n_ref) + b"".join(raws)
    assert len(raw) < 65280                                   # one BGZF block: a virtual offset is a byte offset
    with open(path, "wb") as f:
        f.write(bamfix.bgzf_blocks(raw))
    return str(path)


def write_bai(path, raws, firsts, n_ref=3):
    """A BAI with linear indices alone (all the region reader looks at): firsts[t] = {16-kb window: record index}."""
    offs = np.cumsum([len(header(n_ref))] + [len(r) for r in raws])
    out = b"BAI\1" + struct.pack("<i", n_ref)
    for t in range(n_ref):
        w = firsts.get(t, {})
        n = max(w) + 1 if w else 0
        out += struct.pack("<i", 0) + struct.pack("<i", n) + b"".join(struct.pack("<Q", int(offs[w[k]]) if k in w else 0) for k in range(n))
    out += struct.pack("<Q", 0)
    with open(path + ".bai", "wb") as f:
        f.write(out)


def read_table(path, sa, flags, malformed=0, region=None):
    """The file's table == junction_ref.segments(its pileup, sa), sa keyed by pileup read index; the pileup itself
    is the plain reader's."""
    pl, info, table = host.read_bam(path, threads=3, junctions=True, region=region)
    plain, _ = host.read_bam(path, threads=3, region=region)
    for f in ("tid_off", "pos", "endpos", "cig_off", "cigar", "clip"):
        assert np.array_equal(getattr(pl, f), getattr(plain, f)), f
    assert info["sa_malformed"] == malformed
    pl.flag = np.array(flags if flags is not None else [0] * pl.n_reads, dtype=np.uint16)
    want = J.segments(pl, sa)
    assert table[2].dtype == want[2].dtype
    for got, w in zip(table, want):
        assert np.array_equal(got, w), (got, w)
    return pl, table


def files(tmp_path):
    """Every BAM of this module: {name: (path, sa, flags, malformed, region)} (tests/test_junction_san.py reads
    them under the sanitizers)."""
    out = {}
    e1, e2, e3 = (0, 2301, "+", "1000S500M5I20D30M7H"), (1, 1, "-", "3H4S10=2X6N1M9S"), (2, 77, "-", "10M")
    cg_then_sa = b"CGBI" + struct.pack("<I3I", 3, 30 << 4 | M, 5 << 4 | D, 10 << 4 | M) + sa_tag([e3])
    raws = [rec(0, 1000, [(M, 1000), (S, 540)], aux=sa_tag([e1])),                                  # SA alone, 1-based -> 0-based
            rec(0, 1100, [(S, 10), (M, 90), (I, 5), (D, 20), (M, 30), (H, 7)], flag=16, aux=EVERY_TYPE + sa_tag([e1, e2, e3])),
            rec(0, 1200, [(M, 50)], aux=EVERY_TYPE),                                                # no SA (a Z value that names it is not it)
            rec(0, 1300, [(H, 3), (M, 50), (S, 2)], flag=2048 | 16, aux=sa_tag([e3, e1]) + EVERY_TYPE),
            rec(1, 5, [(M, 20)], aux=b"SAZ\0"),                                                     # an empty value: the own segment alone
            rec(2, 9, [(M, 1000), (D, 300), (M, 700)] * 3, aux=b"NMi\x01\x00\x00\x00" + sa_tag([e2]) + b"ASC\x07", cg=True, seed=3),
            rec(2, 10, [(M, 30)], aux=sa_tag([e1]), cg=True, seed=4),                               # one CG op: the placeholder stays
            rec(2, 11, [(S, 40), (N, 35)], aux=cg_then_sa)]                                         # SA behind the CG tag
    out["aux"] = (write(tmp_path / "a.bam", raws), {0: [e1], 1: [e1, e2, e3], 3: [e3, e1], 4: [], 5: [e2], 6: [e1], 7: [e3]},
                  [0, 16, 0, 2048 | 16, 0, 0, 0, 0], 0, None)
    e, f = (0, 5001, "+", "100S50M"), (1, 901, "+", "100S50M")
    raws = [rec(1, 700, [(M, 100), (S, 50)], aux=sa_tag([f])), rec(0, 4000, [(M, 100), (S, 50)], aux=sa_tag([e])),
            rec(0, 30, [(M, 10)]), rec(0, 4000, [(M, 90), (S, 60)], flag=16, aux=sa_tag([e, e])), rec(0, 12, [(S, 5), (M, 10)], aux=sa_tag([e]))]
    # sorted: (0, 12) (0, 30) (0, 4000: the first in the file) (0, 4000: the second) (1, 700)
    out["unsorted"] = (write(tmp_path / "u.bam", raws), {0: [e], 2: [e], 3: [e, e], 4: [f]}, [0, 0, 0, 16, 0], 0, None)

    def entry(k):
        return (0, 100 + 20000 * k + 301, "+", "100S50M")
    raws = [rec(0, 100 + 20000 * k, [(M, 100), (S, 50)], aux=sa_tag([entry(k)])) for k in range(5)]
    raws += [rec(1, 50, [(M, 100), (S, 50)], aux=sa_tag([entry(0)]))]
    path = write(tmp_path / "r.bam", raws)
    write_bai(path, raws, {0: {0: 0, 1: 1, 2: 2, 3: 3, 4: 4}, 1: {0: 5}})
    out["whole"] = (path, {**{k: [entry(k)] for k in range(5)}, 5: [entry(0)]}, None, 0, None)
    # from the 16-kb window of (contig 1, 40 000) up to, excluding, (contig 1, 70 000): the records at 40 100 and
    # 60 100, numbered from 0
    out["region"] = (path, {0: [entry(2)], 1: [entry(3)]}, None, 0, (0, 40000, 0, 70000))
    good = (0, 100, "+", "50M")
    raws = []
    for k, bad in enumerate(MALFORMED):
        raws.append(rec(0, 10 * k, [(M, 20)], aux=b"XXi\x01\x00\x00\x00" + b"SAZ" + bad + b"\0"))
        raws.append(rec(0, 10 * k + 5, [(M, 20), (S, 5)], aux=sa_tag([good])))
    raws.append(rec(0, 5000, [(M, 20)], aux=b"SAZchr1,100,+,50M,60,1;"))      # the value runs off the record: no tag found
    out["malformed"] = (write(tmp_path / "m.bam", raws), {2 * k + 1: [good] for k in range(len(MALFORMED))}, None, len(MALFORMED), None)
    return out


MALFORMED = [b"chr1,100,+,50M,60;", b"chr1,100,+,50M,60,1,9;", b"chr1,100,+,50M,60,1", b"chr9,100,+,50M,60,1;", b"chr1,100,+,,60,1;",
             b"chr1,100,+,*,60,1;", b"chr1,100,+,50,60,1;", b"chr1,100,+,M,60,1;", b"chr1,100,+,50Q,60,1;", b"chr1,0,+,50M,60,1;",
             b"chr1,-5,+,50M,60,1;", b"chr1,,+,50M,60,1;", b"chr1,100,*,50M,60,1;", b"chr1,100,+-,50M,60,1;", b"chr1,100,,50M,60,1;",
             b",100,+,50M,60,1;", b"chr1,100,+,50M,60,1;chr1,200,+,50M", b"chr1,100,+,50M,,1;", b"chr1,100,+,50M,60,;",
             b"chr1,4294967296,+,50M,60,1;", b"chr1,2147483647,+,4294967295M,60,1;", b"chr1,100,+,50M,x,1;", b";"]


def test_positions_entries_strands_and_aux_fields_around_sa(tmp_path):
    pl, (read, off, seg) = read_table(*files(tmp_path)["aux"])
    assert read.tolist() == [0, 1, 3, 4, 5, 6, 7] and off.tolist() == [0, 2, 6, 9, 10, 12, 14, 16]
    # written out: the reverse-strand record's own segment starts at its trailing clip, the CG records' come
    # from the restored CIGAR, and the SA rows are 0-based
    assert tuple(seg[2]) == (0, 1, 1100, 1240, 7, 132) and tuple(seg[3]) == (0, 0, 2300, 2850, 1000, 1535)
    assert tuple(seg[4]) == (1, 1, 0, 19, 9, 22) and tuple(seg[10]) == (2, 0, 9, 6009, 0, 5100)
    assert tuple(seg[12]) == (2, 0, 10, 40, 30, 30) and tuple(seg[14]) == (2, 0, 11, 56, 0, 40)
    assert tuple(seg[15]) == (2, 1, 76, 86, 0, 10)


def test_unsorted_file_indices_follow_the_sort(tmp_path):
    pl, (read, off, seg) = read_table(*files(tmp_path)["unsorted"])
    assert pl.pos.tolist() == [12, 30, 4000, 4000, 700] and read.tolist() == [0, 2, 3, 4] and off.tolist() == [0, 2, 4, 7, 9]


def test_region_read(tmp_path):
    f = files(tmp_path)
    whole, _ = read_table(*f["whole"])
    assert whole.n_reads == 6
    pl, (read, off, seg) = read_table(*f["region"])
    assert pl.pos.tolist() == [40100, 60100] and read.tolist() == [0, 1]


def test_every_malformed_shape_is_counted_and_dropped(tmp_path):
    n = len(MALFORMED)
    pl, (read, off, seg) = read_table(*files(tmp_path)["malformed"])
    assert pl.n_reads == 2 * n + 1 and read.tolist() == [2 * k + 1 for k in range(n)]


def test_cpu_backend_cli_refuses_split_reads(tmp_path):
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_cpu", "svtrek_cpu")
    path = files(tmp_path)["aux"][0]
    p = subprocess.run([cli, "call", "-b", path, "--split-reads"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode != 0 and "not supported by this backend" in p.stderr and p.stdout == ""
