"""The junction classifier (svtrek_amd/csrc/svt_jnclass.h: jn_next + jn_classify) on the CPU:
tests/native/jnclass_shim.cpp, built with g++ alone, against junction_ref.junction, rearr_ref.rearrangement and
bnd_ref.breakend on the same rows -- the smallest cases at which each rule can go wrong, the 32-bit fields'
extremes, and a seeded table of 20 000 records on which every outcome occurs at least 100 times."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from svtrek_amd._lib import JUNCTION_SEG_DTYPE, SVT_DEL, SVT_DUP, SVT_INS, SVT_INV

import bnd_ref
import junction_ref
import rearr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the engine's SV_MIN_LENGTH, IX_SAT, CM_LEN_MAX and JN_EXT_MAX, as the refs have them
SAT, LEN_MAX, EXT_MAX = junction_ref.SAT, junction_ref.LEN_MAX, (1 << 31) - 1
LIM = np.array([50, SAT, LEN_MAX, EXT_MAX], np.int64)
NONE, DEL, INS, DUP, INV, BND = range(6)
FIELDS = ("have", "kind", "other", "past", "tid", "x", "len", "lo", "hi", "tid_hi", "y", "o")
SEED, RECORDS = 20250117, 20000
U32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jc") / "jnclass_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "svtrek_amd", "csrc"), "-o", out,
                    os.path.join(ROOT, "tests", "native", "jnclass_shim.cpp")], check=True)
    lib = C.CDLL(out)
    lib.jc_fields.restype = C.c_int
    lib.jc_classify.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.jc_table_size.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.jc_table_copy.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.jc_digest.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_int]
    assert lib.jc_fields() == len(FIELDS)
    return lib


def native(lib, off, seg):
    """[n] dicts of FIELDS: the shim's record of every table record."""
    n = len(off) - 1
    out = np.zeros((n, len(FIELDS)), np.int64)
    seg = np.ascontiguousarray(seg)
    lib.jc_classify(LIM.ctypes.data, n, off.ctypes.data, seg.ctypes.data, out.ctypes.data)
    return [dict(zip(FIELDS, r)) for r in out.tolist()]


def shim_table(lib, which):
    n, rows = C.c_uint64(), C.c_uint64()
    lib.jc_table_size(which, SEED, RECORDS, C.byref(n), C.byref(rows))
    off, seg = np.zeros(n.value + 1, np.uint64), np.zeros(rows.value, JUNCTION_SEG_DTYPE)
    lib.jc_table_copy(which, SEED, RECORDS, off.ctypes.data, seg.ctypes.data)
    return off, seg


def as_rows(seg):
    """The rows as dicts of Python ints: what the refs index, without numpy's scalar overhead."""
    names = seg.dtype.names
    return [dict(zip(names, r)) for r in seg.tolist()]


def table_of(records):
    off = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
    return off, np.array([s for r in records for s in r], dtype=JUNCTION_SEG_DTYPE).reshape(int(off[-1]))


def want(rows):
    """The record the shim must give for a record's rows, from the three refs alone."""
    z = dict.fromkeys(FIELDS, 0)
    j, r, b = junction_ref.junction(rows), rearr_ref.rearrangement(rows), bnd_ref.breakend(rows)
    if j is None:
        assert r is None and b is None
        return z
    z.update(have=1, other=int(j[0] == "other"))
    got = []
    A = rows[0]
    later = [s for s in rows if junction_ref._key(s) > junction_ref._key(A)]
    Bs = min(later, key=junction_ref._key)
    ext = dict(lo=min(min(A["r_beg"], Bs["r_beg"]), EXT_MAX), hi=min(max(A["r_end"], Bs["r_end"]), EXT_MAX))
    if j[0] in (SVT_DEL, SVT_INS):
        ty, tid, x, ln, lo, hi = j
        assert (min(lo, EXT_MAX), min(hi, EXT_MAX)) == (ext["lo"], ext["hi"])
        got.append(dict(kind=DEL if ty == SVT_DEL else INS, tid=tid, x=min(x, SAT), len=min(ln, LEN_MAX), past=int(x >= SAT), **ext))
    if r is not None:
        ty, tid, x, ln = r
        got.append(dict(kind=DUP if ty == SVT_DUP else INV, tid=tid, x=min(x, SAT), len=min(ln, LEN_MAX), past=int(x >= SAT), **ext))
    if b is not None:
        t_lo, x, t_hi, y, o = b
        got.append(dict(kind=BND, tid=t_lo, x=x, tid_hi=t_hi, y=y, o=o, past=int(x >= bnd_ref.SAT or y >= bnd_ref.SAT)))
    assert len(got) <= 1, "the three headers' rules partition the junctions"
    if got:
        z.update(got[0])
    return z


def outcome(w):
    if not w["have"]:
        return "no B"
    if w["kind"] != NONE:
        return ("DEL", "INS", "DUP", "INV", "BND")[w["kind"] - 1]
    return "other" if w["other"] else "none"


def agree(lib, records):
    off, seg = table_of(records)
    got, rows = native(lib, off, seg), as_rows(seg)
    wants = [want(rows[int(off[k]):int(off[k + 1])]) for k in range(len(records))]
    for k, (g, w) in enumerate(zip(got, wants)):
        assert g == w, (k, records[k])
    return wants


def seg(tid, strand, r_beg, r_end, q_beg, q_end):
    return (tid, strand, r_beg, r_end, q_beg, q_end)


def pair(strand, dr, dq, tid=0):
    """A and a later B of one contig and strand with the given dr and dq (A is Lf on strand +, Rt on -)."""
    A = seg(tid, strand, 100000, 101000, 500, 1500)
    Bq = (1500 + dq, 2500 + dq)
    if strand == 0:
        return [A, seg(tid, 0, 101000 + dr, 102000 + dr, *Bq)]
    return [A, seg(tid, 1, 99000 - dr, 100000 - dr, *Bq)]


EDGES = (49, 50, 51, -49, -50, -51)


@pytest.mark.parametrize("strand", [0, 1])
def test_dr_and_d_at_the_thresholds_on_both_strands(shim, strand):
    recs = [pair(strand, dr, dq) for dr in EDGES + (0, 1, -1) for dq in (0, 1, 2)]
    recs += [pair(strand, d + dq, dq) for d in EDGES for dq in (0, 1, 60, 200)]          # d at the thresholds
    recs += [pair(strand, dr, dr - d) for dr in EDGES for d in EDGES if dr - d > -400]   # both at once
    seen = {outcome(w) for w in agree(shim, recs)}
    assert {"DEL", "INS", "DUP", "none"} <= seen


@pytest.mark.parametrize("strand", [0, 1])
def test_dq_at_0_and_1(shim, strand):
    ws = agree(shim, [pair(strand, dr, dq) for dr in (-500, -50, -10, 0) for dq in (0, 1)])
    # dq = 0 is no INS and not `other`, a DUP stays a DUP
    assert [outcome(w) for w in ws[:4]] == ["DUP", "DUP", "none", "INS"]
    assert [w["other"] for w in ws[:2]] == [0, 1]


def inv_pair(sa, sb, w, a_first=True):
    """A and B of one contig on different strands whose joined coordinates p, q are w apart."""
    A = seg(2, sa, 50000, 51000, 0, 1000)
    p = 50000 if sa else 51000
    q = p + w if a_first else p - w
    Bs = seg(2, sb, q - 800, q, 1000, 1800) if sb else seg(2, sb, q, q + 800, 1000, 1800)
    return [A, Bs]


def test_the_four_inv_geometries_and_p_q_at_the_threshold(shim):
    recs = [inv_pair(sa, 1 - sa, w, first) for sa in (0, 1) for first in (True, False) for w in (0, 49, 50, 51, 3000)]
    ws = agree(shim, recs)
    assert [outcome(w) for w in ws[:5]] == ["other", "other", "other", "INV", "INV"]
    assert all(w["other"] for w in ws)


def test_the_four_bnd_orientations_from_both_read_strands_and_a_tid_above_b_tid(shim):
    fwd = {1: (seg(1, 0, 1000, 2000, 0, 1000), seg(5, 0, 7000, 8000, 1000, 2000)),
           0: (seg(1, 0, 1000, 2000, 0, 1000), seg(5, 1, 6000, 7000, 1000, 2000)),
           3: (seg(1, 1, 2000, 3000, 0, 1000), seg(5, 0, 7000, 8000, 1000, 2000)),
           2: (seg(1, 1, 2000, 3000, 0, 1000), seg(5, 1, 6000, 7000, 1000, 2000))}
    flip = lambda s, q0: (s[0], 1 - s[1], s[2], s[3], q0, q0 + (s[5] - s[4]))   # noqa: E731
    recs = []
    for o in range(4):
        A, Bs = fwd[o]
        recs += [[A, Bs], [flip(Bs, 0), flip(A, Bs[5] - Bs[4])]]   # the other strand's read: A.tid > B.tid
    ws = agree(shim, recs)
    for o in range(4):
        for w in ws[2 * o:2 * o + 2]:
            assert (w["kind"], w["tid"], w["x"], w["tid_hi"], w["y"], w["o"], w["other"]) == (BND, 1, 2000, 5, 7000, o, 1)


def test_no_later_tuple_equal_tuples_and_an_own_row_that_is_not_the_smallest(shim):
    A = seg(0, 0, 1000, 2000, 500, 1500)
    recs = [[A],
            [A, A],                                                    # equal tuples never pair
            [A, seg(0, 0, 5000, 6000, 0, 400)],                        # only an earlier tuple
            [A, seg(0, 0, 5000, 6000, 0, 400), seg(0, 0, 9000, 9500, 1500, 2000), seg(0, 0, 3000, 4000, 1500, 2000)],
            [A, seg(0, 0, 1000, 2000, 500, 1500 + 1)],                 # later by q_end alone
            [A, seg(1, 0, 1000, 2000, 500, 1500)],                     # by tid alone
            [A, seg(0, 0, 1001, 2000, 500, 1500)],                     # by r_beg alone
            [A, seg(0, 1, 1000, 2000, 500, 1500)]]                     # by strand alone
    ws = agree(shim, recs)
    assert [w["have"] for w in ws] == [0, 0, 0, 1, 1, 1, 1, 1]
    assert (ws[3]["kind"], ws[3]["x"], ws[3]["len"]) == (DEL, 2000, 1000)   # B is the (1500, 2000) row at 3000


def test_a_200_row_record_shuffled(shim):
    rnd = random.Random(7)
    A = seg(3, 0, 200000, 201000, 1000, 2000)
    rest = [seg(rnd.randrange(5), rnd.randrange(2), rnd.randrange(1, 400000), 400000 + rnd.randrange(1000),
                rnd.randrange(0, 4000), 4000 + rnd.randrange(100)) for _ in range(198)]
    rest.append(seg(3, 0, 201900, 202500, 2000, 2100))   # the B: q_beg 2000 is drawn above only with a q_end past 2100
    recs = []
    for _ in range(4):
        rnd.shuffle(rest)
        recs.append([A] + list(rest))
    ws = agree(shim, recs)
    assert all(w == ws[0] for w in ws) and ws[0]["have"]


def test_x_y_len_and_the_extents_at_their_clamps(shim):
    recs = []
    for x in (SAT - 1, SAT, SAT + 1):
        recs.append([seg(0, 0, x - 1000, x, 0, 1000), seg(0, 0, x + 700, x + 900, 1000, 1200)])            # DEL at x
        recs.append([seg(0, 0, x - 1000, x, 0, 1000), seg(0, 0, x, x + 900, 1300, 1500)])                  # INS at x
        recs.append([seg(0, 0, x + 500, x + 2000, 0, 1500), seg(0, 0, x, x + 900, 1500, 2400)])            # DUP at x
        recs.append([seg(0, 0, x - 1000, x, 0, 1000), seg(0, 1, x + 100, x + 5000, 1000, 5900)])           # INV at x (p = x, q beyond)
        recs.append([seg(0, 0, x - 1000, x, 0, 1000), seg(1, 0, 77, 500, 1000, 1423)])                     # BND, x at the limit
        recs.append([seg(0, 0, 500, 1000, 0, 500), seg(1, 0, x, x + 10, 500, 510)])                        # BND, y at the limit
    for ln in (LEN_MAX - 1, LEN_MAX, LEN_MAX + 1):
        recs.append([seg(0, 0, 0, 1000, 0, 1000), seg(0, 0, 1000 + ln, 2000 + ln, 1000, 2000)])            # DEL of len
        recs.append([seg(0, 0, 0, 1000, 0, 1000), seg(0, 0, 1000, 2000, 1000 + ln, 2000 + ln)])            # INS of len
        recs.append([seg(0, 0, ln + 60, ln + 4000, 0, 1000), seg(0, 0, 60, ln + 4060, 1000, 2000)])        # DUP: -dr = ln + 3940
        recs.append([seg(0, 0, 0, 1000, 0, 1000), seg(0, 1, 100, 1000 + ln, 1000, 2000)])                  # INV of len
    for e in (EXT_MAX - 1, EXT_MAX, EXT_MAX + 1, U32):
        recs.append([seg(0, 0, 0, 1000, 0, 1000), seg(0, 0, 2000, e, 1000, 2000)])                         # hi at e
        recs.append([seg(0, 0, e - 10, e, 0, 1000), seg(0, 0, min(e + 500, U32), U32, 1000, 2000)])        # lo at e - 10
        recs.append([seg(0, 0, e - 1, e, 0, 1000), seg(0, 1, e - 1, e, 1000, 2000)])
    ws = agree(shim, recs)
    assert [w["past"] for w in ws[:18]] == [0] * 6 + [1] * 12
    assert [w["len"] for w in ws[18:30:4]] == [LEN_MAX - 1, LEN_MAX, LEN_MAX]


def test_fields_at_0_and_at_2_32_minus_1_need_signed_64_bit_arithmetic(shim):
    V = (0, U32)
    recs = [[seg(0, sa, a0, a1, 0, 10), seg(tb, sb, b0, b1, q0, q1)]
            for sa in (0, 1) for sb in (0, 1) for tb in (0, 1) for a0 in V for a1 in V for b0 in V for b1 in V
            for q0, q1 in ((11, U32), (U32, U32), (0, 11), (0, U32))]
    seen = {outcome(w) for w in agree(shim, recs)}
    assert {"DEL", "DUP", "INV", "BND"} <= seen


def test_the_extreme_value_table(shim):
    off, seg_ = shim_table(shim, 1)
    got, rows = native(shim, off, seg_), as_rows(seg_)
    assert len(got) == 7 ** 4 * 12
    for k, g in enumerate(got):
        assert g == want(rows[int(off[k]):int(off[k + 1])]), k


def test_the_seeded_table_covers_every_outcome_and_agrees(shim):
    off, seg_ = shim_table(shim, 0)
    rows = as_rows(seg_)
    assert len(off) - 1 == RECORDS
    nrows = np.diff(off.astype(np.int64))
    assert nrows.min() == 1 and nrows.max() == 6
    wants = [want(rows[int(off[k]):int(off[k + 1])]) for k in range(RECORDS)]
    count = {}
    for w in wants:
        count[outcome(w)] = count.get(outcome(w), 0) + 1
    print(count)
    for name in ("no B", "none", "other", "DEL", "INS", "DUP", "INV", "BND"):   # from the refs alone, before any comparison
        assert count.get(name, 0) >= 100, (name, count)
    got = native(shim, off, seg_)
    for k, (g, w) in enumerate(zip(got, wants)):
        assert g == w, k
    # the flags against the counts of the refs' items()
    table = (np.arange(RECORDS), off, rows)
    _, jst = junction_ref.items(None, table)
    _, rst = rearr_ref.items(table)
    _, bst = bnd_ref.items(table)
    n = lambda kind: sum(1 for g in got if g["have"] and g["kind"] == kind)   # noqa: E731
    assert jst["junctions"] == sum(g["have"] for g in got)
    assert jst["other"] == sum(g["other"] for g in got)
    assert (jst["del_items"], jst["ins_items"]) == (n(DEL), n(INS))
    assert jst["skipped"] == sum(g["past"] for g in got if g["kind"] in (DEL, INS)) > 0
    assert (rst["dup_items"], rst["inv_items"]) == (n(DUP), n(INV))
    assert (bst["items"], bst["skipped"]) == (n(BND), sum(g["past"] for g in got if g["kind"] == BND))
    assert bst["skipped"] > 0
