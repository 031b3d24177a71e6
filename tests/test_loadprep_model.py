"""The load's host pass (svtrek_amd/csrc/svt_loadprep.h) on the CPU: tests/native/loadprep_shim.cpp, built with
g++ alone, against the numpy model tests/loadprep_ref.py -- on the smallest shapes at which each part can go
wrong, every rejection with its message, and the thread cap at 1 and at 16."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loadprep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIM = R.LIMITS
KEYS = ("bkt_shift", "ncig_mask", "op_soft", "wave", "rcap", "t_min", "t_max", "ix_ranges", "group_ops", "threads")
ARRAYS = {"emax": (0, np.int32), "rec": (1, np.uint32), "clip8": (2, np.uint8), "bkt": (3, np.uint32), "bkt_off": (4, np.int64),
          "part": (5, np.uint64), "vtop": (6, np.int64), "nc": (7, np.uint32), "soff": (8, np.uint64), "words": (9, np.uint32)}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lp") / "loadprep_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "svtrek_amd", "csrc"), "-o", out,
                    os.path.join(ROOT, "tests", "native", "loadprep_shim.cpp")], check=True)
    lib = C.CDLL(out)
    lib.lp_prep.restype = lib.lp_stream_prep.restype = C.c_void_p
    lib.lp_prep.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    lib.lp_stream_prep.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
    lib.lp_error.restype = C.c_char_p
    lib.lp_bytes.restype = lib.lp_nops.restype = C.c_uint64
    lib.lp_n_ranges.restype = lib.lp_n_groups.restype = C.c_uint32
    for f in (lib.lp_error, lib.lp_n_ranges, lib.lp_n_groups, lib.lp_nops, lib.lp_free):
        f.argtypes = [C.c_void_p]
    lib.lp_bytes.argtypes = [C.c_void_p, C.c_int]
    lib.lp_copy.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.lp_seeded_digest.argtypes = [C.c_uint64, C.c_int, C.c_char_p, C.c_int]
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def _take(lib, h, names):
    try:
        err = lib.lp_error(h)
        if err is not None:
            raise R.Rejected(err.decode())
        out = {}
        for name in names:
            which, dt = ARRAYS[name]
            a = np.zeros(lib.lp_bytes(h, which) // np.dtype(dt).itemsize, dt)
            lib.lp_copy(h, which, _ptr(a))
            out[name] = a.reshape(-1, {"rec": 4, "bkt": 2}[name]) if name in ("rec", "bkt") else a
        out.update(n_ranges=lib.lp_n_ranges(h), n_groups=lib.lp_n_groups(h), nops=lib.lp_nops(h))
        return out
    finally:
        lib.lp_free(h)


def native_prep(lib, lim, tid_off, pos, endpos, nc, soff):
    L = np.array([lim[k] for k in KEYS], np.int64)
    nt = len(tid_off) - 1
    return _take(lib, lib.lp_prep(_ptr(L), nt, _ptr(tid_off), _ptr(pos), _ptr(endpos), _ptr(nc), _ptr(soff)),
                 ("emax", "rec", "clip8", "bkt", "bkt_off", "part", "vtop"))


def native_stream(lib, lim, tid_off, pos, endpos, cig_off, cigar, clip):
    L = np.array([lim[k] for k in KEYS], np.int64)
    nt = len(tid_off) - 1
    return _take(lib, lib.lp_stream_prep(_ptr(L), nt, _ptr(tid_off), _ptr(pos), _ptr(endpos), _ptr(cig_off), _ptr(cigar), _ptr(clip)),
                 ("nc", "soff", "words"))


def columns(per_contig, ops=1):
    """per_contig: per contig a list of (pos, endpos); every read `ops` ops (an int, or one count per read)."""
    tid_off = np.cumsum([0] + [len(c) for c in per_contig]).astype(np.int64)
    reads = [r for c in per_contig for r in c]
    pos = np.array([r[0] for r in reads], np.int32)
    endpos = np.array([r[1] for r in reads], np.int32)
    n = np.full(len(reads), ops, np.int64) if np.isscalar(ops) else np.asarray(ops, np.int64)
    soff = np.concatenate([[0], np.cumsum(np.maximum(n, 1))]).astype(np.uint64)
    return tid_off, pos, endpos, n.astype(np.uint32), soff


def agree(lib, lim, cols):
    want, got = R.prep(lim, *cols), native_prep(lib, lim, *cols)
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)), k
    assert got["part"][-1] == cols[0][-1] and len(got["part"]) == got["n_ranges"] + 1   # part ends in nr
    return got


def walk(n, step=100, length=150):
    return [(i * step, i * step + length) for i in range(n)]


PREP_CASES = {
    "no_contigs": lambda: columns([]),
    "three_empty_contigs": lambda: columns([[], [], []]),
    "one_read": lambda: columns([[(7, 9)]]),
    "pos_on_bucket_edge": lambda: columns([[(4095, 4200), (4096, 4300)]]),
    "endpos_on_bucket_edge": lambda: columns([[(10, 4096), (20, 4097)]]),        # the last bucket: the {nr, nr} sentinel
    "contained_reads": lambda: columns([[(0, 20000), (100, 300), (5000, 5100), (9000, 9500), (19000, 21000)]]),
    "cut_at_contig_starts": lambda: columns([walk(3), [], walk(2), walk(1)]),
    "cut_after_T_ops": lambda: columns([walk(40)], ops=100),                     # T at its floor of 2048: a cut every 21 reads
    "64_reads_one_group": lambda: columns([walk(64)]),
    "65_reads_two_groups": lambda: columns([walk(40), walk(25)]),
    "clip_bits": lambda: columns([walk(4)], ops=[1 | 1 << 30, 2 | 2 << 30, 3 | 3 << 30, 4]),
}


@pytest.mark.parametrize("name", list(PREP_CASES))
def test_prep_agrees_with_the_model(shim, name):
    cols = PREP_CASES[name]()
    if name == "clip_bits":   # (columns() sized the stream from nc with its clip bits: size it from the ops)
        cols = cols[:4] + (np.array([0, 1, 3, 6, 10], np.uint64),)
    got = agree(shim, LIM, cols)
    if name == "endpos_on_bucket_edge":
        assert got["bkt"].tolist() == [[0, 0], [2, 0], [2, 2]]
    if name == "cut_after_T_ops":
        assert got["part"].tolist() == [0, 21, 40]
    if name == "cut_at_contig_starts":
        assert got["part"].tolist() == [0, 3, 5, 6]
    if name.endswith("group") or name.endswith("groups"):
        assert got["n_groups"] == (1 if name.startswith("64") else 2)


def test_range_cut_after_rcap_reads(shim):
    got = agree(shim, dict(LIM, rcap=4), columns([walk(10), walk(3)]))
    assert got["part"].tolist() == [0, 4, 8, 10, 13]


def test_group_of_2_27_ops_turns_the_lane_index_off(shim):
    # (soff is synthetic: no stream is allocated, the pass never reads it)
    full = columns([walk(64)], ops=1 << 21)
    assert agree(shim, LIM, full)["n_groups"] == 0
    ops = np.full(64, 1 << 21)
    ops[-1] -= 1
    assert agree(shim, LIM, columns([walk(64)], ops=ops))["n_groups"] == 1


@pytest.mark.parametrize("threads", [1, 16])
def test_thread_cap_does_not_change_the_output(shim, threads):
    rng = np.random.default_rng(5)
    contigs = []
    for n in (300, 0, 1, 700, 64, 129):
        pos = np.sort(rng.integers(0, 200000, n))
        contigs.append([(int(p), int(p) + int(rng.integers(1, 30000))) for p in pos])
    cols = columns(contigs, ops=rng.integers(0, 40, sum(len(c) for c in contigs)))
    agree(shim, dict(LIM, threads=threads), cols)


def _bad(cols, **edit):
    names = ("tid_off", "pos", "endpos", "nc", "soff")
    cols = [c.copy() for c in cols]
    for k, (i, v) in edit.items():
        cols[names.index(k)][i] = v
    return tuple(cols)


BASE = columns([walk(5), walk(4)], ops=3)
PREP_REJECTIONS = {
    "unsorted": (_bad(BASE, pos=(7, 50)), "reads not sorted by pos within a contig"),       # contig 1: 0, 100, 50
    "negative_pos": (_bad(BASE, pos=(0, -1)), "pos < 0 or endpos <= pos"),
    "endpos_at_pos": (_bad(BASE, endpos=(3, 300)), "pos < 0 or endpos <= pos"),
    "offsets_go_back": (_bad(BASE, soff=(4, 5)), "bad cig_off"),
    "offset_past_the_stream": (_bad(BASE, soff=(8, 28)), "bad cig_off"),
    "offsets_disagree_with_nc": (_bad(BASE, nc=(2, 2)), "bad cig_off"),
}


@pytest.mark.parametrize("name", list(PREP_REJECTIONS))
def test_prep_rejections(shim, name):
    cols, message = PREP_REJECTIONS[name]
    agree(shim, LIM, BASE)   # (a contig's first read may lie before the last one of the contig before it)
    for f in (lambda: R.prep(LIM, *cols), lambda: native_prep(shim, LIM, *cols)):
        with pytest.raises(R.Rejected) as e:
            f()
        assert str(e.value) == message


# ---- the preamble of svt_load_pileup
S, M, D = 4, 0, 2
VIEW_TID = np.array([0, 3, 5], np.int64)
VIEW_POS = np.array([0, 10, 20, 5, 6], np.int32)
VIEW_END = VIEW_POS + 100
VIEW_WORDS = np.array([5 << 4 | S, 90 << 4 | M, 60 << 4 | D, 7 << 4 | S,  70 << 4 | M, 3 << 4 | S,  9 << 4 | S], np.uint32)


def view(cig_off, clip=None, words=VIEW_WORDS):
    return VIEW_TID, VIEW_POS, VIEW_END, np.array(cig_off, np.uint64), words, clip


def stream_agree(lib, v):
    nc, soff, words, nops = R.stream_prep(LIM, *v)
    got = native_stream(lib, LIM, *v)
    assert np.array_equal(got["nc"], nc) and np.array_equal(got["soff"], soff) and np.array_equal(got["words"], words)
    assert got["nops"] == nops
    return got


def test_clip_given_against_clip_from_the_words(shim):
    derived = stream_agree(shim, view([0, 2, 4, 6, 7, 7]))
    assert (derived["nc"] >> 30).tolist() == [2, 1, 1, 3, 0]
    given = stream_agree(shim, view([0, 2, 4, 6, 7, 7], clip=np.array([3, 0, 2, 1, 7], np.uint8)))
    assert (given["nc"] >> 30).tolist() == [3, 0, 2, 1, 3]
    assert (given["nc"] & LIM["ncig_mask"]).tolist() == [2, 2, 2, 1, 0]


def test_reads_without_ops_get_a_0M_word(shim):
    got = stream_agree(shim, view([0, 0, 2, 2, 4, 7]))
    assert got["soff"].tolist() == [0, 1, 3, 4, 6, 9] and got["nops"] == 7
    assert got["words"][[0, 3]].tolist() == [0, 0]
    whole = stream_agree(shim, view([0, 2, 4, 5, 6, 7]))   # every read has ops: the caller's arrays as they are
    assert whole["soff"].tolist() == [0, 2, 4, 5, 6, 7] and np.array_equal(whole["words"], VIEW_WORDS)


def test_preamble_without_contigs(shim):
    got = native_stream(shim, LIM, np.zeros(1, np.int64), None, None, None, None, None)
    assert len(got["nc"]) == 0 and got["nops"] == 0


ONE = np.ones(1, np.uint32)
STREAM_REJECTIONS = {
    "tid_off_from_1": ((np.array([1, 3, 5], np.int64),) + view([0, 2, 4, 6, 7, 7])[1:], "tid_off[0] != 0"),
    "tid_off_goes_back": ((np.array([0, 6, 5], np.int64),) + view([0, 2, 4, 6, 7, 7])[1:], "tid_off not monotone"),
    "no_pos": ((VIEW_TID, None) + view([0, 2, 4, 6, 7, 7])[2:], "missing arrays"),
    "no_endpos": ((VIEW_TID, VIEW_POS, None) + view([0, 2, 4, 6, 7, 7])[3:], "missing arrays"),
    "no_cig_off": ((VIEW_TID, VIEW_POS, VIEW_END, None, VIEW_WORDS, None), "missing arrays"),
    "no_cigar": (view([0, 2, 4, 6, 7, 7], words=None), "missing arrays"),
    "cig_off_from_1": (view([1, 2, 4, 6, 7, 7]), "cig_off[0] != 0"),
    "cig_off_goes_back": (view([0, 4, 2, 6, 7, 7]), "bad cig_off"),
    "cig_off_past_the_end": (view([0, 2, 4, 9, 7, 7]), "bad cig_off"),
    # (offsets alone say "more than NCIG_MASK ops": the clip bits are given and the words are never reached)
    "too_many_ops": (view([0, 2, 4, 6, 7, 7 + LIM["ncig_mask"] + 1], clip=np.zeros(5, np.uint8), words=ONE), "bad cig_off"),
}


@pytest.mark.parametrize("name", list(STREAM_REJECTIONS))
def test_preamble_rejections(shim, name):
    v, message = STREAM_REJECTIONS[name]
    for f in (lambda: R.stream_prep(LIM, *v), lambda: native_stream(shim, LIM, *v)):
        with pytest.raises(R.Rejected) as e:
            f()
        assert str(e.value) == message
