"""The error exits of the host BAM reader (bam_ingest.cpp): a table of small crafted files -- damaged BGZF
framing, damaged BAM headers and records, missing and damaged BAIs -- read through every entry that can reach
the damage: host threads (1 and 4, libdeflate and zlib), the inflater callback and svth_bam_read_device (both
on the CPU backend), svth_bam_read_seq and svth_bam_read_sa.  Every read must fail with the message named in
ROWS.  tests/test_ingest_err_san.py reads the same files under ASan+UBSan with the leak checker on.

The zlib variant runs in one child process (the library picks its inflater once per process):
    python tests/test_ingest_errors.py DIR      # prints {row: {entry: message}} for the files written to DIR
"""
import ctypes as C
import gzip
import json
import os
import random
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from svtrek_amd import Engine, Params, host  # noqa: E402
from svtrek_amd._lib import bind_abi  # noqa: E402

import bamfix  # noqa: E402

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SHORT_BLOCK = bytes.fromhex("1f8b08040000000000ff060042430200130000 00".replace(" ", ""))   # bsize 20 < xlen + 20
NO_BC = bytes.fromhex("1f8b08040000000000ff0600585902001b0003000000000000000000")         # subfield XY, not BC


def header(n_ref=2, text=b"@HD\tVN:1.6\tSO:coordinate\n"):
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref)
    for t in range(n_ref):
        nm = b"chr%d\0" % (t + 1)
        hdr += struct.pack("<i", len(nm)) + nm + struct.pack("<i", 1 << 20)
    return hdr


def records(n=6):
    rng = random.Random(3)
    return [bamfix.record(k // 4, 100 + 10 * k, b"r%d" % k, [(0, 30), (1, 60), (0, 10)], 0, 100, b"NMi\x01\x00\x00\x00", False, rng)
            for k in range(n)]


def good_raw():
    return header() + b"".join(records())


def one_block(raw):
    """`raw` as one BGZF block, without the EOF block."""
    return bamfix.bgzf_blocks(raw)[:-len(EOF_BLOCK)]


def bai(n_ref=2, voff=0, magic=b"BAI\1", cut=0):
    out = magic + struct.pack("<i", n_ref)
    for _ in range(n_ref):
        out += struct.pack("<ii", 0, 1) + struct.pack("<Q", voff)
    return out[:len(out) - cut]


def cigar_past_end():
    r = bytearray(records(1)[0])
    r[16:18] = struct.pack("<H", 60000)   # n_cigar_op: 240 000 bytes of CIGAR in a record of < 200
    return bytes(r)


def damaged(blk, what):
    b = bytearray(blk)
    if what == "deflate":
        b[18] = 0x07                       # the first deflate block: final, of the reserved type 3
    else:
        b[-4:] = struct.pack("<I", struct.unpack("<I", b[-4:])[0] + 1)   # ISIZE one too large
    return bytes(b)


# name -> (file bytes, the .bai's bytes or None, region read?, the message of host threads, of the inflater callback (both
# through svth_bam_read_ex, and _seq and _sa for RECORD_ROWS) and of svth_bam_read_device; {path} is the BAM's path)
REGION = (0, 0, 1, 1 << 20)
GZ, BC, CUT = "not a BGZF file (bad gzip header)", "BGZF block without BC subfield", "truncated BGZF block at end of file"
INFLATE, ISIZE = "corrupt BGZF block (inflate failed)", "corrupt BGZF block 0 (does not inflate to its ISIZE)"
NOT_BAM, CUT_HDR, CUT_REFS, ONE_BATCH = "not a BAM file", "truncated BAM header", "truncated reference list", " (or longer than one batch)"
SMALL, CUT_REC, BAD_REC = "corrupt BAM record (block_size < 32)", "truncated BAM record", "corrupt BAM record"
BAD_BAI, PAST_END = "corrupt BAI: {path}.bai", "BAI offset past the end of the BAM"
GOOD = bamfix.bgzf_blocks(good_raw())
# The short block (BSIZE smaller than the block's own framing) is refused by the one block scan before any inflater sees
# it.  (The host threads used to take its length, wrapped to 2^64, to the inflater: "corrupt BGZF block (inflate failed)"
# alone, "not a BGZF file (bad gzip header)" when followed by zeros.)
ROWS = {
    "empty": (b"", None, False, NOT_BAM, NOT_BAM, "not a BAM file (no BGZF blocks)"),
    "not_gzip": (b"this is a text file, not a BAM\n", None, False, GZ, GZ, GZ),
    "no_fextra": (gzip.compress(good_raw()), None, False, GZ, GZ, GZ),
    "no_bc": (NO_BC, None, False, BC, BC, BC),
    "short_block": (SHORT_BLOCK, None, False, BC, BC, BC),
    "short_block_zeros": (SHORT_BLOCK + bytes(64), None, False, BC, BC, BC),
    "cut_block": (one_block(good_raw())[:-5], None, False, CUT, CUT, CUT),
    "bad_deflate": (damaged(one_block(good_raw()), "deflate") + EOF_BLOCK, None, False, INFLATE, ISIZE, NOT_BAM),
    "bad_isize": (damaged(one_block(good_raw()), "isize") + EOF_BLOCK, None, False, INFLATE, ISIZE, NOT_BAM),
    "bad_magic": (bamfix.bgzf_blocks(b"BAX\1" + good_raw()[4:]), None, False, NOT_BAM, NOT_BAM, NOT_BAM),
    "cut_text": (bamfix.bgzf_blocks(b"BAM\1" + struct.pack("<i", 1000) + b"@HD\tVN:1.6\n"), None, False,
                 CUT_HDR, CUT_HDR, CUT_HDR + ONE_BATCH),
    "neg_n_ref": (bamfix.bgzf_blocks(b"BAM\1" + struct.pack("<ii", 0, -3)), None, False, "bad n_ref", "bad n_ref", "bad n_ref"),
    "cut_ref_name": (bamfix.bgzf_blocks(header()[:-7]), None, False, CUT_REFS, CUT_REFS, CUT_REFS + ONE_BATCH),
    "small_block_size": (bamfix.bgzf_blocks(header() + struct.pack("<i", 16) + bytes(16)), None, False, SMALL, SMALL, SMALL),
    "cut_record": (bamfix.bgzf_blocks(good_raw()[:-7]), None, False, CUT_REC, CUT_REC,
                   "svt error -1 (EINVAL): truncated BAM record at end of file"),   # (the CPU backend's decoder)
    "cigar_past_end": (bamfix.bgzf_blocks(header() + records(2)[1] + cigar_past_end()), None, False, BAD_REC, BAD_REC, BAD_REC),
    "no_bai": (GOOD, None, True, "cannot open BAI: {path}.bai", "cannot open BAI: {path}.bai", None),
    "bai_magic": (GOOD, bai(magic=b"BAJ\1"), True, BAD_BAI, BAD_BAI, None),
    "bai_cut": (GOOD, bai(cut=5), True, BAD_BAI, BAD_BAI, None),
    "bai_past_end": (GOOD, bai(voff=(len(GOOD) + 1000) << 16 | 5), True, PAST_END, PAST_END, None),
}
RECORD_ROWS = ("small_block_size", "cut_record", "cigar_past_end")


def write_row(d, name):
    data, index, region = ROWS[name][:3]
    path = os.path.join(str(d), name + ".bam")
    with open(path, "wb") as f:
        f.write(data)
    if index is not None:
        with open(path + ".bai", "wb") as f:
            f.write(index)
    return path, REGION if region else None


def message(fn, path, **kw):
    """The message a read of `path` fails with, the path itself written {path}; None when it does not fail."""
    try:
        fn(path, **kw)
    except Exception as e:   # (OSError from the reader; the decoder's load reports through the engine's error type)
        return str(e).replace(path, "{path}")
    return None


def host_messages(path, region, name):
    out = {}
    for threads in (1, 4):
        out[f"host t{threads}"] = message(host.read_bam, path, threads=threads, region=region)
        if name in RECORD_ROWS:
            out[f"host t{threads} seq"] = message(host.read_bam, path, threads=threads, region=region, insseq=True)
            out[f"host t{threads} sa"] = message(host.read_bam, path, threads=threads, region=region, junctions=True)
    return out


def cpu_engine():
    return Engine(Params(), device=0, lib=bind_abi(C.CDLL(os.path.join(ROOT, "oracle", "libsvtrek_cpu.so"))))


@pytest.fixture(scope="module")
def cpu():
    eng = cpu_engine()
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def zlib_messages(tmp_path_factory):
    """host_messages of every row with SVTREK_NO_LIBDEFLATE set, from one child process."""
    d = tmp_path_factory.mktemp("zlib")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(d)], env=dict(os.environ, SVTREK_NO_LIBDEFLATE="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    return json.loads(p.stdout.decode())


@pytest.mark.parametrize("name", list(ROWS))
def test_read_fails_with_the_named_message(tmp_path, cpu, zlib_messages, name):
    path, region = write_row(tmp_path, name)
    want_host, want_callback, want_device = ROWS[name][3:]
    got = host_messages(path, region, name)
    got.update({"zlib " + k: v for k, v in zlib_messages[name].items()})
    want = {k: want_host for k in got}
    for k, kw in (("", {}), (" seq", {"insseq": True}), (" sa", {"junctions": True})) if name in RECORD_ROWS else (("", {}),):
        got["callback" + k] = message(host.read_bam, path, threads=3, region=region, inflate=cpu, batch_bytes=100, pinned=False, **kw)
        want["callback" + k] = want_callback
    if not region:   # (the device path reads whole files)
        got["device"] = message(lambda p, **kw: host.load_bam_device(cpu, p, **kw), path, threads=2, batch_bytes=100, pinned=False)
        want["device"] = want_device
    print(name, json.dumps(got, indent=1))
    assert None not in got.values()
    assert got == want


if __name__ == "__main__":
    rows = {}
    for name in ROWS:
        path, region = write_row(sys.argv[1], name)
        rows[name] = host_messages(path, region, name)
    print(json.dumps(rows))
