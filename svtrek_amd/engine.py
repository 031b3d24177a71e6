"""Python host mirror of the reference's per-record refinement calls, over the C ABI.

`Engine.refine(loci)` is the batched form of what thread_func (reference
audit.c:175-232) does per record through deletion()/insertion()/inversion()
(refinement.c:327-339): same parameters (t_arg's six refinement fields,
params.h:81-87, defaults params.h:27-32), same result encoding (0xFFFFFFFF = the
reference's -1 "not refined").  Every call runs the HIP engine; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import (CALL_DTYPE, EVIDENCE_DTYPE, GT_DTYPE, GT_SITE_DTYPE, JUNCTION_SEG_DTYPE, LOCUS_DTYPE, POA_RESULT_DTYPE, RESULT_DTYPE,
                   STATUS_NAMES, SVT_DEL, SVT_DUP, SVT_EINVAL, SVT_INS, SVT_INV, SVT_NA, SW_QUERY_DTYPE, SW_WINDOW_DTYPE, SvtCallBndStats, SvtCallConsensusStats, SvtCallRearrStats,
                   SvtCallJunctionStats, SvtCallMergeStats, SvtCallParams, SvtCallSplitStats, SvtCallStats, SvtGtParams, SvtInsseqView, SvtJunctionView, SvtLoadStats, SvtParams, SvtPoaParams,
                   SvtWork, has_call, has_call_merge, has_call_split, has_callseq, has_evidence, has_bnd, has_genotype, has_junctions, has_rearr, load_engine, ptr)
from .pileup import Pileup

# params.h:27-32
WIDER_INTERVAL = 20000
MEDIAN_INTERVAL = 10000
NARROW_INTERVAL = 2000
CONSENSUS_INTERVAL_RANGE = 500
CONSENSUS_INTERVAL = 5
CONSENSUS_MIN_COUNT = 3


@dataclass
class Params:
    wider_interval: int = WIDER_INTERVAL
    median_interval: int = MEDIAN_INTERVAL
    narrow_interval: int = NARROW_INTERVAL
    consensus_interval_range: int = CONSENSUS_INTERVAL_RANGE
    consensus_interval: int = CONSENSUS_INTERVAL
    consensus_min_count: int = CONSENSUS_MIN_COUNT
    spill_bytes: int = 0

    def to_c(self) -> SvtParams:
        return SvtParams(self.wider_interval, self.median_interval, self.narrow_interval,
                         self.consensus_interval_range, self.consensus_interval, self.consensus_min_count,
                         self.spill_bytes)


class SvtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"svt error {code} ({STATUS_NAMES.get(code, '?')}): {msg}")
        self.code = code


class Engine:
    """One GPU context (svt_ctx).  Use one Engine per process/GPU."""

    def __init__(self, params: Params | None = None, device: int = -1, devices: list[int] | None = None,
                 lib: C.CDLL | None = None):
        """One context on `device` (-1 = current), or -- with `devices` -- one context over
        several GPUs (svt_open_multi: the pileup is replicated, host batches are split).
        lib: another library implementing include/svtrek_gpu.h, bound with _lib.bind_abi --
        only the tests pass one (oracle/libsvtrek_cpu.so, the CPU restatement, to run the
        same calls on both backends); by default the HIP engine, which must be built."""
        self.lib = lib if lib is not None else load_engine()
        self.params = params or Params()
        self._cp = self.params.to_c()
        h = C.c_void_p()
        if devices is not None:
            dv = (C.c_int * len(devices))(*devices)
            rc = self.lib.svt_open_multi(C.byref(self._cp), len(devices), dv, C.byref(h))
        else:
            rc = self.lib.svt_open(C.byref(self._cp), int(device), C.byref(h))
        if rc != 0:
            raise SvtError(rc, "svt_open failed (no HIP device, or consensus_min_count < 1)")
        self._h = h
        self._pileup = None

    @property
    def n_devices(self) -> int:
        return int(self.lib.svt_device_count(self._h))

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise SvtError(rc, self.lib.svt_last_error(self._h).decode(errors="replace"))

    def load_pileup(self, pileup: Pileup) -> None:
        view = pileup.view()
        self._check(self.lib.svt_load_pileup(self._h, C.byref(view)))
        self._pileup = pileup

    def refine(self, loci: np.ndarray) -> np.ndarray:
        loci = np.ascontiguousarray(loci, dtype=LOCUS_DTYPE)
        out = np.empty(len(loci), dtype=RESULT_DTYPE)
        if len(loci):
            self._check(self.lib.svt_refine_batch(self._h, ptr(loci), len(loci), ptr(out)))
        return out

    def refine_device(self, d_loci: int, n: int, d_out: int, stream: int | None = None) -> None:
        """Device pointers (e.g. torch tensor .data_ptr()) on a hipStream_t handle (int)."""
        self._check(self.lib.svt_refine_device(self._h, C.c_void_p(d_loci), n, C.c_void_p(d_out),
                                               C.c_void_p(stream or 0)))

    def refine_device_records(self, d_loci: int, n: int, d_rec: int, d_index: int | None = None,
                              index_base: int = 0, stream: int | None = None) -> None:
        """As refine_device, writing RECORD_DTYPE gather records {index, start, end, 0}."""
        self._check(self.lib.svt_refine_device_records(self._h, C.c_void_p(d_loci), n, C.c_void_p(d_index or 0),
                                                       int(index_base), C.c_void_p(d_rec), C.c_void_p(stream or 0)))

    def _need_evidence(self) -> None:
        if not has_evidence(self.lib):
            raise SvtError(SVT_EINVAL, "this backend does not export svt_evidence_batch / svt_evidence_device "
                                       "(include/svtrek_evidence.h): evidence needs the HIP engine")

    def evidence(self, loci: np.ndarray, refined: np.ndarray) -> np.ndarray:
        """Per-breakpoint evidence of refined calls (svt_evidence_batch, include/svtrek_evidence.h):
        EVIDENCE_DTYPE records {support, depth, lo, hi} of shape (n, 2) -- [:, 0] for
        refined["start"], [:, 1] for refined["end"]; {0, 0, NA, NA} where the value is NA."""
        self._need_evidence()
        loci = np.ascontiguousarray(loci, dtype=LOCUS_DTYPE)
        refined = np.ascontiguousarray(refined, dtype=RESULT_DTYPE)
        if len(refined) != len(loci):
            raise ValueError(f"evidence: {len(loci)} loci but {len(refined)} refined results")
        out = np.empty((len(loci), 2), dtype=EVIDENCE_DTYPE)
        if len(loci):
            self._check(self.lib.svt_evidence_batch(self._h, ptr(loci), ptr(refined), len(loci), ptr(out)))
        return out

    def evidence_device(self, d_loci: int, d_refined: int, n: int, d_out: int, stream: int | None = None) -> None:
        """svt_evidence_device on device pointers: d_out receives 2 * n EVIDENCE_DTYPE records."""
        self._need_evidence()
        self._check(self.lib.svt_evidence_device(self._h, C.c_void_p(d_loci), C.c_void_p(d_refined), n,
                                                 C.c_void_p(d_out), C.c_void_p(stream or 0)))

    # ---- discovery (include/svtrek_call.h): DEL / INS calls from the loaded pileup alone
    def _need_call(self) -> None:
        if not has_call(self.lib):
            raise SvtError(SVT_EINVAL, "this backend does not export svt_call_scan (include/svtrek_call.h): "
                                       "discovery needs the HIP engine")

    def _need_call_split(self) -> None:
        self._need_call()
        if not has_call_split(self.lib):
            raise SvtError(SVT_EINVAL, "this backend does not export svt_call_split_stats_get: splitting calls by "
                                       "length (len_permille) needs engine 0.29.0 or later")

    def _need_call_merge(self) -> None:
        self._need_call()
        if not has_call_merge(self.lib):
            raise SvtError(SVT_EINVAL, "this backend does not export svt_call_merge_stats_get: joining a read's "
                                       "fragments (merge_gap) needs engine 0.31.0 or later")

    def _need_junctions(self) -> None:
        self._need_call()
        if not has_junctions(self.lib):
            raise SvtError(SVT_EINVAL, "this backend does not export svt_load_junctions (include/svtrek_junction.h): "
                                       "calls from split alignments need the HIP engine 0.32.0 or later")

    def _need_rearr(self) -> None:
        self._need_junctions()
        if not has_rearr(self.lib):
            raise SvtError(SVT_EINVAL, "this backend does not export svt_call_rearr_stats_get (include/svtrek_rearr.h): "
                                       "DUP / INV calls need the HIP engine 0.33.0 or later")

    def _need_bnd(self) -> None:
        self._need_junctions()
        if not has_bnd(self.lib):
            raise SvtError(SVT_EINVAL, "this backend does not export svt_call_bnd_stats_get (include/svtrek_bnd.h): "
                                       "BND calls need the HIP engine 0.34.0 or later")

    def load_junctions(self, read, off, seg) -> None:
        """The segment table of the loaded pileup's records that carry an SA tag (svt_load_junctions,
        include/svtrek_junction.h): read uint64 [n] ascending pileup read indices, off uint64 [n + 1], seg
        JUNCTION_SEG_DTYPE rows, a record's own segment first.  host.read_bam(path, junctions=True) gives all three."""
        self._need_junctions()
        read = np.ascontiguousarray(read, dtype=np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        seg = np.ascontiguousarray(seg, dtype=JUNCTION_SEG_DTYPE)
        if len(off) != len(read) + 1 and not (len(read) == 0 and len(off) == 0):
            raise SvtError(SVT_EINVAL, "load_junctions: off has one entry more than read")
        if len(read) and int(off[-1]) != len(seg):
            raise SvtError(SVT_EINVAL, "load_junctions: off[-1] is not the number of segment rows")
        v = SvtJunctionView(len(read), ptr(read) if len(read) else None, ptr(off) if len(read) else None,
                            ptr(seg) if len(seg) else None)
        self._check(self.lib.svt_load_junctions(self._h, C.byref(v)))

    def call(self, link: int | None = None, min_support: int | None = None, types=("DEL", "INS"),
             len_permille: int | None = None, merge_gap: int | None = None, merge_min: int | None = None,
             junctions: bool = False, rearrangements=(), breakends: bool = False) -> np.ndarray:
        """Cluster the pileup's D > 50 / I >= 50 ops by start (svt_call_scan): CALL_DTYPE records in
        (chrom, pos, type, len) order.  link: the largest gap between neighbouring starts of one
        cluster (default 10); min_support: the fewest ops of a call (default consensus_min_count);
        len_permille: 1 .. 1000 cuts every start cluster where its sorted lengths step by more than
        max(link, len * len_permille / 1000), one call per allele (default 0: no split);
        merge_gap: 1 .. 2^20 joins a read's D (I) ops of at least merge_min bases (1 .. 50, default 20)
        that lie within merge_gap bases of each other into one item of their summed length before
        clustering -- 180D 5M 120D counts as one 300 bp deletion (default 0: single ops only);
        junctions: the DEL / INS items of split alignments (load_junctions) join the CIGAR items;
        rearrangements: "DUP" and / or "INV" (a sequence or a comma string) adds the tandem duplications /
        inversions that the split alignments of load_junctions show (include/svtrek_rearr.h) to the same
        list; `types` keeps naming DEL / INS only and may be empty then;
        breakends: adds the translocation breakends those split alignments show -- a next alignment on another
        contig -- as records of type SVT_BND (include/svtrek_bnd.h: end is the partner's position, _lib.call_mate
        reads the partner's chrom and the orientation from pad); `types` may be empty then too."""
        self._need_call()
        if breakends:
            self._need_bnd()
        rearr = rearr_type_bits(rearrangements)
        if rearr:
            self._need_rearr()
        if junctions:
            self._need_junctions()
        if len_permille:
            self._need_call_split()
        if merge_gap:
            self._need_call_merge()
        p = SvtCallParams()
        self.lib.svt_call_default_params(self._h, C.byref(p))
        if link is not None:
            p.link = int(link)
        if min_support is not None:
            p.min_support = int(min_support)
        p.types = call_type_bits(types)
        if rearr:   # (an older engine never sees the field)
            p.rearr = rearr
        if breakends:   # (likewise)
            p.bnd = 1
        if len_permille is not None:
            if not 0 <= int(len_permille) <= 0xffffffff:
                raise SvtError(SVT_EINVAL, "call: len_permille in [0, 1000]")
            p.len_permille = int(len_permille)
        if merge_gap is not None or merge_min is not None:
            self._need_call_merge()   # (an older engine never sees the two fields)
            for name, v in (("merge_gap", merge_gap), ("merge_min", merge_min)):
                if v is not None:
                    if not 0 <= int(v) <= 0xffffffff:
                        raise SvtError(SVT_EINVAL, "call: merge_gap in [0, 2^20], merge_min in [1, 50]")
                    setattr(p, name, int(v))
        if junctions:
            p.junctions = 1
        n = C.c_uint64(0)
        self._check(self.lib.svt_call_scan(self._h, C.byref(p), C.byref(n)))
        return self.call_fetch(0, n.value)

    def call_fetch(self, first: int, n: int) -> np.ndarray:
        """Calls [first, first + n) of the last scan (svt_call_fetch)."""
        self._need_call()
        out = np.empty(int(n), dtype=CALL_DTYPE)
        self._check(self.lib.svt_call_fetch(self._h, int(first), int(n), ptr(out) if n else None))
        return out

    def call_device(self) -> tuple[int, int]:
        """(device pointer, count) of the last scan's calls: valid until the next scan / load / close."""
        self._need_call()
        d = C.c_void_p()
        n = C.c_uint64(0)
        self._check(self.lib.svt_call_device(self._h, C.byref(d), C.byref(n)))
        return int(d.value or 0), int(n.value)

    def call_stats(self) -> dict:
        self._need_call()
        st = SvtCallStats()
        self._check(self.lib.svt_call_stats_get(self._h, C.byref(st)))
        return {k: (float(getattr(st, k)) if k == "scan_ms" else int(getattr(st, k))) for k, _ in SvtCallStats._fields_}

    def call_split_stats(self) -> dict:
        """{candidates, split, groups, big} of the last call(): all zero without len_permille."""
        self._need_call_split()
        st = SvtCallSplitStats()
        self._check(self.lib.svt_call_split_stats_get(self._h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in SvtCallSplitStats._fields_}

    def call_merge_stats(self) -> dict:
        """{fragments, runs, joined_items, items, build_ms} of the last call(): all zero without merge_gap."""
        self._need_call_merge()
        st = SvtCallMergeStats()
        self._check(self.lib.svt_call_merge_stats_get(self._h, C.byref(st)))
        return {k: (float(getattr(st, k)) if k == "build_ms" else int(getattr(st, k))) for k, _ in SvtCallMergeStats._fields_}

    def call_junction_stats(self) -> dict:
        """{records, segments, junctions, del_items, ins_items, other, skipped, build_ms} of the last call():
        all zero without junctions."""
        self._need_junctions()
        st = SvtCallJunctionStats()
        self._check(self.lib.svt_call_junction_stats_get(self._h, C.byref(st)))
        return {k: (float(getattr(st, k)) if k == "build_ms" else int(getattr(st, k))) for k, _ in SvtCallJunctionStats._fields_}

    def call_rearr_stats(self) -> dict:
        """{dup_items, inv_items, skipped, clusters, calls, build_ms} of the last call(): all zero without
        rearrangements."""
        self._need_rearr()
        st = SvtCallRearrStats()
        self._check(self.lib.svt_call_rearr_stats_get(self._h, C.byref(st)))
        return {k: (float(getattr(st, k)) if k == "build_ms" else int(getattr(st, k))) for k, _ in SvtCallRearrStats._fields_}

    def call_bnd_stats(self) -> dict:
        """{items, skipped, classes, clusters, groups, calls, build_ms} of the last call(): all zero without
        breakends."""
        self._need_bnd()
        st = SvtCallBndStats()
        self._check(self.lib.svt_call_bnd_stats_get(self._h, C.byref(st)))
        return {k: (float(getattr(st, k)) if k == "build_ms" else int(getattr(st, k))) for k, _ in SvtCallBndStats._fields_}

    # ---- consensus inserted sequence of the INS calls (include/svtrek_callseq.h)
    def _need_callseq(self) -> None:
        self._need_call()
        if not has_callseq(self.lib):
            raise SvtError(SVT_EINVAL, "this backend does not export svt_call_consensus (include/svtrek_callseq.h): "
                                       "the calls' consensus sequences need the HIP engine 0.30.0 or later")

    def call_consensus(self, first: int = 0, n: int | None = None, cap: int = 4096, **poa_kw):
        """(POA_RESULT_DTYPE per call, uint8 [n, cap] nt4 consensus bases) of calls [first, first + n) of the
        last call() -- n None: all from `first` on -- after load_insseq (svt_call_consensus): an INS call's
        record is {len, n_support, n_used, 0} and bases[j, :min(len, cap)] its consensus, a DEL call's
        {-1, 0, 0, 0}.  poa_kw: poa_params' fields (max_len, max_support, max_seqs, ...)."""
        self._need_callseq()
        first = int(first)
        if n is None:
            n = max(self.call_device()[1] - first, 0)
        n = int(n)
        res = np.zeros(n, dtype=POA_RESULT_DTYPE)
        out = np.zeros((n, cap), dtype=np.uint8)
        p = self.poa_params(**poa_kw)
        self._check(self.lib.svt_call_consensus(self._h, C.byref(p), first, n, int(cap), ptr(out) if out.size else None,
                                                ptr(res) if n else None))
        return res, out

    def call_consensus_stats(self) -> dict:
        """{items, reach, ins_calls, window_items, window_max, deferred, table_ms, gather_ms, poa_ms} of the
        last call_consensus()."""
        self._need_callseq()
        st = SvtCallConsensusStats()
        self._check(self.lib.svt_call_consensus_stats_get(self._h, C.byref(st)))
        return {k: (float(getattr(st, k)) if k.endswith("_ms") else int(getattr(st, k)))
                for k, _ in SvtCallConsensusStats._fields_}

    # ---- genotypes (include/svtrek_genotype.h): alt / ref / spanning reads and GT, GQ, PL per site
    def gt_params(self, flank: int | None = None, costs=None) -> SvtGtParams:
        """svt_genotype_default_params with `flank` and `costs` = (ref_cost, alt_cost), three
        milli-phred values each (gt_costs(err) makes them), where given."""
        if not has_genotype(self.lib):
            raise SvtError(SVT_EINVAL, "this backend does not export svt_genotype_batch (include/svtrek_genotype.h): "
                                       "genotypes need the HIP engine")
        p = SvtGtParams()
        self.lib.svt_genotype_default_params(self._h, C.byref(p))
        if flank is not None:
            p.flank = int(flank)
        if costs is not None:
            ref_cost, alt_cost = costs
            for g in range(3):
                p.ref_cost[g], p.alt_cost[g] = int(ref_cost[g]), int(alt_cost[g])
        return p

    def genotype(self, sites: np.ndarray, flank: int | None = None, costs=None) -> np.ndarray:
        """GT_DTYPE records of GT_SITE_DTYPE sites (svt_genotype_batch); calls_to_sites and
        sites_from_loci make sites."""
        p = self.gt_params(flank, costs)
        sites = np.ascontiguousarray(sites, dtype=GT_SITE_DTYPE)
        out = np.empty(len(sites), dtype=GT_DTYPE)
        self._check(self.lib.svt_genotype_batch(self._h, C.byref(p), ptr(sites) if len(sites) else None, len(sites),
                                                ptr(out) if len(sites) else None))
        return out

    def genotype_device(self, d_sites: int, n: int, d_out: int, flank: int | None = None, costs=None,
                        stream: int | None = None) -> None:
        """svt_genotype_device on device pointers: n GT_SITE_DTYPE sites in, n GT_DTYPE records out."""
        p = self.gt_params(flank, costs)
        self._check(self.lib.svt_genotype_device(self._h, C.byref(p), C.c_void_p(d_sites), n, C.c_void_p(d_out),
                                                 C.c_void_p(stream or 0)))

    def genotype_calls(self, flank: int | None = None, costs=None) -> np.ndarray:
        """GT_DTYPE records of the last call()'s calls, genotyped where they lie on the device
        (svt_genotype_calls); record k belongs to call k."""
        p = self.gt_params(flank, costs)
        n = self.call_device()[1]
        out = np.empty(n, dtype=GT_DTYPE)
        self._check(self.lib.svt_genotype_calls(self._h, C.byref(p), ptr(out) if n else None, n))
        return out

    def reindex(self, stream: int | None = None) -> None:
        """Rebuild the device index of the loaded pileup on a hipStream_t handle (svt_reindex:
        asynchronous, no host work, results unchanged)."""
        self._check(self.lib.svt_reindex(self._h, C.c_void_p(stream or 0)))

    def bgzf_inflate(self, comp, blocks: np.ndarray, out_bytes: int | None = None) -> np.ndarray:
        """Inflate BGZF blocks on the device (svt_bgzf_inflate): comp = the compressed bytes,
        blocks = BGZF_BLOCK_DTYPE rows {coff, uoff, clen, ulen}; returns the uint8 output."""
        from ._lib import BGZF_BLOCK_DTYPE
        c = np.ascontiguousarray(np.frombuffer(comp, dtype=np.uint8) if isinstance(comp, (bytes, bytearray)) else comp,
                                 dtype=np.uint8)
        b = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK_DTYPE)
        if out_bytes is None:
            out_bytes = int((b["uoff"].astype(np.uint64) + b["ulen"]).max()) if len(b) else 0
        out = np.empty(max(out_bytes, 1), dtype=np.uint8)
        self._check(self.lib.svt_bgzf_inflate(self._h, c.ctypes.data, c.nbytes, b.ctypes.data, len(b),
                                              out.ctypes.data, out_bytes))
        return out[:out_bytes]

    def last_inflate_ms(self) -> float:
        return float(self.lib.svt_bgzf_last_inflate_ms(self._h))

    def sync(self, stream: int | None = None) -> None:
        self._check(self.lib.svt_sync(self._h, C.c_void_p(stream or 0)))

    def count_work(self, loci: np.ndarray) -> dict:
        loci = np.ascontiguousarray(loci, dtype=LOCUS_DTYPE)
        w = SvtWork()
        self._check(self.lib.svt_count_work(self._h, ptr(loci), len(loci), C.byref(w)))
        return {f: int(getattr(w, f)) for f, _ in SvtWork._fields_}

    def sliding_window_ins(self, queries: np.ndarray, window_size: int, slide_size: int,
                           with_subwindows: bool = False):
        """sliding_window_ins (reference sliding_window.c:8-97) for every query
        {chrom, start, end} (SW_QUERY_DTYPE): int32 bestCandidateOverall per query (-1 = none),
        plus, with `with_subwindows`, (offsets, SW_WINDOW_DTYPE per sub-window in order).
        Uses this engine's consensus_min_count."""
        q = np.ascontiguousarray(queries, dtype=SW_QUERY_DTYPE)
        best = np.empty(len(q), dtype=np.int32)
        sub = None
        off = None
        if with_subwindows:
            off = np.zeros(len(q) + 1, dtype=np.int64)
            ws = max(int(window_size), 1)
            span = q["end"].astype(np.int64) - q["start"].astype(np.int64)
            off[1:] = np.cumsum(np.where(span > 0, (span + ws - 1) // ws, 0))
            sub = np.empty(int(off[-1]), dtype=SW_WINDOW_DTYPE)
        self._check(self.lib.svt_sliding_window_ins(self._h, ptr(q), len(q), int(window_size), int(slide_size),
                                                    ptr(best), ptr(sub)))
        return (best, off, sub) if with_subwindows else best

    # ---- allele consensus (POA) of refined INS calls: no reference behaviour (the reference
    # never calls abPOA); parity against oracle/poa_oracle.c only.  See include/svtrek_gpu.h.
    @property
    def ins_count(self) -> int:
        """I >= 50 ops in the loaded pileup: the sequence count load_insseq expects."""
        return int(self.lib.svt_pileup_ins_count(self._h))

    def load_insseq(self, off: np.ndarray, bases: np.ndarray) -> None:
        off = np.ascontiguousarray(off, dtype=np.uint64)
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        v = SvtInsseqView(len(off) - 1, ptr(off), ptr(bases) if len(bases) else None)
        self._check(self.lib.svt_load_insseq(self._h, C.byref(v)))
        self._insseq = (off, bases)

    @staticmethod
    def poa_params(**kw) -> SvtPoaParams:
        p = SvtPoaParams()
        load_engine().svt_poa_default_params(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, int(v))
        return p

    def poa_consensus(self, loci: np.ndarray, refined: np.ndarray, cap: int = 4096, **kw):
        """(POA_RESULT_DTYPE per locus, uint8 [n, cap] nt4 consensus bases)."""
        loci = np.ascontiguousarray(loci, dtype=LOCUS_DTYPE)
        refined = np.ascontiguousarray(refined, dtype=RESULT_DTYPE)
        res = np.zeros(len(loci), dtype=POA_RESULT_DTYPE)
        out = np.zeros((len(loci), cap), dtype=np.uint8)
        p = self.poa_params(**kw)
        if len(loci):
            self._check(self.lib.svt_poa_consensus(self._h, C.byref(p), ptr(loci), ptr(refined), len(loci), cap,
                                                   ptr(out), ptr(res)))
        return res, out

    @property
    def poa_deferred(self) -> int:
        """Loci the last poa_consensus call reran on full-size scratch slots."""
        return int(self.lib.svt_poa_deferred(self._h))

    @property
    def device_bytes(self) -> int:
        return int(self.lib.svt_pileup_device_bytes(self._h))

    def load_stats(self) -> dict:
        """Timings (ms) of the last load_pileup: host pass, H2D copies, device index build."""
        st = SvtLoadStats()
        self._check(self.lib.svt_last_load_stats(self._h, C.byref(st)))
        return {k: (round(v, 3) if isinstance(v, float) else int(v))
                for k, v in ((k, getattr(st, k)) for k, _ in SvtLoadStats._fields_)}

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.lib.svt_close(self._h)
            self._h = None
        self._pileup = None   # the host arrays (a large pileup's memory) are no longer pinned here

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def call_type_bits(types) -> int:
    """svt_call_params.types of DEL / INS names (a comma-separated string or a sequence)."""
    names = types.split(",") if isinstance(types, str) else list(types)
    code = {"DEL": SVT_DEL, "INS": SVT_INS}
    bits = 0
    for t in names:
        if str(t).strip().upper() not in code:
            raise ValueError(f"call: unknown type {t!r} (DEL, INS)")
        bits |= 1 << code[str(t).strip().upper()]
    return bits


def rearr_type_bits(types) -> int:
    """svt_call_params.rearr of DUP / INV names (a comma-separated string or a sequence; empty: 0)."""
    names = [t for t in types.split(",") if t.strip()] if isinstance(types, str) else list(types)
    code = {"DUP": SVT_DUP, "INV": SVT_INV}
    bits = 0
    for t in names:
        if str(t).strip().upper() not in code:
            raise ValueError(f"call: unknown rearrangement {t!r} (DUP, INV)")
        bits |= 1 << code[str(t).strip().upper()]
    return bits


def calls_to_loci(calls: np.ndarray) -> np.ndarray:
    """CALL_DTYPE records as the LOCUS_DTYPE loci refine / evidence / audt take."""
    calls = np.asarray(calls, dtype=CALL_DTYPE)
    loci = np.empty(len(calls), dtype=LOCUS_DTYPE)
    for f in ("type", "chrom", "pos", "end"):
        loci[f] = calls[f]
    return loci


def calls_to_sites(calls: np.ndarray) -> np.ndarray:
    """CALL_DTYPE records as GT_SITE_DTYPE sites: the fields of the same names (a BND call passes through as a
    site of type SVT_BND, which no genotyper takes: the invalid record)."""
    calls = np.asarray(calls, dtype=CALL_DTYPE)
    sites = np.empty(len(calls), dtype=GT_SITE_DTYPE)
    for f in GT_SITE_DTYPE.names:
        sites[f] = calls[f]
    return sites


def sites_from_loci(loci: np.ndarray, refined: np.ndarray, radius: int = 10, len_tol: int | None = None) -> np.ndarray:
    """GT_SITE_DTYPE sites of an audited VCF's loci and their refined results.  The site spans
    [refined start, refined end] (INS: [start, start + 1]) and takes the items starting within
    `radius` of the refined start; a DEL's of a length within `len_tol` of end - start - 1 (any
    length when len_tol is None), an INS's of any length.  A locus of another type, or one whose
    refined start (DEL: or end) is NA, becomes an invalid site (type 0)."""
    loci = np.asarray(loci, dtype=LOCUS_DTYPE)
    refined = np.asarray(refined)
    if len(refined) != len(loci):
        raise ValueError(f"sites_from_loci: {len(loci)} loci but {len(refined)} refined results")
    start, end = refined["start"].astype(np.int64), refined["end"].astype(np.int64)
    is_del, is_ins = loci["type"] == SVT_DEL, loci["type"] == SVT_INS
    ok = (start != SVT_NA) & (is_ins | (is_del & (end != SVT_NA) & (end > start)))
    sites = np.zeros(len(loci), dtype=GT_SITE_DTYPE)
    sites["type"] = np.where(ok, loci["type"], 0)
    sites["chrom"] = loci["chrom"]
    sites["pos"] = np.where(ok, start, 0)
    sites["end"] = np.where(ok, np.where(is_del, end, start + 1), 0)
    sites["x_lo"] = np.where(ok, np.maximum(start - radius, 0), 1)   # (invalid besides: x_lo > x_hi)
    sites["x_hi"] = np.where(ok, start + radius, 0)
    dlen = end - start - 1
    if len_tol is None:
        lo, hi = np.zeros(len(loci), dtype=np.int64), np.full(len(loci), 0xFFFFFFFF, dtype=np.int64)
    else:
        lo, hi = np.maximum(dlen - len_tol, 0), np.minimum(dlen + len_tol, 0xFFFFFFFF)
    sites["len_lo"] = np.where(ok & is_del, lo, 0)
    sites["len_hi"] = np.where(ok & is_del, hi, 0xFFFFFFFF)
    return sites


def gt_costs(err: float = 0.05):
    """(ref_cost, alt_cost) of a per-read error rate: round(-10000 * log10 p) milli-phred per read under
    0/0, 0/1, 1/1, p = 1 - err, 0.5, err for a ref read and the reverse for an alt read."""
    import math
    if not 0.0 < err < 1.0:
        raise ValueError("gt_costs: err must lie in (0, 1)")
    ref = tuple(int(round(-10000.0 * math.log10(p))) for p in (1.0 - err, 0.5, err))
    return ref, ref[::-1]


def version() -> str:
    return load_engine().svt_version().decode()
