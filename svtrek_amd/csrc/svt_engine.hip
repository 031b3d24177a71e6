// svt_engine.hip -- MI355X (gfx950) SV-refinement engine: the one translation unit behind the C ABI of
// include/svtrek_gpu.h.  This file holds the shared constants and kernel argument structs, the
// context (svt_ctx), the launch logic and the core entry points; the device code and the host
// halves of the side modes are in the .inc files it includes.
//
// What a refine step does.  A locus has one window (INS) or two (DEL: refine_start, refine_end); a
// window's result is the reference's consensus_pos vote (refinement.c:41-101) over the breakpoint
// candidates its reads yield.
//   * At load, every candidate event of every read is filed once by the value it votes with, in
//     1 kb value buckets per contig and window kind (BkIndex); the per-read span lists (DevPileup's
//     spD / spI) are built beside them.
//   * refine_lane_kernel, the default: a wave takes 32 or 64 windows, reads each window's exact
//     vote band from its buckets, and votes one window per LANE (in-register sort, 16-bit offsets).
//   * Windows the lane path cannot take (band off or too full, positions past 2^30, ...) go on a list
//     for refine_redo_kernel: one wave per window, the buckets wave-wide, else the span-list
//     fallback (span walk, wave-wide sort + vote, a device spill pool past SVT_LDS_CANDS candidates).
//   * refine_span_kernel is that wave-per-window path for every window (small batches,
//     SVTREK_GATHER=span1); refine_kernel<true> is its counting build (svt_count_work).
// No floating point on the vote's values, no MFMA: integer filters and votes, bound by dependent loads.
//
// Which file holds what (in include order):
//   svt_wave.inc          wave primitives: ballots, readlanes, DPP scans, lane_xor, the PH() hooks
//   svt_gather.inc        candidate sink, region query, per-read replay, span walk, gather
//   svt_vote.inc          register / LDS sorts, band filter, consensus_pos and sliding votes, vote_window
//   svt_bucket.inc        the value buckets, refine side
//   svt_refine.inc        the wave-per-window kernels: refine_kernel, refine_span_kernel,
//                         refine_redo_kernel, sw_kernel, sw_reduce_kernel
//   svt_lane.inc          refine_lane_kernel and its helpers
//   svt_evidence.inc      read support, depth and value range per refined breakpoint
//   svt_call.inc          DEL / INS discovery from the value buckets (host side: svt_call_host.inc)
//   svt_genotype.inc      genotypes of DEL / INS sites (host side: svt_genotype_host.inc)
//   svt_callindex.inc     what the builds of svt_call_scan's derived indexes share: the filing step, the slot
//                         counters, the table's next-segment search (host side: svt_callindex_host.inc, the
//                         one build path of the three indexes below)
//   svt_callmerge.inc     a read's fragmented D / I ops joined into the merged index of svt_call_scan's
//                         merge_gap (host side: svt_callmerge_host.inc)
//   svt_junction.inc      DEL / INS items from split alignments filed beside the base view's events into the
//                         union index of svt_call_scan's junctions (host side: svt_junction_host.inc)
//   svt_rearr.inc         DUP / INV items from the same table in an index of their own, the scan's second
//                         pass over it and the merge of the two call lists (host side: svt_rearr_host.inc)
//   svt_bnd.inc           translocation breakends from the same table: an item list without buckets, radix
//                         sorts by (class, x) and by y, the BND calls (host side: svt_bnd_host.inc)
//   svt_index.inc, svt_index2.inc, svt_bucket_build.inc   the index builds (span lists, value buckets)
//   svt_poa.inc, svt_poa_host.inc      allele consensus (POA): kernels, slot pools and poa_run
//   svt_callseq.inc       consensus sequence of discovered INS calls: item table and support gather
//                         (host side: svt_callseq_host.inc)
//   svt_bam.inc, svt_inflate.inc, svt_bam_host.inc   BGZF inflate and BAM decode: kernels, svt_bam_dec_*
//   svt_devmem.inc        host only: DevBuf / DevEvent, the owners of every device allocation and event
//                         the host code makes, the pileup's three owners (ReadCols, SpanIndex, ValueBuckets) and
//                         the side modes' scratch records (CallScratch and its CallIndex, CallSeqScratch, PoaPool)
//   svt_loadprep.h        host only, no HIP: the load's host pass (validation, prefix-max endpos, records, read
//                         buckets, index ranges, groups) and svt_load_pileup's preamble
//   svt_load_host.inc     host only: the pileup load (svt_load_pileup, load_core for the BAM decoder), the
//                         span-list and value-bucket builds, svt_reindex, svt_last_load_stats
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <atomic>
#include <type_traits>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/svtrek_gpu.h"
#include "../../include/svtrek_evidence.h"
#include "../../include/svtrek_call.h"
#include "../../include/svtrek_genotype.h"
#include "../../include/svtrek_callseq.h"
#include "../../include/svtrek_junction.h"
#include "../../include/svtrek_rearr.h"
#include "../../include/svtrek_bnd.h"
#include "svt_bamrec.h"
#include "svt_loadprep.h"
#include "svt_jnclass.h"

#define SVT_VERSION "svtrek_amd 0.34.0 (gfx950, value-bucketed event index filed by a lane-per-read walk with a 9-B LDS stage, band + prefix-max facts, packed span walk fed by readlane, lane vote on 64 windows a wave, BGZF inflate + BAM decode, DEL/INS discovery from the value buckets, genotypes from the events' own read extents, consensus sequence of INS calls, a read's fragmented D / I ops joined before calling, DEL/INS items, DUP/INV calls and translocation breakends from split alignments)"

namespace {

constexpr int WAVE = 64;
constexpr int CAP = SVT_LDS_CANDS;          // LDS candidates per window
constexpr int SV_MIN_LENGTH = 50;           // params.h:33
constexpr uint32_t OP_INS = 1, OP_DEL = 2, OP_SOFT = 4;   // params.h:11-14
constexpr int K_START = 0, K_END = 1, K_INS = 2;          // refine_start / refine_end / refine_ins
constexpr int32_t T_INS = 1, T_DEL = 2;
constexpr int BKT_SHIFT = 12;               // read-start bucket = 4096 bp
constexpr uint32_t NCIG_MASK = 0x1fffffffu; // rec.z: n_cigar | clip << 30
constexpr uint32_t STREAM_PAD = 4096;       // zero words after the CIGAR stream (the index walks' slot over-read)
// Walk positions in the index saturate at IX_SAT.  The reference's uint32 reference_pos
// (refinement.c:118-145) cannot wrap before it passes a window end below 2^30 (one op
// advances it by < 2^28), so for every window with e < WEXACT "walk position <= e" and every
// candidate value are exact on saturated positions; windows ending at or past WEXACT take the
// per-read replay of the reference's uint32 arithmetic (walk_read).
constexpr uint32_t IX_SAT = 1u << 30;
constexpr uint32_t WEXACT = 1u << 30;
// Span events (svt_load_pileup, the index builds): every read's breakpoint events, 16 B each,
// self-contained {x, w, endpos, aux} so that a window is one filter over a contiguous span:
//   D list: D > 50 ops {walk position before the op, CIGAR word, endpos, 0} (refinement.c:124,:188),
//           SP_TRAIL {walk end, SP_TRAIL, endpos, 0} for cigar[n-1] == S (:120,:147),
//           SP_LEAD {pos, SP_LEAD, endpos, walk end} for cigar[0] == S (:210);
//   I list: I >= 50 ops {walk position before the op, CIGAR word, endpos, 0} (refinement.c:299).
constexpr uint32_t SP_TRAIL = 0xEu, SP_LEAD = 0xFu;   // op codes no candidate event carries

struct DevPileup {
    const int32_t *pos;       // [n_reads]
    const int32_t *emax;      // [n_reads] prefix max of endpos within the contig
    const uint4 *rec;         // [n_reads] {pos, endpos, n_cig | clip<<30, 0}
    const uint64_t *off64;    // [n_reads+1] read r's CIGAR = cigar[off64[r] .. off64[r] + n_cig)
    const int64_t *tid_off;   // [n_targets+1]
    const int64_t *bkt_off;   // [n_targets+1] start of each contig's bucket table
    const uint2 *bkt;         // {first read with pos >= b << BKT_SHIFT, first read with emax >= b << BKT_SHIFT}
    const uint32_t *cigar;    // the CIGAR stream (caller's words; one 0M word for n_cigar == 0 reads)
    const uint64_t *spoffD;   // [n_reads+1] span events: read r's D-list events are spD[spoffD[r] .. spoffD[r+1])
    const uint64_t *spoffI;   // [n_reads+1]              its I-list events spI[spoffI[r] .. spoffI[r+1])
                              // (= the I >= 50 ops before read r: the POA mode's sequence index)
    const uint4 *spD;
    const uint4 *spI;
    int32_t n_targets;
};

// The value-bucketed event index (svt_bucket.inc, svt_bucket_build.inc): per window kind one array
// of events filed by candidate value in 1 kb buckets per contig.
constexpr int BKS = 10;                                  // bucket = 1 kb of candidate value
constexpr int BA_S = 0, BA_E = 1, BA_I = 2, BA_L = 3, BA_N = 4;
struct BkIndex {
    const uint4 *ev;              // the events of the four arrays, S, E, I, L one after the other -- S: D > 50
                                  // + trailing S by x; E: D > 50 by x + len + 1, leading S by walk end + 1;
                                  // I: I >= 50 by x; L: leading S by read start
    const uint32_t *off;          // [BA_N][nbk + 1] first event (an index into ev) of every bucket
    const int32_t *pm;            // [3][nbk + 1] S, E, I: prefix max (within the contig) of the BELOW keys
    const uint64_t *cbase;        // [n_targets] contig t's first bucket
    const uint32_t *cnb;          // [n_targets] its buckets (the last one: every value past the others)
    const uint32_t *maxd;         // [n_targets] its longest D > 50 op (0: none)
    uint64_t nbk;                 // buckets per array (every contig's)
    int on;                       // built (SVTREK_INDEX=lists: 0, the span lists alone)
};

struct KParams {
    int32_t wider, median, narrow, range, ci, min_count;
    int32_t sw_window, sw_slide;   // sliding_window_ins mode only
    // refine_end's leading-S reads whose walk passes e (refinement.c:210-221) push the position
    // after the break op + 1 >= e + 2.  When e + 2 already lies at or past everything the vote
    // reads -- pos + range + max(ci, 0) and pos + 26 (narrow + 2 >= both widths) -- any value
    // >= e + 2 votes the same (see band_filter), so these reads count as one candidate at e + 2
    // and no stop search is needed; otherwise refine_end windows take the per-read replay.
    int32_t sent_ok;
};

struct KArgs {
    DevPileup pile;
    KParams prm;
    const svt_locus *loci;
    svt_result *out;
    uint32_t n;                 // loci
    int32_t *pool;              // spill slabs (int32 words)
    unsigned long long *pool_head;   // epoch << 40 | words handed out in that launch
    unsigned long long pool_words;
    uint32_t epoch;                  // this launch's pool epoch (1 .. 2^24-1)
    int32_t *status;            // bit0: spill pool exhausted
    unsigned long long *work;   // svt_work counters (COUNT builds only)
    const uint4 *sw_sub;        // sliding_window_ins mode: per sub-window {chrom, start, end, 0}
    int2 *sw_out;               //   per sub-window {bestCandidate, maxSupport}
    uint4 *rec_out;             // gather records {index, start, end, 0} instead of `out` (or null)
    const uint32_t *rec_index;  //   index of locus i: rec_index[i], or rec_base + i when null
    uint32_t rec_base;
    uint32_t *redo_list;        // lane-vote launches: windows left for refine_redo_kernel
    uint32_t *redo_ctr;         //   their count (this launch's counter)
    uint32_t *redo_next;        //   the next launch's counter (reset by refine_redo_kernel)
    BkIndex bk;                 // the value-bucketed event index
};

// svt_work counter slots (gather_window's wk[], the context's work words)
constexpr int W_WINDOWS = 0, W_READS = 1, W_OPS = 2, W_CANDS = 3, W_SPILLED = 4, W_QUERIES = 5, W_PROBE = 6,
              W_RANGE = 7, W_LREADS = 8, W_LENTRIES = 9, W_STOPS = 10, W_STOPCH = 11, W_SQUERIES = 12,
              W_SPAN = 13, W_BQ = 14, W_BEV = 15, W_N = 16;
// The context's control block (svt_ctx::d_ctl, CTL_BYTES of device memory) as the host addresses it: ctl(c)
// points at it, and the kernels get pointers to its words.
constexpr size_t CTL_BYTES = 256;
struct Ctl {
    unsigned long long pool_head;     // epoch << 40 | words handed out in that launch
    int32_t status;                   // the launches' sticky status (bit0: spill pool exhausted)
    uint32_t ix_status;               // the index builds' sticky status (take_ix_status)
    unsigned long long work[W_N];     // svt_work counters of a counting launch
    unsigned char unused[200 - 16 - 8 * W_N];
    uint32_t redo[4];                 // left-over counters: two alternating (direct launches), one + scratch (captured)
};
static_assert(offsetof(Ctl, pool_head) == 0 && offsetof(Ctl, status) == 8 && offsetof(Ctl, ix_status) == 12 &&
              offsetof(Ctl, work) == 16 && offsetof(Ctl, redo) == 200 && sizeof(Ctl) <= CTL_BYTES,
              "the control block's layout");

constexpr int LV_WMAX = 1023;   // band half-width for 16-bit offsets and prefix sums (32 * 2046 < 2^16)

#include "svt_wave.inc"
#include "svt_gather.inc"
#include "svt_vote.inc"
#include "svt_bucket.inc"
#include "svt_refine.inc"
#include "svt_lane.inc"
#include "svt_evidence.inc"
#include "svt_call.inc"
#include "svt_genotype.inc"
#include "svt_index.inc"
#include "svt_index2.inc"
#include "svt_bucket_build.inc"
#include "svt_callindex.inc"
#include "svt_callmerge.inc"
#include "svt_junction.inc"
#include "svt_rearr.inc"
#include "svt_bnd.inc"
#include "svt_poa.inc"
#include "svt_callseq.inc"
#include "svt_bam.inc"
#include "svt_inflate.inc"

#include "svt_devmem.inc"

// Everything that lives exactly as long as a loaded pileup: free_pileup is one assignment of a
// default-constructed Pileup.
struct Pileup {
    int32_t n_targets = 0;
    int64_t n_reads = 0;
    uint64_t n_ops = 0;
    uint64_t n_ins = 0;               // I >= 50 ops in the pileup (= I-list events; ix.d_spoffI indexes them per read)
    ReadCols reads;                   // the read columns
    SpanIndex ix;                     // the span-list index
    ValueBuckets bk;                  // the value-bucketed event index
    // allele-consensus mode: the inserted sequences (svt_load_insseq)
    DevBuf<uint64_t> d_ins_off;
    DevBuf<uint8_t> d_ins_bases;
    bool insseq_loaded = false;
    CallScratch call;                 // svt_call_scan
    CallSeqScratch callseq;           // svt_call_consensus
    uint64_t dev_bytes = 0;
    bool loaded = false;
};

}  // namespace

// ====================================================================== C ABI
struct svt_ctx : Pileup {
    svt_params prm{};
    int device = 0;
    bool lane_vote = true;        // refine_lane_kernel from 64K windows up; SVTREK_GATHER=span1: refine_span_kernel always
    uint64_t ix_ranges = 32768;   // index ranges per pileup (SVTREK_IX_RANGES, A/B): ~n_ops / this ops each,
                                  // at most IX_TMAX ops (and IX_RCAP reads) a range
    int lane_w = 0;               // SVTREK_LANE_W=32 forces the lane kernel at every batch size (tests)
    int lane_wide = -1;           // SVTREK_LANE_WIDE=0 / 1: 32 / 64 windows a wave at every size (-1: by window count)
    int ix_mode = 0;              // index build: 0 by read length, 1 lane per read (svt_index2.inc), 2 stream
                                  // walk (svt_index.inc) -- SVTREK_IX=auto|lane|stream
    bool bk_on = true;            // SVTREK_INDEX=lists: off (the span lists alone, rounds 1-5)
    DevBuf<uint32_t> d_redo;      // lane-vote launches: left-over window list (grown, never shrunk)
    uint32_t lane_par = 0;        // which of the two redo counters the next lane launch uses
    char err[512] = {0};
    svt_load_stats load_stats{};  // timings of the last svt_load_pileup
    // allele-consensus mode (svt_poa_consensus)
    PoaPool poa_small, poa_big;   // POA scratch slots (poa_pool)
    uint64_t poa_deferred = 0;    // loci the last svt_poa_consensus reran on full-size slots
    // batch scratch
    DevBuf<svt_locus> d_loci;
    DevBuf<svt_result> d_out;
    DevBuf<svt_evidence> d_evid;  // svt_evidence_batch's records [2 * n]
    DevBuf<svt_gt_site> d_gtsite; // svt_genotype_batch's sites
    DevBuf<svt_gt> d_gt;          // svt_genotype_batch's / svt_genotype_calls' records
    // spill pool (d_pool.cap() words) + status + work counters
    DevBuf<int32_t> d_pool;
    DevBuf<unsigned char> d_ctl;  // the control block (Ctl)
    uint32_t epoch = 0;           // launches so far (pool epochs cycle through 1 .. 2^24-1)
    // launches run in submission order across streams (order_on)
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    DevEvent order_ev;
    // svt_open_multi: the contexts of devices[1..] (this one drives devices[0])
    std::vector<svt_ctx *> subs;
    // BGZF inflate (svt_bgzf_inflate): device buffers grown on demand, never shrunk
    DevBuf<uint8_t> d_infc, d_info;
    DevBuf<svt_bgzf_block> d_infb;
    DevBuf<uint32_t> d_inferr;
    double inf_ms = 0;            // device time of the last svt_bgzf_inflate's kernel
};
static_assert(!std::is_copy_constructible<svt_ctx>::value && !std::is_copy_assignable<svt_ctx>::value,
              "a context owns its device memory");

namespace {

svt_status fail(svt_ctx *c, svt_status code, const char *fmt, const char *detail) {
    if (c) snprintf(c->err, sizeof c->err, fmt, detail ? detail : "");
    return code;
}

#define HIP_TRY(ctx, expr)                                                               \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) return fail((ctx), SVT_EDEVICE, #expr ": %s", hipGetErrorString(e_)); \
    } while (0)

Ctl *ctl(const svt_ctx *c) { return reinterpret_cast<Ctl *>(c->d_ctl.get()); }

// The index builds' sticky status word (and, with `launch`, the launches' beside it, in the same copy), read
// after the caller's synchronise and cleared when set: every build guard is reported once.  The
// codes: 1 emit overran the census's sizes / a count disagreed, 2 a look-back never ended, 3 an
// event outside its value bucket's extent; the caller words its own message.
svt_status take_ix_status(svt_ctx *c, uint32_t *code, int32_t *launch = nullptr) {
    static_assert(offsetof(Ctl, ix_status) == offsetof(Ctl, status) + 4, "one copy reads both status words");
    int32_t w[2] = {0, 0};
    HIP_TRY(c, hipMemcpy(w, &ctl(c)->status, sizeof w, hipMemcpyDeviceToHost));
    if (w[1]) HIP_TRY(c, hipMemset(&ctl(c)->ix_status, 0, 4));
    *code = (uint32_t)w[1];
    if (launch) *launch = w[0];
    return SVT_OK;
}

// A failed device allocation as the site's status: SVT_ENOMEM with its message.
svt_status nomem(svt_ctx *c, hipError_t e, const char *what) {
    return e == hipSuccess ? SVT_OK : fail(c, SVT_ENOMEM, "%s", what);
}

// Every entry point runs on its context's device and gives the calling thread its current
// device back (one host thread may drive contexts on several GPUs).
struct DevGuard {
    int prev = -1, dev;
    bool ok = true;
    explicit DevGuard(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DevGuard() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};
#define DEV_GUARD(ctx)                                                                    \
    DevGuard dg_((ctx)->device);                                                          \
    if (!dg_.ok) return fail((ctx), SVT_EDEVICE, "hipSetDevice(%s) failed", "ctx device")

// A context's launches share its spill pool (epoch-tagged head), sticky status and work
// counters, so they must not overlap: a launch on another stream than the previous one
// first waits for everything issued so far on that one.
svt_status order_on(svt_ctx *c, hipStream_t st) {
    if (c->have_last && st != c->last_stream) {
        if (!c->order_ev) HIP_TRY(c, c->order_ev.create(hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->order_ev, c->last_stream));
        HIP_TRY(c, hipStreamWaitEvent(st, c->order_ev, 0));
    }
    c->last_stream = st;
    c->have_last = true;
    return SVT_OK;
}

// After a launch reported the spill pool exhausted: the head word of that launch's epoch
// holds every word its spilled windows asked for (svt_refine_*'s CAS adds them even past
// the end); grow the pool to that, at least doubling it.
svt_status grow_pool(svt_ctx *c) {
    unsigned long long head = 0;
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(&head, &ctl(c)->pool_head, 8, hipMemcpyDeviceToHost));
    const uint64_t need = (uint32_t)(head >> 40) == c->epoch ? (head & ((1ull << 40) - 1ull)) : 0ull;
    const uint64_t words = std::max<uint64_t>(need + need / 8 + 1024, 2 * c->d_pool.cap());
    return nomem(c, c->d_pool.reserve(words), "growing the candidate spill pool failed");
}

void free_pileup(svt_ctx *c) { static_cast<Pileup &>(*c) = Pileup{}; }

// The loaded pileup as the kernels read it: the read columns and the span lists.
DevPileup pile_view(const svt_ctx *c) {
    DevPileup v;
    c->reads.view(v);
    c->ix.view(v);
    v.n_targets = c->n_targets;
    return v;
}

KArgs make_args(svt_ctx *c, const svt_locus *d_loci, svt_result *d_out, uint32_t n, bool count) {
    KArgs a;
    a.pile = pile_view(c);
    const svt_params &q = c->prm;
    // KParams::sent_ok: narrow + 2 >= max(range + max(ci, 0), 26) (64-bit: any int32 parameters)
    const int64_t width = std::max<int64_t>((int64_t)q.consensus_interval_range + std::max<int64_t>(q.consensus_interval, 0),
                                            SV_MIN_LENGTH / 2 + 1);
    a.prm = KParams{q.wider_interval, q.median_interval, q.narrow_interval, q.consensus_interval_range,
                    q.consensus_interval, q.consensus_min_count, 0, 0, (int64_t)q.narrow_interval + 2 >= width ? 1 : 0};
    a.loci = d_loci;
    a.out = d_out;
    a.n = n;
    a.pool = c->d_pool;
    a.pool_head = &ctl(c)->pool_head;
    a.pool_words = c->d_pool.cap();
    a.epoch = c->epoch;
    a.status = &ctl(c)->status;
    a.work = count ? ctl(c)->work : nullptr;
    a.sw_sub = nullptr;
    a.sw_out = nullptr;
    a.rec_out = nullptr;
    a.rec_index = nullptr;
    a.rec_base = 0;
    a.redo_list = nullptr;
    a.redo_ctr = a.redo_next = nullptr;
    a.bk = c->bk.view();
    return a;
}

svt_status launch(svt_ctx *c, const svt_locus *d_loci, svt_result *d_out, size_t n, hipStream_t st, bool count,
                  svt_record *rec_out = nullptr, const uint32_t *rec_index = nullptr, uint32_t rec_base = 0) {
    if (n == 0) return SVT_OK;
    if (n > 0x3fffffffull) return fail(c, SVT_EINVAL, "batch too large (%s)", "n > 2^30-1");
    svt_status s = order_on(c, st);
    if (s) return s;
    // A launch captured into a HIP graph (the caller's stream capture) is replayed with the
    // epoch and redo-counter parity of its capture, so its graph also clears the pool head and
    // its redo counter itself (two memset nodes); otherwise nothing per launch is reset.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (st) HIP_TRY(c, hipStreamIsCapturing(st, &cap));
    const bool captured = cap == hipStreamCaptureStatusActive;
    // no per-launch reset of the spill pool (epoch-tagged head; launches never overlap,
    // order_on); the work counters of a counting launch start from zero; the head word is
    // cleared once per epoch cycle
    c->epoch = c->epoch % ((1u << 24) - 1u) + 1u;
    if (c->epoch == 1 || captured) {   // a new epoch cycle (or every replay): the pool head starts from zero
        HIP_TRY(c, hipMemsetAsync(&ctl(c)->pool_head, 0, 8, st));
    }
    if (count) HIP_TRY(c, hipMemsetAsync(ctl(c)->work, 0, 8 * W_N, st));
    KArgs a = make_args(c, d_loci, d_out, (uint32_t)n, count);
    a.rec_out = reinterpret_cast<uint4 *>(rec_out);
    a.rec_index = rec_index;
    a.rec_base = rec_base;
    dim3 grid((unsigned)((2 * n + WPB - 1) / WPB)), block(64 * WPB);
    if (count) {
        hipLaunchKernelGGL((refine_kernel<true>), grid, block, 0, st, a);
    } else if (c->lane_vote && (c->lane_w != 0 || 2 * n >= (size_t)65536)) {
        // lane kernel (32 or 64 windows a wave) once the batch has >= 64K windows; below that the
        // one-wave-per-window span kernel is as fast or faster (fewer, longer waves leave the
        // chip underfilled: cfg2 20K windows 33 us span vs 76 us lane<8>, 107 us lane<32>;
        // cfg3 100K windows 111 vs 109 us; cfg4 2M windows 2.23 ms vs 0.905 ms)
        HIP_TRY(c, c->d_redo.reserve(2 * n));   // window list of the wave-wide left-overs
        // Two left-over counters alternate between direct lane launches: this launch appends to
        // ctr[par]; its redo kernel reads that and zeroes ctr[par ^ 1] for the next one.  The
        // parity advances on direct lane launches only (counting and span launches in between leave
        // both alone), and both start zeroed (svt_open).  A launch captured into a graph has its own
        // counter, ctr[2], zeroed by a memset node at the head of its graph, and its redo kernel's
        // "next" word is the scratch ctr[3]: replays run whenever the caller likes, so they must
        // neither read nor leave state the direct launches' alternation depends on.
        a.redo_list = c->d_redo;
        uint32_t *ctr = ctl(c)->redo;
        if (captured) {
            a.redo_ctr = ctr + 2;
            a.redo_next = ctr + 3;
            HIP_TRY(c, hipMemsetAsync(a.redo_ctr, 0, sizeof(uint32_t), st));
        } else {
            a.redo_ctr = ctr + c->lane_par;
            a.redo_next = ctr + (c->lane_par ^ 1u);
            c->lane_par ^= 1u;
        }
        // (16 windows a wave for the 250K-window launches of a 125K-locus shard measured slower:
        // 0.132-0.138 vs 0.117-0.121 ms, profiles/r04_sh)
        // 64 windows a wave (phase 2 on every lane) once the launch still fills the chip with them,
        // and whenever the lane kernel is forced; SVTREK_LANE_WIDE=0 / 1 overrides (A/B, tests)
        const bool wide = c->lane_wide >= 0 ? c->lane_wide != 0 : (c->lane_w != 0 || 2 * n >= LANE_WIDE_MIN);
        const unsigned per = WPB * (wide ? 64u : 32u);
        const dim3 lgrid((unsigned)((2 * n + per - 1) / per));
        if (wide) {
            if (c->bk.ready) hipLaunchKernelGGL((refine_lane_kernel<64, true>), lgrid, block, 0, st, a);
            else hipLaunchKernelGGL((refine_lane_kernel<64, false>), lgrid, block, 0, st, a);
        } else {
            if (c->bk.ready) hipLaunchKernelGGL((refine_lane_kernel<32, true>), lgrid, block, 0, st, a);
            else hipLaunchKernelGGL((refine_lane_kernel<32, false>), lgrid, block, 0, st, a);
        }
        hipLaunchKernelGGL(refine_redo_kernel, dim3(8192), block, 0, st, a);   // ~1 left-over window per wave
    } else {
        hipLaunchKernelGGL(refine_span_kernel, grid, block, 0, st, a);
    }
    HIP_TRY(c, hipGetLastError());
    return SVT_OK;
}

svt_status ensure_batch(svt_ctx *c, size_t n) {
    HIP_TRY(c, c->d_loci.reserve(n));
    HIP_TRY(c, c->d_out.reserve(n));
    return SVT_OK;
}

template <typename T>
svt_status upload(svt_ctx *c, DevBuf<T> &dst, const T *src, size_t n, size_t pad_elems = 0) {
    size_t bytes = (n + pad_elems) * sizeof(T);
    HIP_TRY(c, dst.reserve(std::max<size_t>(n + pad_elems, 1)));
    if (n) HIP_TRY(c, hipMemcpy(dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    if (pad_elems) HIP_TRY(c, hipMemset(dst + n, 0, pad_elems * sizeof(T)));
    c->dev_bytes += bytes;
    return SVT_OK;
}

#include "svt_poa_host.inc"

}  // namespace

extern "C" {

const char *svt_version(void) { return SVT_VERSION; }

const char *svt_last_error(const svt_ctx *ctx) { return ctx ? ctx->err : "null context"; }

svt_status svt_open(const svt_params *params, int device, svt_ctx **out) {
    if (!params || !out) return SVT_EINVAL;
    *out = nullptr;
    if (params->consensus_min_count < 1) return SVT_EINVAL;   // min_count <= 0 reads locations[-1]
    svt_ctx *c = new (std::nothrow) svt_ctx();
    if (!c) return SVT_ENOMEM;
    c->prm = *params;
    const char *g = getenv("SVTREK_GATHER");   // "span1": the one-wave-per-window kernel at every batch size
    c->lane_vote = !(g && strcmp(g, "span1") == 0);
    if (const char *x = getenv("SVTREK_IX")) c->ix_mode = strcmp(x, "lane") == 0 ? 1 : strcmp(x, "stream") == 0 ? 2 : 0;
    if (const char *x = getenv("SVTREK_IX_RANGES")) c->ix_ranges = std::max<uint64_t>(1, strtoull(x, nullptr, 10));
    if (const char *lw = getenv("SVTREK_LANE_W")) c->lane_w = atoi(lw) == 32 ? 32 : 0;
    if (const char *lw = getenv("SVTREK_LANE_WIDE")) c->lane_wide = atoi(lw) != 0 ? 1 : 0;
    if (const char *x = getenv("SVTREK_INDEX")) c->bk_on = strcmp(x, "lists") != 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        delete c;
        return SVT_EDEVICE;
    }
    if (device >= 0) {
        if (device >= ndev) { delete c; return SVT_EDEVICE; }
        c->device = device;
    } else {
        (void)hipGetDevice(&c->device);
    }
    DevGuard dg(c->device);
    if (!dg.ok) { delete c; return SVT_EDEVICE; }
    uint64_t pool_bytes = params->spill_bytes ? params->spill_bytes : (64ull << 20);
    if (c->d_pool.reserve(pool_bytes / 4) != hipSuccess || c->d_ctl.reserve(CTL_BYTES) != hipSuccess) {
        delete c;
        return SVT_ENOMEM;
    }
    (void)hipMemset(c->d_ctl, 0, CTL_BYTES);
    // load the code object now (HIP loads it lazily at the first launch), so that no later
    // call -- and no timing of one -- pays for it
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(index_kernel));
    *out = c;
    return SVT_OK;
}

svt_status svt_open_multi(const svt_params *params, int device_count, const int *devices, svt_ctx **out) {
    if (!params || !out || device_count < 1) return SVT_EINVAL;
    *out = nullptr;
    svt_ctx *c = nullptr;
    svt_status s = svt_open(params, devices ? devices[0] : 0, &c);
    if (s) return s;
    for (int i = 1; i < device_count; i++) {
        svt_ctx *d = nullptr;   // (a device may repeat: two independent contexts on one GPU)
        s = svt_open(params, devices ? devices[i] : i, &d);
        if (s) {
            svt_close(c);
            return s;
        }
        c->subs.push_back(d);
    }
    *out = c;
    return SVT_OK;
}

int svt_device_count(const svt_ctx *c) { return c ? 1 + (int)c->subs.size() : 0; }

// svt_open_multi: run fn(ctx_d, lo_d, hi_d) for the contiguous slices [lo_d, hi_d) of n items,
// one per device, concurrently (one host thread per extra device); the first failure's
// status and message are reported on the parent context.
extern "C++" template <typename F>
static svt_status for_devices(svt_ctx *c, size_t n, F fn) {
    const size_t D = 1 + c->subs.size();
    if (D == 1) return fn(c, (size_t)0, n);
    std::vector<svt_ctx *> ctx(D);
    ctx[0] = c;
    for (size_t d = 1; d < D; d++) ctx[d] = c->subs[d - 1];
    std::vector<svt_status> st(D, SVT_OK);
    const size_t per = (n + D - 1) / D;
    std::vector<std::thread> th;
    for (size_t d = 1; d < D; d++)
        th.emplace_back([&, d] { st[d] = fn(ctx[d], std::min(n, d * per), std::min(n, (d + 1) * per)); });
    st[0] = fn(c, 0, std::min(n, per));
    for (auto &t : th) t.join();
    for (size_t d = 0; d < D; d++)
        if (st[d] != SVT_OK) {
            if (d) snprintf(c->err, sizeof c->err, "device %d: %s", ctx[d]->device, ctx[d]->err);
            return st[d];
        }
    return SVT_OK;
}

static svt_status refine_device_any(svt_ctx *c, const svt_locus *d_loci, size_t n, svt_result *d_out,
                                    svt_record *d_rec, const uint32_t *d_index, uint32_t index_base, void *stream) {
    if (!c) return SVT_EINVAL;
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    if (n && (!d_loci || (!d_out && !d_rec))) return fail(c, SVT_EINVAL, "%s", "null loci/out");
    DEV_GUARD(c);
    return launch(c, d_loci, d_out, n, (hipStream_t)stream, false, d_rec, d_index, index_base);
}

svt_status svt_refine_device(svt_ctx *c, const svt_locus *d_loci, size_t n, svt_result *d_out, void *stream) {
    return refine_device_any(c, d_loci, n, d_out, nullptr, nullptr, 0, stream);
}

svt_status svt_refine_device_records(svt_ctx *c, const svt_locus *d_loci, size_t n, const uint32_t *d_index,
                                     uint32_t index_base, svt_record *d_rec, void *stream) {
    if (c && n && !d_rec) return fail(c, SVT_EINVAL, "%s", "null records");
    return refine_device_any(c, d_loci, n, nullptr, d_rec, d_index, index_base, stream);
}

svt_status svt_sync(svt_ctx *c, void *stream) {
    if (!c) return SVT_EINVAL;
    DEV_GUARD(c);
    HIP_TRY(c, hipStreamSynchronize((hipStream_t)stream));
    if (c->have_last && c->last_stream != (hipStream_t)stream) HIP_TRY(c, hipStreamSynchronize(c->last_stream));
    int32_t status = 0;
    uint32_t ixerr = 0;
    if (svt_status s = take_ix_status(c, &ixerr, &status)) return s;
    if (ixerr)   // the index build's guard fired: census and emit disagreed (an engine bug)
        return fail(c, SVT_EDEVICE, "%s",
                    ixerr == 2   ? "device index build: a look-back never ended (results invalid)"
                    : ixerr == 3 ? "device index build: an event outside its value bucket's extent (results invalid)"
                                 : "device index build: emit overran the census's sizes (results invalid)");
    if (status & 1) {
        HIP_TRY(c, hipMemset(&ctl(c)->status, 0, 4));   // sticky until reported
        const svt_status g = grow_pool(c);            // a re-run of the batch now fits
        if (g) return g;
        return fail(c, SVT_EOVERFLOW, "%s", "candidate spill pool exhausted (pool grown; re-run the batch)");
    }
    return SVT_OK;
}

// One synchronous launch over host loci on one device (count: the work-counting kernel);
// a launch whose spilled windows outgrew the pool is re-run once the pool has grown.
static svt_status run_batch_1(svt_ctx *c, const svt_locus *loci, size_t n, svt_result *out, svt_work *w) {
    if (n == 0) return SVT_OK;
    DEV_GUARD(c);
    svt_status s = ensure_batch(c, n);
    if (s) return s;
    HIP_TRY(c, hipMemcpy(c->d_loci, loci, n * sizeof(svt_locus), hipMemcpyHostToDevice));
    for (int attempt = 0;; attempt++) {
        s = launch(c, c->d_loci, c->d_out, n, nullptr, w != nullptr);
        if (s) return s;
        s = svt_sync(c, nullptr);
        if (s != SVT_EOVERFLOW || attempt == 3) break;
    }
    if (s) return s;
    if (out) HIP_TRY(c, hipMemcpy(out, c->d_out, n * sizeof(svt_result), hipMemcpyDeviceToHost));
    if (w) {
        unsigned long long k[W_N];
        HIP_TRY(c, hipMemcpy(k, ctl(c)->work, sizeof k, hipMemcpyDeviceToHost));
        w->windows = k[W_WINDOWS]; w->reads = k[W_READS]; w->ops_walked = k[W_OPS]; w->candidates = k[W_CANDS];
        w->spilled_windows = k[W_SPILLED]; w->queries = k[W_QUERIES]; w->probe_entries = k[W_PROBE];
        w->range_reads = k[W_RANGE]; w->list_reads = k[W_LREADS]; w->list_entries = k[W_LENTRIES];
        w->stop_searches = k[W_STOPS]; w->stop_chunk_words = k[W_STOPCH];
        w->span_bounds = k[W_SQUERIES]; w->span_events = k[W_SPAN];
        // algorithmic bytes of the span walk (DESIGN.md "Roofline"): locus in + result out, two
        // bucket words per search pair, the search entries, the two span bounds of a query and
        // its 16-B events, per stop search the chunk words scanned, the word before the break
        // chunk and its 8 CIGAR words
        w->bucket_queries = k[W_BQ];
        w->bucket_events = k[W_BEV];
        w->event_bytes = 24ull * n + 32ull * w->queries + 4ull * w->probe_entries + 36ull * w->stop_searches +
                         4ull * w->stop_chunk_words + 16ull * w->span_bounds + 16ull * w->span_events;
        // the value buckets (svt_bucket.inc): locus in + result out, per window two bucket offsets
        // and one prefix-max key, the 16-B events of its band's buckets and of the walks for ABOVE
        // (windows the buckets do not take -- none at the default parameters -- are not priced)
        if (c->bk.ready) w->event_bytes = 24ull * n + 12ull * w->bucket_queries + 16ull * w->bucket_events;
    }
    return SVT_OK;
}

svt_status svt_refine_batch(svt_ctx *c, const svt_locus *loci, size_t n, svt_result *out) {
    if (!c) return SVT_EINVAL;
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    if (n == 0) return SVT_OK;
    if (!loci || !out) return fail(c, SVT_EINVAL, "%s", "null loci/out");
    return for_devices(c, n, [&](svt_ctx *x, size_t lo, size_t hi) {
        return run_batch_1(x, loci + lo, hi - lo, out + lo, nullptr);
    });
}

svt_status svt_count_work(svt_ctx *c, const svt_locus *loci, size_t n, svt_work *out) {
    if (!c || !out) return SVT_EINVAL;
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    memset(out, 0, sizeof(*out));
    if (n == 0) return SVT_OK;
    if (!loci) return fail(c, SVT_EINVAL, "%s", "null loci");
    std::vector<svt_work> part(1 + c->subs.size());
    std::vector<svt_ctx *> who(part.size(), nullptr);
    const svt_status s = for_devices(c, n, [&](svt_ctx *x, size_t lo, size_t hi) {
        const size_t d = x == c ? 0 : (size_t)(std::find(c->subs.begin(), c->subs.end(), x) - c->subs.begin()) + 1;
        memset(&part[d], 0, sizeof(svt_work));
        return run_batch_1(x, loci + lo, hi - lo, nullptr, &part[d]);
    });
    if (s) return s;
    uint64_t *o = reinterpret_cast<uint64_t *>(out);
    for (const svt_work &p : part) {
        const uint64_t *q = reinterpret_cast<const uint64_t *>(&p);
        for (size_t i = 0; i < sizeof(svt_work) / 8; i++) o[i] += q[i];
    }
    return SVT_OK;
}

uint64_t svt_sw_subwindows(const svt_sw_query *q, int32_t window_size) {
    if (!q || window_size < 1 || q->end <= q->start) return 0;
    return ((uint64_t)(q->end - q->start) + (uint64_t)window_size - 1) / (uint64_t)window_size;
}

static svt_status sw_1(svt_ctx *c, const svt_sw_query *q, size_t n, int32_t window_size, int32_t slide_size,
                       int32_t *best, svt_sw_window *sub);

svt_status svt_sliding_window_ins(svt_ctx *c, const svt_sw_query *q, size_t n, int32_t window_size,
                                  int32_t slide_size, int32_t *best, svt_sw_window *sub) {
    if (!c) return SVT_EINVAL;
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    if (window_size < 1 || slide_size < 1)
        return fail(c, SVT_EINVAL, "%s", "window_size and slide_size must be >= 1 (the reference loops forever)");
    if (n == 0) return SVT_OK;
    if (!q || !best) return fail(c, SVT_EINVAL, "%s", "null queries/best");
    std::vector<uint64_t> soff(n + 1, 0);   // each query's first sub-window in `sub`
    for (size_t i = 0; i < n; i++) soff[i + 1] = soff[i] + svt_sw_subwindows(q + i, window_size);
    return for_devices(c, n, [&](svt_ctx *x, size_t lo, size_t hi) {
        return sw_1(x, q + lo, hi - lo, window_size, slide_size, best + lo, sub ? sub + soff[lo] : nullptr);
    });
}

static svt_status sw_1(svt_ctx *c, const svt_sw_query *q, size_t n, int32_t window_size, int32_t slide_size,
                       int32_t *best, svt_sw_window *sub) {
    if (n == 0) return SVT_OK;
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    std::vector<uint64_t> off(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        if ((uint64_t)q[i].end + (uint64_t)window_size > 0x100000000ull)
            return fail(c, SVT_EINVAL, "%s", "end + window_size > 2^32 (sub_start wraps, sliding_window.c:12)");
        off[i + 1] = off[i] + svt_sw_subwindows(q + i, window_size);
    }
    const uint64_t ns = off[n];
    if (ns > 0x3fffffffull) return fail(c, SVT_EINVAL, "%s", "more than 2^30-1 sub-windows in one call");
    std::vector<uint4> subs((size_t)ns);
    for (size_t i = 0; i < n; i++) {
        uint64_t k = off[i];
        for (uint32_t ss = q[i].start; ss < q[i].end; ss += (uint32_t)window_size, k++) {   // :12-15
            uint32_t se = ss + (uint32_t)window_size;
            subs[(size_t)k] = make_uint4((uint32_t)q[i].chrom, ss, se > q[i].end ? q[i].end : se, 0u);
        }
    }
    DEV_GUARD(c);
    svt_status so = order_on(c, nullptr);
    if (so) return so;
    DevBuf<uint4> d_sub;
    DevBuf<int2> d_res;
    DevBuf<uint64_t> d_off;
    DevBuf<int32_t> d_best;
    HIP_TRY(c, d_sub.reserve(std::max<size_t>(1, (size_t)ns)));
    HIP_TRY(c, d_res.reserve(std::max<size_t>(1, (size_t)ns)));
    HIP_TRY(c, d_off.reserve(n + 1));
    HIP_TRY(c, d_best.reserve(n));
    if (ns) HIP_TRY(c, hipMemcpy(d_sub, subs.data(), (size_t)ns * sizeof(uint4), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_off, off.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemsetAsync(c->d_ctl, 0, CTL_BYTES, nullptr));
    if (ns) {
        KArgs a = make_args(c, nullptr, nullptr, (uint32_t)ns, false);
        a.prm.sw_window = window_size;
        a.prm.sw_slide = slide_size;
        a.sw_sub = d_sub;
        a.sw_out = d_res;
        const dim3 grid((unsigned)((ns + WPB - 1) / WPB)), block(64 * WPB);
        hipLaunchKernelGGL(sw_kernel, grid, block, 0, nullptr, a);
        HIP_TRY(c, hipGetLastError());
    }
    hipLaunchKernelGGL(sw_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, d_res, d_off, (uint32_t)n,
                       d_best);
    HIP_TRY(c, hipGetLastError());
    if (svt_status s = svt_sync(c, nullptr)) return s;
    HIP_TRY(c, hipMemcpy(best, d_best, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (sub && ns) HIP_TRY(c, hipMemcpy(sub, d_res, (size_t)ns * sizeof(int2), hipMemcpyDeviceToHost));
    return SVT_OK;
}

// ---- allele-consensus mode (POA; no reference behaviour, see svt_poa.inc)
void svt_poa_default_params(svt_poa_params *p) {
    if (p) *p = svt_poa_params{2, 4, 4, 2, 10, 10, 32, 4000, 32768, 20, 64};
}

uint64_t svt_pileup_ins_count(const svt_ctx *c) { return c ? c->n_ins : 0; }

svt_status svt_load_insseq(svt_ctx *c, const svt_insseq_view *v) {
    if (!c || !v) return SVT_EINVAL;
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    if (v->n_ins != c->n_ins) return fail(c, SVT_EINVAL, "insseq: %s", "n_ins differs from the pileup's I >= 50 op count");
    if (v->n_ins >= (1ull << 31)) return fail(c, SVT_EINVAL, "insseq: %s", ">= 2^31 sequences");
    if (v->n_ins && (!v->off || !v->bases)) return fail(c, SVT_EINVAL, "insseq: %s", "missing arrays");
    if (v->n_ins && v->off[0] != 0) return fail(c, SVT_EINVAL, "insseq: %s", "off[0] != 0");
    for (uint64_t k = 0; k < v->n_ins; k++)
        if (v->off[k + 1] < v->off[k]) return fail(c, SVT_EINVAL, "insseq: %s", "off not monotone");
    DEV_GUARD(c);
    c->d_ins_off.reset();
    c->d_ins_bases.reset();
    c->insseq_loaded = false;
    const uint64_t nb = v->n_ins ? v->off[v->n_ins] : 0;
    svt_status s;
    if (v->n_ins) { if ((s = upload(c, c->d_ins_off, v->off, (size_t)v->n_ins + 1))) return s; }
    else if ((s = upload<uint64_t>(c, c->d_ins_off, nullptr, 0, 1))) return s;
    if (nb) { if ((s = upload(c, c->d_ins_bases, v->bases, (size_t)nb))) return s; }
    else if ((s = upload<uint8_t>(c, c->d_ins_bases, nullptr, 0, 1))) return s;
    c->insseq_loaded = true;
    return SVT_OK;
}

svt_status svt_poa_consensus(svt_ctx *c, const svt_poa_params *p, const svt_locus *loci, const svt_result *refined,
                             size_t n, int32_t cap, uint8_t *bases, svt_poa_result *res) {
    if (!c || !p) return SVT_EINVAL;
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    if (!c->insseq_loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_insseq not called");
    if (n == 0) return SVT_OK;
    if (!loci || !refined || !res || cap < 0 || (cap > 0 && !bases)) return fail(c, SVT_EINVAL, "%s", "null arrays / cap");
    if (n > 0x3fffffffull) return fail(c, SVT_EINVAL, "%s", "batch too large");
    if (!poa_params_ok(p)) return fail(c, SVT_EINVAL, "%s", "poa params out of range");
    DEV_GUARD(c);
    return poa_run(c, p, loci, refined, n, cap, bases, res);
}

// ---- include/svtrek_evidence.h
static svt_status evidence_launch(svt_ctx *c, const svt_locus *d_loci, const svt_result *d_refined, size_t n,
                                  svt_evidence *d_out, hipStream_t st) {
    if (n > 0x3fffffffull) return fail(c, SVT_EINVAL, "batch too large (%s)", "n > 2^30-1");
    const svt_status s = order_on(c, st);   // after every launch already issued (svt_reindex rebuilds the buckets)
    if (s) return s;
    const KArgs a = make_args(c, d_loci, nullptr, (uint32_t)n, false);
    hipLaunchKernelGGL(evidence_kernel, dim3((unsigned)((2 * n + WPB - 1) / WPB)), dim3(64 * WPB), 0, st, a, d_refined,
                       d_out);
    HIP_TRY(c, hipGetLastError());
    return SVT_OK;
}

svt_status svt_evidence_device(svt_ctx *c, const svt_locus *d_loci, const svt_result *d_refined, size_t n,
                               svt_evidence *d_out, void *stream) {
    if (!c) return SVT_EINVAL;
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    if (n == 0) return SVT_OK;
    if (!d_loci || !d_refined || !d_out) return fail(c, SVT_EINVAL, "%s", "null loci/refined/out");
    DEV_GUARD(c);
    return evidence_launch(c, d_loci, d_refined, n, d_out, (hipStream_t)stream);
}

static svt_status evidence_1(svt_ctx *c, const svt_locus *loci, const svt_result *refined, size_t n, svt_evidence *out) {
    if (n == 0) return SVT_OK;
    DEV_GUARD(c);
    svt_status s = ensure_batch(c, n);   // d_out holds the refined results here
    if (s) return s;
    HIP_TRY(c, c->d_evid.reserve(2 * n));
    HIP_TRY(c, hipMemcpy(c->d_loci, loci, n * sizeof(svt_locus), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_out, refined, n * sizeof(svt_result), hipMemcpyHostToDevice));
    if ((s = evidence_launch(c, c->d_loci, c->d_out, n, c->d_evid, nullptr))) return s;
    HIP_TRY(c, hipStreamSynchronize(nullptr));
    HIP_TRY(c, hipMemcpy(out, c->d_evid, 2 * n * sizeof(svt_evidence), hipMemcpyDeviceToHost));
    return SVT_OK;
}

svt_status svt_evidence_batch(svt_ctx *c, const svt_locus *loci, const svt_result *refined, size_t n, svt_evidence *out) {
    if (!c) return SVT_EINVAL;
    if (!c->loaded) return fail(c, SVT_ESTATE, "%s", "svt_load_pileup not called");
    if (n == 0) return SVT_OK;
    if (!loci || !refined || !out) return fail(c, SVT_EINVAL, "%s", "null loci/refined/out");
    return for_devices(c, n, [&](svt_ctx *x, size_t lo, size_t hi) {
        return evidence_1(x, loci + lo, refined + lo, hi - lo, out + 2 * lo);
    });
}

// ---- the pileup load and the index builds
#include "svt_load_host.inc"

// ---- include/svtrek_call.h
#include "svt_callindex_host.inc"
#include "svt_callmerge_host.inc"
#include "svt_call_host.inc"
#include "svt_junction_host.inc"
#include "svt_rearr_host.inc"
#include "svt_bnd_host.inc"

// ---- include/svtrek_genotype.h
#include "svt_genotype_host.inc"

// ---- include/svtrek_callseq.h
#include "svt_callseq_host.inc"

uint64_t svt_pileup_device_bytes(const svt_ctx *c) { return c ? c->dev_bytes : 0; }

uint64_t svt_poa_deferred(const svt_ctx *c) { return c ? c->poa_deferred : 0; }

svt_status svt_bgzf_inflate_device(svt_ctx *c, const uint8_t *d_comp, const svt_bgzf_block *d_blocks, size_t n,
                                   uint8_t *d_out, void *stream) {
    if (!c) return SVT_EINVAL;
    if (n == 0) return SVT_OK;
    if (!d_comp || !d_blocks || !d_out) return fail(c, SVT_EINVAL, "%s", "null buffer");
    if (n > 0xfffffffeull) return fail(c, SVT_EINVAL, "%s", "more than 2^32 - 2 blocks in one call");
    DEV_GUARD(c);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)std::min<size_t>(n, (size_t)INF_GRID);
    HIP_TRY(c, c->d_inferr.reserve(1));
    // the scratch slots and the error word are per context: calls on different streams run in
    // submission order (like every other launch of the context)
    if (svt_status s = order_on(c, st)) return s;
    HIP_TRY(c, hipMemsetAsync(c->d_inferr, 0xff, sizeof(uint32_t), st));
    hipLaunchKernelGGL(inflate_kernel, dim3(grid), dim3(WAVE), 0, st, d_comp, d_blocks, 0u, (uint32_t)n, d_out, c->d_inferr);
    HIP_TRY(c, hipGetLastError());
    return SVT_OK;
}

svt_status svt_bgzf_inflate_status(svt_ctx *c, void *stream, uint32_t *bad_block) {
    if (!c || !bad_block) return SVT_EINVAL;
    *bad_block = 0xffffffffu;
    if (!c->d_inferr) return SVT_OK;
    DEV_GUARD(c);
    // the error word belongs to the context's last inflate: order after it, whatever its stream
    const hipStream_t st = (hipStream_t)stream;
    if (svt_status s = order_on(c, st)) return s;
    HIP_TRY(c, hipMemcpyAsync(bad_block, c->d_inferr, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (*bad_block != 0xffffffffu) {
        char m[64];
        snprintf(m, sizeof m, "%u", *bad_block);
        return fail(c, SVT_EINVAL, "corrupt BGZF block %s (does not inflate to its ISIZE)", m);
    }
    return SVT_OK;
}

svt_status svt_bgzf_inflate(svt_ctx *c, const uint8_t *comp, size_t comp_bytes, const svt_bgzf_block *blocks, size_t n,
                            uint8_t *out, size_t out_bytes) {
    if (!c) return SVT_EINVAL;
    if (n == 0) return SVT_OK;
    if (!comp || !blocks || !out) return fail(c, SVT_EINVAL, "%s", "null buffer");
    for (size_t i = 0; i < n; i++) {   // every block inside its buffers (the kernel trusts the table)
        const svt_bgzf_block &k = blocks[i];
        if (k.clen > 65536u || k.ulen > 65536u || k.coff > comp_bytes || k.clen > comp_bytes - k.coff ||
            k.uoff > out_bytes || k.ulen > out_bytes - k.uoff)
            return fail(c, SVT_EINVAL, "%s", "BGZF block outside its buffers (or over 64 KiB)");
    }
    DEV_GUARD(c);
    svt_status s = order_on(c, nullptr);
    if (s) return s;
    HIP_TRY(c, c->d_infc.reserve(comp_bytes + 64));
    HIP_TRY(c, c->d_info.reserve(std::max<size_t>(out_bytes, 1)));
    HIP_TRY(c, c->d_infb.reserve(n));
    HIP_TRY(c, hipMemcpy(c->d_infc, comp, comp_bytes, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_infb, blocks, n * sizeof(svt_bgzf_block), hipMemcpyHostToDevice));
    DevEvent e0, e1;
    HIP_TRY(c, e0.create());
    HIP_TRY(c, e1.create());
    (void)hipEventRecord(e0, nullptr);
    s = svt_bgzf_inflate_device(c, c->d_infc, c->d_infb, n, c->d_info, nullptr);
    (void)hipEventRecord(e1, nullptr);
    uint32_t bad = 0;
    if (s == SVT_OK) s = svt_bgzf_inflate_status(c, nullptr, &bad);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) c->inf_ms = ms;
    if (s) return s;
    HIP_TRY(c, hipMemcpy(out, c->d_info, out_bytes, hipMemcpyDeviceToHost));
    return SVT_OK;
}

double svt_bgzf_last_inflate_ms(const svt_ctx *c) { return c ? c->inf_ms : 0.0; }

void *svt_host_alloc(svt_ctx *c, size_t bytes) {
    if (!c) return nullptr;
    DevGuard dg(c->device);
    void *p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

void svt_host_free(svt_ctx *c, void *p) {
    if (!c || !p) return;
    DevGuard dg(c->device);
    (void)hipHostFree(p);
}

#if SVT_PHASE_PROF
// diagnostic builds: refine_lane_kernel's phase times and counts since the last call (then cleared)
int svt_diag_phase(unsigned long long *out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ph_prof), sizeof ph_prof) != hipSuccess) return 1;
    const unsigned long long z[16] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(ph_prof), z, sizeof z) != hipSuccess;
}
#endif

void svt_close(svt_ctx *c) {
    if (!c) return;
    for (svt_ctx *d : c->subs) svt_close(d);
    c->subs.clear();
    DevGuard dg(c->device);
    delete c;   // its buffers and its event go with it, on its own device
}

}  // extern "C"

#include "svt_bam_host.inc"
