/*
 * svtrek_callseq.h -- the consensus inserted sequence of discovered INS calls (an extension of
 * include/svtrek_call.h: svt_call_scan finds the calls, svt_load_insseq brings the inserted bases,
 * and the allele-consensus mode's poa_kernel, unchanged, fuses them).
 *
 * Sequence index k is svt_load_insseq's: the I >= 50 ops of the loaded pileup in (read, op) order.
 * For call j of the last svt_call_scan:
 *
 *   DEL call   res = {-1, 0, 0, 0}: no consensus.
 *   INS call   the ITEMS OF THE CALL are the I >= 50 ops of contig chrom - 1 with
 *                x_lo <= x <= x_hi      x the walk position of svtrek_call.h: the read's pos plus the
 *                                       lengths of every earlier op but I and S (H, P, N and the codes
 *                                       9-15 advance it), saturated at 2^30 -- an op at x >= 2^30
 *                                       belongs to no call (every call has x_hi < 2^30)
 *                len_lo <= len <= len_hi.
 *
 * These are exactly the ops the scan counted into the call, for any len_permille:
 *   - the start clusters of one (contig, type) have x ranges more than `link` apart (a cluster is a
 *     maximal run of sorted x whose neighbours differ by <= link), so an op of another start cluster
 *     lies outside [x_lo, x_hi] -- the call's x range is inside its cluster's;
 *   - the allele groups of one start cluster have disjoint len ranges (they are cut from the cluster's
 *     items sorted by len), so an op of a sibling group, or one that fell below min_support, lies
 *     outside [len_lo, len_hi]; with len_permille = 0 the call is the whole cluster and [len_lo,
 *     len_hi] holds every length in it;
 *   - an op of the call's own cluster and group lies inside both ranges by their definition.
 * Hence the number of items equals call.support (svtrek_genotype.h's alt_all == support is the same
 * statement).
 *
 *   SUPPORTING SEQUENCES   the call's items with len <= max_len in ascending k -- (read, op) order: it
 *                does not depend on the order of the events inside a bucket, which differs from rebuild
 *                to rebuild.  n_support is their count; the first max_support are kept.
 *   CONSENSUS    from there on svt_poa_consensus's rule, unchanged (oracle/poa_oracle.c): of the kept
 *                sequences, in order, the first max_seqs that fit (1 <= bases, the graph within
 *                max_nodes) are fused, the heaviest bundle is the consensus, and
 *                res = {len, n_support, n_used, 0}; bases[j * cap .. + min(len, cap)) holds nt4 codes.
 *                support_radius is not used.
 *
 * The mechanism (svt_callseq.inc): an ITEM TABLE {x, len} per sequence index, built once per loaded
 * pileup by the first svt_call_consensus -- one lane per read that owns an I >= 50 op walks its CIGAR --
 * together with the pileup's REACH, the largest x - read pos over the items with x < 2^30.  An item
 * of a call then belongs to a read with pos in [x_lo - reach, x_hi]: two binary searches in the contig's
 * sorted pos give a contiguous range of the table, which one wave per call filters in k order.
 *
 * Status codes: SVT_EINVAL on a NULL context or params; SVT_ESTATE before svt_load_pileup, without an
 * svt_call_scan of the loaded pileup, and before svt_load_insseq; SVT_EINVAL for a range past the
 * scanned count; SVT_OK for n == 0; then SVT_EINVAL for NULL res, cap < 0, NULL bases with cap > 0,
 * n > 2^30 - 1, and parameters outside the limits svt_poa_consensus checks (the same test).
 * svt_call_consensus is synchronous, ordered after every launch the context has issued (svt_reindex
 * included: the table does not depend on the buckets), selects / restores the device as the other
 * entry points do, acts on the first device of an svt_open_multi context and must not be captured
 * into a HIP graph.  The table is allocated by the first call and freed with the pileup; the last
 * scan's calls are read where they lie and stay as they are.
 */
#ifndef SVTREK_CALLSEQ_H
#define SVTREK_CALLSEQ_H

#include "svtrek_call.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svt_call_consensus_stats {   /* of the last svt_call_consensus */
    uint64_t items;          /* entries of the item table: the pileup's I >= 50 ops */
    uint64_t reach;          /* largest x - read pos over the items with x < 2^30 (0: none) */
    uint64_t ins_calls;      /* INS calls in the window */
    uint64_t window_items;   /* table entries the gather streamed: the candidate ranges of those calls, summed */
    uint64_t window_max;     /* the largest candidate range */
    uint64_t deferred;       /* calls rerun on the full-size POA slots */
    double table_ms;         /* HIP-event time of the table build (kept from the call that built it) */
    double gather_ms;        /* ... of the support gather */
    double poa_ms;           /* ... of the consensus launches and their copies */
} svt_call_consensus_stats;

/* Consensus of calls [first, first + n) of the last scan: res[j], bases[j * cap ..] for call first + j. */
svt_status svt_call_consensus(svt_ctx *ctx, const svt_poa_params *p, uint64_t first, uint64_t n, int32_t cap,
                              uint8_t *bases, svt_poa_result *res);

svt_status svt_call_consensus_stats_get(const svt_ctx *ctx, svt_call_consensus_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* SVTREK_CALLSEQ_H */
