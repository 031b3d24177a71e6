/*
 * svtrek_call.h -- discovery of DEL / INS calls from the loaded pileup alone (an extension of
 * include/svtrek_gpu.h; the reference's own `disc` mode needs GFA/GAF/FASTQ and prints nothing).
 *
 * For contig t and type T the ITEMS are
 *   DEL  every D op with len > 50 of every read of t,
 *   INS  every I op with len >= 50,
 * each as (x, len), x = the reference's walk position before the op (refinement.c:124, :299: H, P,
 * N and the op codes 9-15 advance x; x saturates at 2^30 as the index does).  These are exactly the
 * OP_DEL events of the value-bucket array S and the events of array I; the trailing-S markers of S
 * are not items.  No flag is filtered, as everywhere else.  Items with x >= 2^30 are dropped and
 * counted in stats.skipped.
 *
 * With the items of (t, T) sorted by x, a CLUSTER is a maximal run whose consecutive x differ by
 * <= link; clusters never span contigs or types.  A cluster of c items is a CALL iff
 * c >= min_support.  Its record:
 *   support        c
 *   pos            (sum x + c/2) / c      (integer c/2, 64-bit sum: consensus_pos's rounding)
 *   len            (sum len + c/2) / c
 *   x_lo, x_hi     the smallest / largest x;  len_lo, len_hi the smallest / largest len
 *   end            DEL: (sum (x + len + 1) + c/2) / c -- the value refine_end votes with, so an
 *                  audit of the call votes on the same numbers;  INS: pos + 1
 *   depth          reads of t with pos <= call.pos < endpos (svtrek_evidence.h's depth)
 *   chrom          t + 1 (svt_locus's);  type SVT_DEL / SVT_INS
 * Calls are ordered by (chrom, pos, type code).  Nothing depends on the order of the events inside
 * a bucket (it differs from rebuild to rebuild): a scan of the same pileup gives the same records.
 *
 * SPLITTING BY LENGTH (svt_call_params.len_permille = P).  With P = 0, the default, items are
 * clustered by their start alone: two deletions of different length at one start become ONE call,
 * whose len is their mean (len_lo / len_hi show it).  With P in 1 .. 1000 the start clusters are
 * formed exactly as above and each is then cut into ALLELE GROUPS: its items are sorted by len, and
 * between sorted neighbours lo <= hi there is a cut iff hi - lo > max(link, lo * P / 1000) (integer
 * division, 64-bit product).  A group is a maximal run without a cut -- single linkage: lengths
 * 300, 320, 340, 360 at P = 100 stay one group.  A group of c >= min_support items is a call, and
 * its record is the record above computed over the group's items only (support = c, the same
 * rounded means, the group's own x_lo / x_hi / len_lo / len_hi, depth at the group's pos).
 * min_support applies per group: a start cluster of 5 items cut 3 + 2 at min_support = 3 gives one
 * call, cut 2 + 2 + 1 none.  Calls are then ordered by (chrom, pos, type code, len): the groups of one
 * start cluster have disjoint len ranges more than link apart, so their rounded mean len differ and
 * still no two calls compare equal; they may come in any order of pos, equal pos included, while
 * groups of different start clusters keep the clusters' order.  stats.clusters still counts the start
 * clusters, stats.calls the calls.  svt_call_split_stats describes the split: a start cluster is a
 * CANDIDATE iff it has >= min_support items and len_hi - len_lo > max(link, len_lo * P / 1000) -- no
 * other cluster can contain a cut (the gap allowed does not decrease with lo) or give a call from a
 * part.  After a scan with P = 0 every field is zero, and such a scan launches, allocates and reads
 * back exactly what it did before the split existed, whatever was scanned before it.
 *
 * JOINING A READ'S FRAGMENTS (svt_call_params.merge_gap = G, merge_min = m).  An aligner often writes
 * one long deletion of a noisy read as 180D 5M 120D.  With G = 0, the default, the items are exactly
 * the ones above, merge_min is ignored, and a scan launches, allocates and reads back exactly what it
 * did before the merge existed, whatever was scanned before it.  With G in 1 .. 2^20 (and m in
 * 1 .. 50; 20 is the CLI's and Python's default) the items are MERGED ITEMS, defined per read of the
 * pileup (no flag filter, as everywhere):
 *   walk position  x is the item definition's -- the position before the op; H, P, N and the codes
 *                  9-15 advance it, I and S do not -- but kept in 64 bits here, unsaturated.
 *   FRAGMENT       of type DEL: a D op with len >= m; of type INS: an I op with len >= m.  Its TAIL is
 *                  x + len for DEL and x for INS.
 *   JOIN           take the fragments of one read and one type in CIGAR order: fragment j+1 joins
 *                  fragment j iff x[j+1] - tail[j] <= G.  The two types never interact: a 40I between
 *                  two D fragments moves nothing (an I does not advance x).  A 19D with m = 20 is no
 *                  fragment; it only adds 19 to the distance.
 *   RUN            a maximal chain of joined fragments (single linkage: three fragments each 40 apart
 *                  at G = 50 are one run).
 *   MERGED ITEM    a run of total L = sum len is an item iff L > 50 (DEL) / L >= 50 (INS).  The item is
 *                  (x, len) = (min(x of the first fragment, 2^30), min(L, 2^28 - 1)) and carries its
 *                  read's pos / endpos.
 * Because m <= 50, every item of an unmerged scan is a fragment and ends in exactly one run: the merged
 * items of a pileup in which no two fragments join and no lone fragment is shorter than the thresholds
 * are the unmerged items.  Everything downstream is unchanged and runs on the merged items: clusters,
 * min_support, the rounded means, ranges, depth and order; stats.events / skipped (now counts of merged
 * items); the split by length; svt_genotype_calls, which genotypes against the index the LAST scan
 * used, so that alt_all == support still holds for every call (svt_genotype_batch / _device keep
 * using the plain items).  A DEL call's end stays the mean of x + len + 1 with the SUMMED len: the
 * matched bases between the fragments are not counted, so end lies short of the last fragment's end by
 * them.  svt_call_merge_stats describes the merge; every field is zero after a scan with G = 0.
 * The merged items are a function of the pileup and (G, m) alone: they are built by the first scan that
 * asks for them (stats.scan_ms does not include the build, merge stats' build_ms is its device time),
 * kept until G or m change or the pileup is replaced or closed, and not touched by svt_reindex.  A
 * context that never merges allocates nothing for them.
 * Out of scope: inserted bases of merged calls (svt_call_consensus after a merged scan is
 * SVT_ESTATE), sites genotyped against the merged items, several devices (the scan acts on the first,
 * as before), and the CPU backend (no discovery there, as before).
 *
 * Status codes: svt_call_scan is SVT_ESTATE before svt_load_pileup and when the value buckets are
 * not built (SVTREK_INDEX=lists, or a pileup too large for them); SVT_EINVAL on NULL arguments,
 * link < 0, link > 2^20, min_support < 1, len_permille > 1000, merge_gap > 2^20, merge_gap > 0 with
 * merge_min outside 1 .. 50, or no known type bit (unless rearr != 0: svtrek_rearr.h, or bnd = 1: svtrek_bnd.h); SVT_ESTATE for more than 2^31 - 1 merged items.  svt_call_fetch is SVT_EINVAL for a
 * range past the scanned count (n == 0 is SVT_OK).  svt_call_scan is ordered after every launch the
 * context has issued (svt_reindex included), selects / restores the device as the other entry
 * points do, acts on the first device of an svt_open_multi context, synchronises, and must not be
 * captured into a HIP graph.  Its scratch is allocated by the first scan: a context that never
 * scans pays nothing.  The scratch of the split is allocated by the first scan with
 * len_permille > 0 and freed with the pileup, like the rest.
 */
#ifndef SVTREK_CALL_H
#define SVTREK_CALL_H

#include "svtrek_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svt_call {            /* 48 B */
    int32_t type, chrom;             /* SVT_DEL / SVT_INS (SVT_DUP / SVT_INV with rearr != 0: svtrek_rearr.h; SVT_BND with bnd = 1: svtrek_bnd.h); chrom = tid + 1 (svt_locus's) */
    uint32_t pos, end, support, depth, len, len_lo, len_hi, x_lo, x_hi, pad;
} svt_call;

typedef struct svt_call_params {
    int32_t link, min_support;
    uint32_t types;                  /* bit SVT_INS | bit SVT_DEL: (1u << SVT_INS) | (1u << SVT_DEL) */
    uint32_t len_permille;           /* 0: clusters by start alone; 1 .. 1000: split by length (above) */
    uint32_t merge_gap, merge_min;   /* 0: single ops as items; 1 .. 2^20: join a read's fragments of len >= merge_min (above) */
    uint32_t junctions;              /* 0: CIGAR items alone; 1: plus the items of split alignments (svtrek_junction.h) */
    uint32_t rearr;                  /* 0, or bits (1u << SVT_DUP) | (1u << SVT_INV): DUP / INV calls from split alignments (svtrek_rearr.h) */
    uint32_t bnd;                    /* 0, or 1: translocation breakends from split alignments, SVT_BND calls (svtrek_bnd.h) */
} svt_call_params;

typedef struct svt_call_stats {
    uint64_t events;                 /* items of the scanned types (the skipped ones included) */
    uint64_t skipped;                /* items with x >= 2^30 */
    uint64_t clusters, calls;
    uint64_t big_buckets;            /* buckets too large for the tile sort (sorted in device memory) */
    double scan_ms;                  /* HIP-event time around the scan's device work */
} svt_call_stats;

typedef struct svt_call_split_stats {   /* all zero after a scan with len_permille = 0 */
    uint64_t candidates;             /* start clusters that could hold a cut (above) */
    uint64_t split;                  /* candidates cut into more than one group */
    uint64_t groups;                 /* groups of all candidates, at any support */
    uint64_t big;                    /* candidates of more items than the tile sort holds (sorted in device memory) */
} svt_call_split_stats;

typedef struct svt_call_merge_stats {   /* all zero after a scan with merge_gap = 0 */
    uint64_t fragments;              /* D / I ops of len >= merge_min, of both types whatever the scan's type bits */
    uint64_t runs;                   /* maximal chains of joined fragments */
    uint64_t joined_items;           /* merged items of >= 2 fragments */
    uint64_t items;                  /* merged items (those with x >= 2^30 included) */
    double build_ms;                 /* HIP-event time of the build of the merged items this scan ran on */
} svt_call_merge_stats;

/* link 10, min_support = the context's consensus_min_count (at least 1), both types, len_permille 0,
 * merge_gap 0, merge_min 20, junctions 0, rearr 0, bnd 0 */
void svt_call_default_params(const svt_ctx *ctx, svt_call_params *out);

/* Synchronous; the calls stay on the device. */
svt_status svt_call_scan(svt_ctx *ctx, const svt_call_params *params, uint64_t *n_calls);

/* Host copy of calls [first, first + n) of the last scan. */
svt_status svt_call_fetch(svt_ctx *ctx, uint64_t first, uint64_t n, svt_call *out);

/* The last scan's calls on the device: valid until the next scan / load / close. */
svt_status svt_call_device(svt_ctx *ctx, const svt_call **d_calls, uint64_t *n);

svt_status svt_call_stats_get(const svt_ctx *ctx, svt_call_stats *out);

/* The last scan's split by length. */
svt_status svt_call_split_stats_get(const svt_ctx *ctx, svt_call_split_stats *out);

/* The last scan's joining of fragments. */
svt_status svt_call_merge_stats_get(const svt_ctx *ctx, svt_call_merge_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* SVTREK_CALL_H */
