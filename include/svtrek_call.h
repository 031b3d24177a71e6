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
 * LIMITATION: items are clustered by their start alone.  Two deletions of different length at one
 * start become ONE call, whose len is their mean; len_lo / len_hi show it.  Splitting by length is
 * out of scope; svtrek_genotype.h genotypes the calls (or any site with a length range of its own).
 *
 * Status codes: svt_call_scan is SVT_ESTATE before svt_load_pileup and when the value buckets are
 * not built (SVTREK_INDEX=lists, or a pileup too large for them); SVT_EINVAL on NULL arguments,
 * link < 0, link > 2^20, min_support < 1, or no known type bit.  svt_call_fetch is SVT_EINVAL for a
 * range past the scanned count (n == 0 is SVT_OK).  svt_call_scan is ordered after every launch the
 * context has issued (svt_reindex included), selects / restores the device as the other entry
 * points do, acts on the first device of an svt_open_multi context, synchronises, and must not be
 * captured into a HIP graph.  Its scratch is allocated by the first scan: a context that never
 * scans pays nothing.
 */
#ifndef SVTREK_CALL_H
#define SVTREK_CALL_H

#include "svtrek_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svt_call {            /* 48 B */
    int32_t type, chrom;             /* SVT_DEL / SVT_INS; chrom = tid + 1 (svt_locus's) */
    uint32_t pos, end, support, depth, len, len_lo, len_hi, x_lo, x_hi, pad;
} svt_call;

typedef struct svt_call_params {
    int32_t link, min_support;
    uint32_t types, pad;             /* bit SVT_INS | bit SVT_DEL: (1u << SVT_INS) | (1u << SVT_DEL) */
} svt_call_params;

typedef struct svt_call_stats {
    uint64_t events;                 /* items of the scanned types (the skipped ones included) */
    uint64_t skipped;                /* items with x >= 2^30 */
    uint64_t clusters, calls;
    uint64_t big_buckets;            /* buckets too large for the tile sort (sorted in device memory) */
    double scan_ms;                  /* HIP-event time around the scan's device work */
} svt_call_stats;

/* link 10, min_support = the context's consensus_min_count (at least 1), both types */
void svt_call_default_params(const svt_ctx *ctx, svt_call_params *out);

/* Synchronous; the calls stay on the device. */
svt_status svt_call_scan(svt_ctx *ctx, const svt_call_params *params, uint64_t *n_calls);

/* Host copy of calls [first, first + n) of the last scan. */
svt_status svt_call_fetch(svt_ctx *ctx, uint64_t first, uint64_t n, svt_call *out);

/* The last scan's calls on the device: valid until the next scan / load / close. */
svt_status svt_call_device(svt_ctx *ctx, const svt_call **d_calls, uint64_t *n);

svt_status svt_call_stats_get(const svt_ctx *ctx, svt_call_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* SVTREK_CALL_H */
