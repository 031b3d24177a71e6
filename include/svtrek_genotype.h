/*
 * svtrek_genotype.h -- genotypes of DEL / INS sites from the loaded pileup alone (an extension of
 * include/svtrek_gpu.h, beside svtrek_call.h and svtrek_evidence.h).
 *
 * A SITE is a type, a contig, the interval [pos, end] a read has to span, and the ALT items: a
 * range of starts [x_lo, x_hi] and of lengths [len_lo, len_hi], both inclusive.  An svt_call is a
 * site through its fields of the same names (svt_genotype_calls reads the last scan's calls where
 * they lie).  For a site, every quantity in 64 bits:
 *   a = max(pos - flank, 0),  b = end + flank
 *   a read of contig chrom - 1 SPANS iff read.pos <= a and read.endpos > b -- the half-open
 *     convention of svtrek_evidence.h's depth: flank = 0, pos = end = R gives depth(R)
 *   span      the spanning reads
 *   ITEMS     svtrek_call.h's: every D op with len > 50 (DEL) / I op with len >= 50 (INS) as (x, len),
 *             x < 2^30.  Trailing-S markers and the items of the other type are not items.
 *   alt_all   the items of the site's type with x_lo <= x <= x_hi and len_lo <= len <= len_hi
 *   alt       those of them whose own read spans
 *   ref       span - alt, saturating at 0
 * A read with two matching items counts twice in alt (only possible for ranges wider than 50; ref
 * then saturates).  A spanning read that carries an op outside the site's length range counts as
 * ref: two alleles at one start are told apart by the site's length range.  The calls of a scan
 * with len_permille > 0 (svtrek_call.h, SPLITTING BY LENGTH) bring that range with them: a split
 * call's [x_lo, x_hi] x [len_lo, len_hi] holds exactly its own items, so alt_all == support for
 * every call, and the reads that carry a sibling allele span the site without a matching item and
 * count as ref (DR) -- a 300 / 500 heterozygote becomes two 0/1 records.  (A joint multi-allelic
 * genotype, 1/2, is not made.)  A call of a scan with len_permille = 0 covers every length at its
 * start, and its genotype counts either allele as alt.
 *
 * The genotype, in integers:
 *   L[g]   = ref * ref_cost[g] + alt * alt_cost[g]   (uint64; g = 0: 0/0, 1: 0/1, 2: 1/1)
 *   gt     = the g of the smallest L, ties to the lowest g
 *   pl[g]  = min((L[g] - min L + 500) / 1000, 65535)
 *   gq     = min(the smaller of the two other pl, 99)
 *   alt + ref == 0: gt = -1, gq = 0, pl = {0, 0, 0}
 * The costs are milli-phred per read, round(-10000 * log10 p); the defaults are those of a per-read
 * error of 0.05: ref_cost = {223, 3010, 13010}, alt_cost = {13010, 3010, 223}.
 *
 * An INVALID site gives an all-zero record with gt = -1: a type other than DEL / INS, chrom
 * outside 1..n_targets, x_lo > x_hi, len_lo > len_hi, or a contig without reads.  x_hi is then
 * clamped to 2^30 - 1 (a valid site whose x_lo lies past that has no items; its span is counted).
 *
 * Status codes: SVT_ESTATE before svt_load_pileup and when the value buckets are not built
 * (SVTREK_INDEX=lists, or a pileup too large for them); SVT_EINVAL on NULL arguments, flank < 0 or
 * flank > 2^20, n > 2^30 - 1.  svt_genotype_calls is SVT_ESTATE without a scan of the loaded pileup
 * and SVT_EINVAL when n_out is not the scanned count.  Every entry point is ordered after the
 * launches the context has issued (svt_reindex included), selects / restores the device as the
 * others do and acts on the first device of an svt_open_multi context.  Nothing is allocated
 * before the first svt_genotype_batch / svt_genotype_calls; svt_genotype_device allocates nothing.
 */
#ifndef SVTREK_GENOTYPE_H
#define SVTREK_GENOTYPE_H

#include "svtrek_call.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svt_gt_site {   /* 32 B */
    int32_t type, chrom;       /* SVT_DEL / SVT_INS; tid + 1 */
    uint32_t pos, end;         /* the interval reads must span */
    uint32_t x_lo, x_hi;       /* ALT items: start in [x_lo, x_hi] ...              */
    uint32_t len_lo, len_hi;   /* ... and length in [len_lo, len_hi] (inclusive)   */
} svt_gt_site;

typedef struct svt_gt_params {
    int32_t flank, pad;                      /* default 50 */
    uint32_t ref_cost[3], alt_cost[3];       /* milli-phred per read under 0/0, 0/1, 1/1 */
} svt_gt_params;

typedef struct svt_gt {        /* 32 B */
    uint32_t alt, ref, span, alt_all;
    int32_t gt;                /* -1 no call, 0 = 0/0, 1 = 0/1, 2 = 1/1 */
    uint32_t gq;
    uint16_t pl[3], pad;
} svt_gt;

/* flank 50, the costs of a per-read error of 0.05 */
void svt_genotype_default_params(const svt_ctx *ctx, svt_gt_params *out);

/* Host buffers, synchronous. */
svt_status svt_genotype_batch(svt_ctx *ctx, const svt_gt_params *params, const svt_gt_site *sites, size_t n, svt_gt *out);

/* Device buffers, one launch on `stream` (a hipStream_t; NULL: the default stream), asynchronous. */
svt_status svt_genotype_device(svt_ctx *ctx, const svt_gt_params *params, const svt_gt_site *d_sites, size_t n,
                               svt_gt *d_out, void *stream);

/* The last svt_call_scan's calls as sites, genotyped where they lie on the device; out[k] is call k's
 * record (svt_call_fetch's order).  n_out must equal the scanned count.  Synchronous. */
svt_status svt_genotype_calls(svt_ctx *ctx, const svt_gt_params *params, svt_gt *out, uint64_t n_out);

#ifdef __cplusplus
}
#endif
#endif /* SVTREK_GENOTYPE_H */
