/*
 * svtrek_evidence.h -- per-breakpoint evidence of refined calls (an extension of
 * include/svtrek_gpu.h; the reference prints the refined position only).
 *
 * For locus i and breakpoint k (k = 0: result.start, k = 1: result.end) let R be the refined
 * value, C the multiset of candidates the reference's walk pushes for that breakpoint's window
 * (what consensus_pos receives: the windows of audit.c:176-225, the region query and walk of
 * refinement.c:103-325) and ci = consensus_interval.  Candidates and R compare as the
 * reference's int values.  out[2*i + k] is
 *
 *   support  #{c in C : |c - R| <= ci}
 *   depth    reads of contig chrom-1 with pos <= R < endpos: what a one-base region query at R
 *            yields, no flag filter
 *   lo, hi   the smallest / largest supporting value (SVT_NA when support == 0)
 *
 * support is defined from R alone: it is not the count of the cluster that won the vote (the
 * winning cluster lies within ci of its rounded mean, so it is contained in the support).
 * depth is NOT guaranteed to be >= support: a read whose trailing soft clip ends exactly at R
 * votes for R but does not cover it (endpos == R), and candidates of one read may count twice.
 *
 *   R == SVT_NA (INV, unknown types, the second slot of an INS, contigs out of range, no
 *   consensus): {0, 0, SVT_NA, SVT_NA}.
 *   support == 0 with a refined R happens only for ci < 0; then lo = hi = SVT_NA.
 *   R != SVT_NA and ci >= 0: support >= consensus_min_count, lo <= R <= hi, hi - lo <= 2 * ci.
 *
 * `refined` is taken as given: a value the engine did not produce just gets counted (a locus
 * type without a window has an empty C).
 *
 * Status codes as in svtrek_gpu.h: SVT_ESTATE before svt_load_pileup, SVT_EINVAL on NULL
 * arguments (n == 0 is SVT_OK).  Both calls are ordered after every launch the context has
 * issued (svt_reindex included) and select / restore the device as the other entry points do.
 * They need not be captured into a HIP graph (svt_evidence_batch synchronises; neither call is
 * tested under stream capture).  On an svt_open_multi context svt_evidence_batch splits the
 * batch over the devices like svt_refine_batch; svt_evidence_device acts on the first device.
 */
#ifndef SVTREK_EVIDENCE_H
#define SVTREK_EVIDENCE_H

#include "svtrek_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svt_evidence {   /* 16 B, one per breakpoint: out[2*i + k] */
    uint32_t support;
    uint32_t depth;
    uint32_t lo, hi;
} svt_evidence;

/* n host-resident loci with their refined results into host-resident out[2n].  Synchronous. */
svt_status svt_evidence_batch(svt_ctx *ctx, const svt_locus *loci, const svt_result *refined, size_t n,
                              svt_evidence *out);

/* The same on DEVICE-resident arrays on `hip_stream` (a hipStream_t as void*, NULL = default
 * stream).  Asynchronous: errors of the launch itself are returned. */
svt_status svt_evidence_device(svt_ctx *ctx, const svt_locus *d_loci, const svt_result *d_refined, size_t n,
                               svt_evidence *d_out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SVTREK_EVIDENCE_H */
