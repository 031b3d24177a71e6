/*
 * svtrek_rearr.h -- DUP / INV calls from split alignments (an extension of include/svtrek_junction.h:
 * svt_call_params.rearr; the CLI's `svtrek call --rearrangements`).
 *
 * A tandem duplication and an inversion leave no CIGAR op behind: an aligner writes a read that crosses
 * one of their breakpoints as two alignments linked by SA:Z tags, the second one UPSTREAM of the first
 * (duplication) or on the OTHER STRAND (inversion).  svtrek_junction.h counts both in stats.other and
 * drops them; this header gives them items, clusters and calls.  The feature is called REARRANGEMENT
 * (rearr) everywhere in code and statistics.
 *
 * Segments, the segment table, A, B, the tuple order, Lf, Rt, dr, dq and d are svtrek_junction.h's,
 * unchanged; the table is the one svt_load_junctions took.  A record's junction yields a rearrangement
 * item only when B.tid == A.tid.
 *
 * INV ITEM, iff B.strand != A.strand.  Let p be the reference coordinate joined at A's query-last base
 * -- A.r_end on strand +, A.r_beg on strand - -- and q the one at B's query-first base -- B.r_beg on
 * strand +, B.r_end on strand -.  In signed 64 bits it is an item iff |p - q| > 50:
 *   (x, len) = (min(p, q), |p - q|).
 * A fold-back (p ~ q) gives none.  A read of either strand that crosses either breakpoint of an
 * inversion [s, e) gives (s, e - s): the items of one inversion cluster.
 *
 * DUP ITEM, iff B.strand == A.strand, dr < -50 and -d >= 50:
 *   (x, len) = (Rt.r_beg, -dr),   the reference interval [Rt.r_beg, Lf.r_end).
 * There is no condition on dq: this is a superset of the same-strand overlaps svt_call_junction_stats.other
 * counts, and other goes on counting them.
 *
 * len is clamped to 2^28 - 1.  An item with x >= 2^30 is dropped and counted in skipped (both
 * svt_call_stats.skipped and svt_call_rearr_stats.skipped count it).
 * x is never past the own segment's end: for DUP x = B.r_beg < A.r_end - 50 on strand + and x == A.r_beg
 * on strand -; for INV x = min(p, q) <= p <= A.r_end.  svt_load_junctions checks every own segment against
 * its pileup record (r_end is the record's endpos, or its pos), and a contig's buckets reach 64 kb past
 * its largest endpos before the last one begins: so no rearrangement item reaches a contig's last
 * bucket, every item lies in its bucket's own 1 kb, and the counting sort of a big bucket
 * (svt_call.inc) holds for this index as it does for the union index.
 *
 * CLUSTERS AND CALLS.  Clusters, min_support, the rounded means, ranges, depth and the split by
 * len_permille are svtrek_call.h's, per (contig, type), on the rearrangement items alone: they are never
 * combined with CIGAR or junction items.  A call's record has type SVT_DUP / SVT_INV and
 *   end = (sum (x + len) + c/2) / c        (no + 1: DEL's exists only for refine_end).
 * The calls of all the types a scan asked for come out in ONE list in (chrom, pos, type code[, len])
 * order; the type codes are INS 1, DEL 2, INV 3, DUP 4.
 *
 * svt_call_params.rearr is a bit mask of (1u << SVT_DUP) | (1u << SVT_INV), 0 by default.  With 0 a scan
 * launches, allocates and reads back exactly what it did before rearrangements existed, whatever was
 * scanned before it, and a context that never asks allocates nothing for them.  It is independent of
 * junctions (it only needs the table) and of merge_gap; types keeps meaning DEL / INS only, and types
 * without a DEL / INS bit is accepted when rearr != 0: a rearrangement-only scan.
 * svt_call_stats.events / skipped / clusters / calls / big_buckets and svt_call_split_stats are sums over
 * everything the scan looked at; svt_call_junction_stats keeps its meaning, other included.
 *
 * THE INDEX.  The items go into their own index of the value buckets' shape: row S holds the DUP events,
 * row I the INV events, an event is {x, len << 4 | OP_DEL (DUP) / OP_INS (INV), extent end, extent begin |
 * mark} as a junction event is.  It is a function of (pileup, table) alone, built by the first scan that
 * asks (outside stats.scan_ms; svt_call_rearr_stats.build_ms is its HIP-event time), kept until either
 * changes, freed with the pileup and untouched by svt_reindex.
 *
 * GENOTYPES AND CONSENSUS.  svt_genotype_calls after such a scan gives the DEL / INS calls the record it
 * gives them today and the DUP / INV calls the invalid-site record (gt = -1, all zero; svtrek_genotype.h).
 * svt_call_consensus after a scan with rearr != 0 is SVT_ESTATE.
 *
 * Status codes.  svt_call_scan: SVT_EINVAL for any other bit in rearr; SVT_ESTATE for rearr != 0 without
 * a table for the loaded pileup; types without a DEL / INS bit stays SVT_EINVAL when rearr == 0.
 * Out of scope: translocations and BND records (include/svtrek_bnd.h calls them from the same table), genotypes of DUP / INV, rearrangement items combined
 * with CIGAR items, several devices, the CPU backend, SA in the device BAM decoder.
 */
#ifndef SVTREK_REARR_H
#define SVTREK_REARR_H

#include "svtrek_junction.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svt_call_rearr_stats {   /* all zero after a scan with rearr = 0 */
    uint64_t dup_items, inv_items;   /* the table's items of both types, whatever the mask (those with x >= 2^30 included) */
    uint64_t skipped;                /* items of the scanned types with x >= 2^30 */
    uint64_t clusters, calls;        /* of the scanned types */
    double build_ms;                 /* HIP-event time of the build of the index this scan ran on */
} svt_call_rearr_stats;

/* The last scan's rearrangements. */
svt_status svt_call_rearr_stats_get(const svt_ctx *ctx, svt_call_rearr_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* SVTREK_REARR_H */
