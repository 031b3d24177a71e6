/*
 * svtrek_bnd.h -- translocation breakends from split alignments (an extension of include/svtrek_rearr.h:
 * svt_call_params.bnd; the CLI's `svtrek call --breakends`).
 *
 * A read that crosses a translocation breakpoint is written as two alignments linked by SA:Z tags, the
 * second one on ANOTHER CONTIG.  svtrek_junction.h and svtrek_rearr.h count such a junction in
 * svt_call_junction_stats.other and drop it; this header gives it an item, clusters and calls.  The
 * feature is called BND (bnd) everywhere in code and statistics.
 *
 * Segments, the segment table, A, B and the tuple order are svtrek_junction.h's, unchanged; the table is
 * the one svt_load_junctions took.
 *
 * BND ITEM of a record, iff it has a B and B.tid != A.tid.  There is no length threshold.
 *   breakend a = (A.tid, p, sa):  p is the reference coordinate joined at A's query-last base -- A.r_end
 *                on strand +, A.r_beg on strand - --, sa = A.strand: 0 means the reference to the LEFT of
 *                p is in the read, 1 the reference to the right of it.
 *   breakend b = (B.tid, q, sb):  q is the coordinate at B's query-first base -- B.r_beg on strand +,
 *                B.r_end on strand - --, sb = 1 - B.strand.
 *   canonical form: lo is the breakend with the smaller tid, hi the other.  The item is
 *                (tid_lo, x = pos_lo, tid_hi, y = pos_hi, o = 2 * s_lo + s_hi).
 * A read of the other strand across the same junction gives the same item: its A is this read's B
 * mirrored (B's query-first base becomes A's query-last one and the strand flips, so (q, sb) is that
 * read's (p, sa) and the other way round).  An item with x >= 2^30 or y >= 2^30 is dropped and counted
 * in skipped (both svt_call_stats.skipped and svt_call_bnd_stats.skipped count it).
 *
 * CLASS: (tid_lo, tid_hi, o).  Items of different classes are never combined, and BND items are never
 * combined with CIGAR, junction or rearrangement items.
 *
 * CLUSTERS AND CALLS, per class.  With the class's items sorted by x, a START CLUSTER is a maximal run
 * whose neighbours differ by <= link.  Each start cluster's items are then sorted by y and cut where
 * neighbours differ by > link; a GROUP is a maximal run without a cut -- single linkage in both
 * coordinates.  A group of c >= min_support items is a call.  len_permille, merge_gap and junctions have
 * no effect on BND calls.
 *
 * RECORD: an svt_call (svtrek_call.h; the field name pad stays) with
 *   type           SVT_BND (6)
 *   chrom          tid_lo + 1
 *   pos            (sum x + c/2) / c
 *   end            (sum y + c/2) / c -- the PARTNER's position, on the partner's contig
 *   support        c
 *   depth          reads of tid_lo with pos <= call.pos < endpos; 0 on a contig without reads
 *   len            0
 *   x_lo, x_hi     the group's smallest / largest x
 *   len_lo, len_hi the group's smallest / largest y
 *   pad            (tid_hi + 1) << 2 | o;  SVT_CALL_MATE_CHROM / SVT_CALL_MATE_ORIENT below read it
 *
 * ORDER.  All the calls of a scan come out in one list in (chrom, pos, type code[, len]) order as before,
 * type code 6 last; BND calls that tie on (chrom, pos) are ordered by (mate chrom, o, end).  The order is
 * total: the groups of one class in one start cluster have disjoint y ranges more than link apart, so
 * their rounded means differ, and the start clusters of one class have disjoint x ranges.
 *
 * svt_call_params.bnd (0 or 1, 0 by default).  With 0 a scan launches, allocates and reads back exactly
 * what it did before breakends existed, whatever was scanned before it, and a context that never asks
 * allocates nothing for them.  It is independent of junctions, rearr and merge_gap (it only needs the
 * table); types without a DEL / INS bit is accepted when bnd == 1, as it is when rearr != 0.
 * svt_call_stats.events / skipped / clusters / calls are sums over everything the scan looked at
 * (clusters counts start clusters); svt_call_junction_stats keeps its meaning, other included.
 *
 * THE ITEM LIST.  No buckets: an item's x may be an SA row's coordinate on a contig that has no read at
 * all.  The items are one list in (class, x) order, a function of (pileup, table) alone, built by the
 * first scan that asks (outside stats.scan_ms; svt_call_bnd_stats.build_ms is its HIP-event time), kept
 * until either changes (svt_load_junctions drops it), freed with the pileup and untouched by
 * svt_reindex.  The order of items with equal keys is arbitrary and nothing reads it: the records are
 * sums, minima and maxima.
 *
 * GENOTYPES AND CONSENSUS.  svt_genotype_calls gives BND calls the invalid-site record (gt = -1, all
 * zero; svtrek_genotype.h), as it does DUP and INV, and the other calls the record they get from the same
 * scan without bnd.  svt_call_consensus after a scan with bnd = 1 is SVT_ESTATE.
 *
 * Status codes.  svt_call_scan: SVT_EINVAL for bnd > 1; SVT_ESTATE for bnd = 1 without a table for the
 * loaded pileup, and for bnd = 1 with 2^30 - 1 targets or more.
 * Out of scope: mate records and MATEID, breakends within one contig, genotypes of BND calls, MAPQ and
 * flag filters, depth at the partner, several devices, the CPU backend, SA in the device BAM decoder.
 */
#ifndef SVTREK_BND_H
#define SVTREK_BND_H

#include "svtrek_rearr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Of a call of type SVT_BND: the partner's chrom (tid_hi + 1) and the orientation o = 2 * s_lo + s_hi. */
#define SVT_CALL_MATE_CHROM(c)  ((int32_t)((c).pad >> 2))
#define SVT_CALL_MATE_ORIENT(c) ((uint32_t)((c).pad & 3u))

typedef struct svt_call_bnd_stats {     /* all zero after a scan with bnd = 0 */
    uint64_t items;                  /* the table's BND items, skipped ones included */
    uint64_t skipped;                /* items dropped for x or y >= 2^30 */
    uint64_t classes;                /* distinct classes among the kept items */
    uint64_t clusters;               /* start clusters */
    uint64_t groups;                 /* groups, at any support */
    uint64_t calls;
    double build_ms;                 /* HIP-event time of the build of the item list this scan ran on */
} svt_call_bnd_stats;

/* The last scan's breakends. */
svt_status svt_call_bnd_stats_get(const svt_ctx *ctx, svt_call_bnd_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* SVTREK_BND_H */
