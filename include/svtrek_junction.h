/*
 * svtrek_junction.h -- DEL / INS items from split alignments (an extension of include/svtrek_call.h:
 * svt_call_params.junctions = 1; the CLI's `svtrek call --split-reads`).
 *
 * A long-read aligner writes a deletion of a few kb and up, or an insertion too long to keep inside one
 * alignment, as TWO alignments of one read linked by their SA:Z tags, not as one CIGAR with a long D or
 * I.  svtrek_call.h's items are single CIGAR ops (or a read's joined ops); this header adds the items
 * such a pair of alignments stands for.  "Split" already means the split by length in svtrek_call.h, so
 * the feature is called JUNCTION everywhere in code and statistics.
 *
 * SEGMENT.  One alignment of a read, {tid, strand, r_beg, r_end, q_beg, q_end}:
 *   cl / ct      the summed length of the leading / trailing run of S and H ops of its CIGAR
 *   qlen, rlen   the sum of the M I = X ops / of the M D N = X ops
 *   r_beg        the 0-based position (SA gives it 1-based);  r_end = r_beg + rlen
 *   q_beg, q_end query coordinates in the read's ORIGINAL orientation:
 *                strand + (0): q_beg = cl, q_end = cl + qlen;  strand - (1): q_beg = ct, q_end = ct + qlen
 *
 * SEGMENT TABLE (svt_junction_view).  One record for every pileup record that carries an SA:Z tag, in
 * ascending pileup read index: read[k] is the record's index in the loaded pileup, its rows are
 * seg[off[k] .. off[k + 1]).  seg[off[k]] is the record's OWN segment, computed from the CIGAR the pileup
 * holds (the CG-restored one) and flag 0x10; the following rows are its SA entries in tag order.  No
 * flag is filtered, as everywhere.
 *
 * JUNCTION of a record.  A is its own segment, T all its segments.  Segments are ordered by the tuple
 * (q_beg, q_end, tid, r_beg, strand).  B is the segment of T with the smallest tuple strictly greater
 * than A's; a record without one has no junction.  Segments with equal tuples therefore never pair, and
 * the order of the SA entries does not matter.  Each junction of a read is emitted exactly once: by the
 * record that is its query-first segment; no flag is consulted for this.
 *   The junction QUALIFIES iff B.tid == A.tid and B.strand == A.strand; otherwise it counts in
 *   stats.other (inversions, duplications and translocations are out of scope).
 *   (Lf, Rt) = (A, B) on strand +, (B, A) on strand -.
 *   In signed 64 bits:  dr = Rt.r_beg - Lf.r_end,  dq = B.q_beg - A.q_end,  d = dr - dq.
 *
 * JUNCTION ITEM of a qualifying junction.
 *   DEL iff d > 50 and dr > 0:                       (x, len) = (Lf.r_end, d)
 *   INS iff -d >= 50 and dq > 0 and dr >= -50:       (x, len) = (Lf.r_end, -d)
 *   -d >= 50 and dq > 0 and dr < -50 is a larger reference overlap -- a duplication -- and counts in
 *   stats.other.  Every other qualifying junction gives no item and counts nowhere but in
 *   stats.junctions.
 *   len is clamped to 2^28 - 1.  An item with x >= 2^30 is dropped and counted in skipped, as the plain
 *   items are (both svt_call_stats.skipped and svt_call_junction_stats.skipped count it).
 *   The item carries the EXTENT (min(Lf.r_beg, Rt.r_beg), max(Lf.r_end, Rt.r_end)) where a CIGAR item
 *   carries its read's pos / endpos (both clamped to 2^31 - 1, past every site's a and b).
 *
 * ITEMS of a scan with junctions = 1: the base items -- the plain ones, or the merged ones when
 * merge_gap > 0 -- plus the junction items of the types asked for.  Clusters, min_support, the rounded
 * means, ranges, end, depth, order, len_permille and stats.events / skipped / clusters / calls are
 * defined on that union exactly as svtrek_call.h defines them on the base items.  With junctions = 0,
 * the default, a scan launches, allocates and reads back exactly what it did before junctions existed,
 * whatever was scanned before it, and a context that never asks for junctions allocates nothing for
 * them.  A table of n == 0 records is valid: the scan then equals the base scan record for record.
 *
 * GENOTYPE of such calls (svt_genotype_calls after a scan with junctions = 1; svtrek_genotype.h).
 * alt_all and alt count junction items too; a junction item "spans" by its carried extent.  span is
 * unchanged: the pileup records that span.  The two halves of a split read do not span, so
 *   ref = span - (alt - alt_j), saturating at 0,
 * where alt_j is the number of junction items among alt.  alt_all == support holds for every call.
 * svt_genotype_batch / _device keep the plain index, as after a merged scan.
 *
 * THE INDEX.  The union of the base view's events and the junction events is a third index in the value
 * buckets' shape, a function of (pileup, table, merge_gap, merge_min).  It is built by the first scan
 * that asks for it (stats.scan_ms excludes the build; svt_call_junction_stats.build_ms is its HIP-event
 * time), kept until one of its four inputs changes, freed with the pileup and untouched by svt_reindex.
 * svt_call_junction_stats describes the TABLE's junctions of both types, whatever the scan's type bits.
 *
 * Status codes.  svt_load_junctions: SVT_ESTATE before svt_load_pileup; SVT_EINVAL for NULL arguments
 * (NULL arrays with n == 0 are fine), read not strictly ascending or past the pileup, off not monotone
 * (off[0] must be 0), a record with no row, strand > 1, r_end < r_beg, q_end < q_beg, tid outside the
 * targets, or an own segment whose tid / r_beg / r_end are not the pileup record's contig / pos /
 * endpos (r_end == pos goes with an endpos of pos + 1, htslib's for an unmapped record or a CIGAR without a
 * reference base: such a record's own segment has rlen 0).  This check bounds a junction's x: it is a segment's
 * end at or before a pileup record's start + 50, so it never reaches a contig's last bucket.  A table that fails leaves the previous one in place.  svt_call_scan: SVT_EINVAL for
 * junctions > 1; SVT_ESTATE for junctions = 1 without a table for the loaded pileup (a new
 * svt_load_pileup drops it) and for more than 2^31 - 1 union items.  svt_call_consensus after a scan
 * with junctions = 1 is SVT_ESTATE.
 * Out of scope: inversions and duplications (counted in other here; include/svtrek_rearr.h calls them
 * from the same table), translocations and BND records (counted in other here; include/svtrek_bnd.h
 * calls them from the same table), MAPQ or
 * flag filters, a per-call count of junction support, inserted bases of junction calls, SA in the device
 * BAM decoder, several devices and the CPU backend.
 */
#ifndef SVTREK_JUNCTION_H
#define SVTREK_JUNCTION_H

#include "svtrek_call.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svt_junction_seg {    /* 24 B */
    int32_t tid;
    uint32_t strand;                 /* 0: +, 1: - */
    uint32_t r_beg, r_end, q_beg, q_end;
} svt_junction_seg;

typedef struct svt_junction_view {
    uint64_t n;                      /* records */
    const uint64_t *read;            /* [n] pileup read index, strictly ascending */
    const uint64_t *off;             /* [n + 1] rows of record k: seg[off[k] .. off[k + 1]) */
    const svt_junction_seg *seg;     /* [off[n]] */
} svt_junction_view;

typedef struct svt_call_junction_stats {   /* all zero after a scan with junctions = 0 */
    uint64_t records, segments;      /* the table's records and rows */
    uint64_t junctions;              /* records with a B */
    uint64_t del_items, ins_items;   /* junction items (those with x >= 2^30 included) */
    uint64_t other;                  /* junctions to another contig or strand, and reference overlaps past 50 */
    uint64_t skipped;                /* junction items with x >= 2^30 */
    double build_ms;                 /* HIP-event time of the build of the index this scan ran on */
} svt_call_junction_stats;

/* After svt_load_pileup; synchronous; the arrays are copied; replaces a previous table. */
svt_status svt_load_junctions(svt_ctx *ctx, const svt_junction_view *view);

/* The last scan's junctions. */
svt_status svt_call_junction_stats_get(const svt_ctx *ctx, svt_call_junction_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* SVTREK_JUNCTION_H */
