/*
 * svtrek_host.h -- host side of the `svtrek audt` drop-in (C ABI, plain types).
 *
 *  - BAM/BGZF ingest -> columnar pileup (replaces, for this path, htslib's
 *    hts_open/sam_hdr_read/sam_index_load + the per-window sam_itr_queryi/sam_itr_next
 *    decode of reference refinement.c:114-117; the whole file is read once, multi-
 *    threaded inflate, SEQ/QUAL/aux dropped except the CG tag).
 *  - VCF record parsing (A1, reference audit.c:62-173) and result printing (A11,
 *    audit.c:176-232), byte-identical to the reference's stdout.
 */
#ifndef SVTREK_HOST_H
#define SVTREK_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "svtrek_gpu.h"
#include "svtrek_evidence.h"
#include "svtrek_call.h"
#include "svtrek_genotype.h"
#include "svtrek_callseq.h"
#include "svtrek_junction.h"
#include "svtrek_rearr.h"
#include "svtrek_bnd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svth_bam svth_bam;

/* Read a BAM (BGZF) completely into a columnar pileup.  threads >= 1 inflate workers.
 * Returns NULL on error (message in err). */
svth_bam *svth_bam_read(const char *path, int threads, char *err, size_t errcap);
/* The records of a coordinate-sorted BAM from (tid0, beg0) up to, excluding, the first
 * record at or past (tid1, end1), read from the BAI's linear-index offset of (tid0, beg0)
 * (`path`.bai, required; the file's header is read from its start).  Every region query
 * (tid, [beg, end)) with (tid0, beg0) <= (tid, beg) and (tid, end) <= (tid1, end1) yields the
 * same reads from this pileup as from the whole file; a few records before beg0 may be
 * included.  tid0 < 0: the whole file (svth_bam_read). */
svth_bam *svth_bam_read_region(const char *path, int threads, int32_t tid0, int64_t beg0, int32_t tid1, int64_t end1,
                               char *err, size_t errcap);
/* A BGZF inflater for the ingest (svth_bam_read_ex): inflate(n blocks of comp -> out, the
 * layout of svt_bgzf_inflate, include/svtrek_gpu.h; 0 = done, else a message in err); alloc /
 * release (optional): the buffers inflate reads and writes fastest (pinned host memory);
 * batch_bytes: compressed bytes per inflate call (0: 1 GiB). */
typedef struct svth_inflater {
    int (*inflate)(void *user, const uint8_t *comp, size_t comp_bytes, const svt_bgzf_block *blocks, size_t n,
                   uint8_t *out, size_t out_bytes, char *err, size_t errcap);
    void *(*alloc)(void *user, size_t bytes);
    void (*release)(void *user, void *p);
    void *user;
    size_t batch_bytes;
} svth_inflater;
/* svth_bam_read_region with the BGZF blocks inflated by `inf` (the CLI passes the device's
 * svt_bgzf_inflate and pinned buffers): batches read by `threads` parallel preads, the next
 * batch read and inflated by a helper thread while the records of the current one are parsed;
 * inf == NULL: host threads inflate. */
svth_bam *svth_bam_read_ex(const char *path, int threads, int32_t tid0, int64_t beg0, int32_t tid1, int64_t end1,
                           const svth_inflater *inf, char *err, size_t errcap);
/* svth_bam_read_ex that also keeps the inserted bases of the kept reads' I >= 50 ops -- what
 * svt_load_insseq takes -- in the final pileup's (read, op) order (after the stable (tid, pos) sort
 * when the file needed one), so that n_ins == svt_pileup_ins_count() once the pileup is loaded.
 * The query offset of an op is the summed length of the M, I, S, = and X ops before it (H, P, N and D
 * consume no SEQ) in the CIGAR the pileup keeps, the one restored from CG:B,I included.  Bases are
 * unpacked from the 4-bit SEQ, high nibble first: codes 1, 2, 4, 8 become 0, 1, 2, 3, every other code
 * 4.  With l_seq == 0, or where an op runs past l_seq, the sequence has its CIGAR length and every
 * base is 4. */
svth_bam *svth_bam_read_seq(const char *path, int threads, int32_t tid0, int64_t beg0, int32_t tid1, int64_t end1,
                            const svth_inflater *inf, char *err, size_t errcap);
/* Those sequences (valid until svth_bam_free): 1, or 0 for a pileup read without them. */
int svth_bam_insseq(const svth_bam *b, svt_insseq_view *out);
/* svth_bam_read_ex that also keeps the segment table of include/svtrek_junction.h -- what svt_load_junctions
 * takes: one record for every kept read that carries an SA:Z tag (found by walking the aux fields, as the CG
 * restoration does), its own segment from the CIGAR the pileup keeps (the CG-restored one included) and flag
 * 0x10 (rlen 0 for an unmapped record, flag 4, as bam_endpos has it), then one row per entry rname,pos,strand,CIGAR,mapQ,NM; of the value in tag order (pos 1-based in the
 * tag, 0-based in the row).  `read` holds indices of the final pileup, after the stable (tid, pos) sort when
 * the file needed one.  A malformed value -- a missing or empty field, an unknown rname, an empty or invalid
 * CIGAR, pos < 1, a strand other than + / -, an entry without its `;`, a number past 32 bits -- drops that
 * record's row and is counted (svth_bam_n_sa_malformed); it is never an error for the file. */
svth_bam *svth_bam_read_sa(const char *path, int threads, int32_t tid0, int64_t beg0, int32_t tid1, int64_t end1,
                           const svth_inflater *inf, char *err, size_t errcap);
/* That table (valid until svth_bam_free): 1, or 0 for a pileup read without it. */
int svth_bam_junctions(const svth_bam *b, svt_junction_view *out);
int64_t svth_bam_n_sa_malformed(const svth_bam *b);
/* A BAM decoded on the device: the file read in batches of whole BGZF blocks (`threads`
 * parallel preads; buffers from sink->alloc when given, e.g. pinned memory) and handed to
 * sink->feed compressed -- the next batch read by a helper thread meanwhile.  The header is
 * inflated and read on the host: sink->begin gets its reference count first, and the first
 * feed's `skip` is its length in the inflated stream (the CLI's sink is svt_bam_dec_*).
 * stage4 (optional): batch reads, feed calls, waits for the next batch, the whole read (s).
 * Returns 0, or 1 with a message in err. */
typedef struct svth_dev_sink {
    int (*begin)(void *user, int32_t n_targets, char *err, size_t errcap);
    int (*feed)(void *user, const uint8_t *comp, size_t comp_bytes, const svt_bgzf_block *blocks, size_t n,
                uint64_t skip, char *err, size_t errcap);
    void *(*alloc)(void *user, size_t bytes);
    void (*release)(void *user, void *p);
    void *user;
    size_t batch_bytes;   /* compressed bytes per batch (0: 1 GiB) */
} svth_dev_sink;
int svth_bam_read_device(const char *path, int threads, const svth_dev_sink *sink, int32_t *n_targets, double *stage4,
                         char *err, size_t errcap);
void      svth_bam_free(svth_bam *b);
/* View valid until svth_bam_free. */
void      svth_bam_view(const svth_bam *b, svt_pileup_view *out);
int32_t   svth_bam_n_targets(const svth_bam *b);
const char *svth_bam_target_name(const svth_bam *b, int32_t tid);
int64_t   svth_bam_n_records(const svth_bam *b);     /* all records incl. tid < 0     */
int64_t   svth_bam_n_cg_restored(const svth_bam *b); /* CIGARs restored from CG:B,I   */
/* Where a device-inflate read spent its time (s): batch reads, header scans, buffer allocation,
 * inflate calls (all on the helper thread), the parser waiting for batches, and the whole read. */
void      svth_bam_stage_seconds(const svth_bam *b, double *s6);

/* A1: parse one VCF data line in place (as strtok_r does).
 * Returns 1 = record reaches the type switch (*l filled), 0 = skipped silently,
 * 2 = skipped with a stderr message (written into err). */
int svth_parse_line(char *line, svt_locus *l, char *err, size_t errcap);

/* A1 over a whole VCF text (the reader loop of process_vcf, audit.c:295-338: lines shorter
 * than 2 bytes and '#' lines skipped, the trailing '\n' stripped), parsed by `threads`
 * threads over '\n'-aligned pieces.  Records in file order; the stderr messages the
 * reference's workers would print (parse errors, "[ERROR] Unkown type.") in file order. */
typedef struct svth_vcf svth_vcf;
svth_vcf        *svth_vcf_parse(const char *text, size_t len, int threads);
size_t           svth_vcf_count(const svth_vcf *v);
const svt_locus *svth_vcf_loci(const svth_vcf *v);
const char      *svth_vcf_messages(const svth_vcf *v, size_t *len);
void             svth_vcf_free(svth_vcf *v);

/* A11 over a batch: the concatenated stdout text of n records in order, formatted by
 * `threads` threads; malloc'ed (free with svth_free), *len = its length. */
char *svth_format_batch(const svt_locus *l, const svt_result *r, size_t n, int threads, size_t *len);
/* The `--evidence FILE` table (include/svtrek_evidence.h): one tab-separated line per record,
 *   row type chrom pos end ref_pos ref_end sup_pos depth_pos lo_pos hi_pos sup_end depth_end lo_end hi_end
 * row = the record's index (0 .. n-1), type its numeric code, chrom the index stdout prints, ev[2k] /
 * ev[2k + 1] record k's two breakpoints; NA stands for 0xFFFFFFFF in ref_* / lo_* / hi_*.  header != 0:
 * the "#row ..." column line first.  malloc'ed (free with svth_free), *len = its length. */
char *svth_format_evidence(const svt_locus *l, const svt_result *r, const svt_evidence *ev, size_t n, int header,
                           int threads, size_t *len);
/* The calls of `svtrek call` (include/svtrek_call.h) as VCF 4.2 text: with header != 0 the ##fileformat,
 * ##source=svtrek_amd call, one ##contig=<ID=name> per names[0 .. n_names), the ##ALT / ##INFO lines and the
 * #CHROM line; then per call
 *   name  pos  svtrek.<TYPE>.<k>  N  <DEL>|<INS>  .  PASS
 *   SVTYPE=T;END=e;SVLEN=[-]len;SUPPORT=c;DEPTH=d;XRANGE=x_lo,x_hi;LENRANGE=len_lo,len_hi
 * name = names[chrom - 1] (the number itself when there is none), k the call's rank among those of its
 * type (from 1).  SVTYPE and END come first and no key contains "END=" before them: svth_parse_line takes
 * the first it finds.  malloc'ed (free with svth_free), *len = its length. */
char *svth_format_calls(const svt_call *calls, size_t n, const char *const *names, size_t n_names, int header,
                        int threads, size_t *len);
/* The same with genotypes (include/svtrek_genotype.h), gts[k] call k's record: the header gains the ##FORMAT
 * lines of GT, GQ, DR, DV and PL and its column line "\tFORMAT\t<sample>" (sample NULL or "": SAMPLE); every
 * record gains
 *   GT:GQ:DR:DV:PL   0/0|0/1|1/1:gq:ref:alt:pl0,pl1,pl2        (a no call: ./.:0:0:0:0,0,0)
 * INFO is unchanged and svth_parse_line reads the first 8 fields, so `svtrek audt` takes the file as it
 * takes the sites-only one.  gts == NULL: svth_format_calls, byte for byte. */
char *svth_format_calls_gt(const svt_call *calls, const svt_gt *gts, size_t n, const char *const *names, size_t n_names,
                           const char *sample, int header, int threads, size_t *len);
/* The same with the consensus inserted sequences (include/svtrek_callseq.h), cons[k] / bases[k * cap ..] call
 * k's svt_call_consensus record: the header gains the ##INFO lines of CONSLEN and CONSREADS; an INS call with
 * 1 <= len <= cap is written as REF N, ALT N followed by the consensus as ACGTN, every other INS call keeps
 * N <INS>; every INS call's INFO ends in ";CONSLEN=<len, or 0 when there is none>;CONSREADS=<n_used>" (SVTYPE
 * and END stay first).  DEL records are unchanged.  cons == NULL: svth_format_calls_gt, byte for byte. */
char *svth_format_calls_seq(const svt_call *calls, const svt_gt *gts, const svt_poa_result *cons, const uint8_t *bases,
                            int32_t cap, size_t n, const char *const *names, size_t n_names, const char *sample, int header,
                            int threads, size_t *len);
/* The same for a scan that asked for rearrangements (include/svtrek_rearr.h), rearr = the scan's svt_call_params.rearr:
 * a call of type SVT_DUP / SVT_INV is written as
 *   name  pos  svtrek.DUP.<k>|svtrek.INV.<k>  N  <DUP>|<INV>  .  PASS  SVTYPE=DUP|INV;END=e;SVLEN=len;...
 * with k its rank among the calls of its own type, SVLEN positive, the INFO keys those of a DEL record and the
 * genotype column, if any, its svt_gt record (the invalid one prints ./.); the header gains
 * ##ALT=<ID=DUP,...> / ##ALT=<ID=INV,...> behind the INS line for the bits set in rearr.  rearr == 0:
 * svth_format_calls_seq, byte for byte (every type but DEL is written as INS there, as before). */
char *svth_format_calls_rearr(const svt_call *calls, const svt_gt *gts, const svt_poa_result *cons, const uint8_t *bases,
                              int32_t cap, size_t n, const char *const *names, size_t n_names, const char *sample, int header,
                              int threads, uint32_t rearr, size_t *len);
/* The same for a scan that asked for breakends too (include/svtrek_bnd.h), bnd = the scan's svt_call_params.bnd: a call
 * of type SVT_BND is written as ONE record,
 *   name  pos  svtrek.BND.<k>  N  ALT  .  PASS  SVTYPE=BND;CHR2=mate;POS2=end;SUPPORT=c;DEPTH=d;XRANGE=lo,hi;X2RANGE=lo,hi
 * with ALT by o = SVT_CALL_MATE_ORIENT: 0 N]mate:end], 1 N[mate:end[, 2 ]mate:end]N, 3 [mate:end[N (s_lo = 0 puts the base
 * first, s_hi = 1 uses '['), mate named by the rule of CHROM, positions printed as the record holds them, k its rank among
 * the BND calls, X2RANGE = len_lo, len_hi, and ./. in the genotype column, if any.  There is no END key.  The header gains the
 * ##INFO lines of CHR2, POS2 and X2RANGE behind LENRANGE and no ##ALT line.  bnd == 0: svth_format_calls_rearr, byte for
 * byte, which forwards here. */
char *svth_format_calls_bnd(const svt_call *calls, const svt_gt *gts, const svt_poa_result *cons, const uint8_t *bases,
                            int32_t cap, size_t n, const char *const *names, size_t n_names, const char *sample, int header,
                            int threads, uint32_t rearr, uint32_t bnd, size_t *len);
void  svth_free(void *p);

/* A11: stdout text for one refined record; returns bytes written (0 = prints nothing:
 * DUP/TRA/BND/unknown -> "[ERROR] Unkown type." on stderr, or DEL/INV of exactly 50 bp). */
int svth_format(const svt_locus *l, const svt_result *r, char *buf, size_t cap);
/* 1 when the record's type has no refinement (the reference prints
 * "[ERROR] Unkown type.\n" to stderr for it, audit.c:233-235). */
int svth_is_unknown_type(const svt_locus *l);

#ifdef __cplusplus
}
#endif
#endif
