// svt_rearr.inc -- DUP / INV items from split alignments (include/svtrek_rearr.h, svt_call_params.rearr;
// included by svt_engine.hip after svt_junction.inc; BkFile, bk_file, bk_stat_add, JN_MARK and jn_limits are
// svt_callindex.inc's, jn_next and jn_classify -- the header's rules -- svt_jnclass.h's, the host side is
// svt_rearr_host.inc).
//
// The items go into a FOURTH index in the value buckets' shape, of the rearrangement events alone: row S
// holds the DUP events, row I the INV events, the off[BA_N][nbk + 1] table with rows S and I filled, an
// event is {x, len << 4 | OP_DEL (DUP) / OP_INS (INV), extent end, extent begin | JN_MARK}.  With that
// call_sort_kernel .. call_pick_kernel and the split kernels run on it unchanged, asked for the rows'
// types through CallArgs.types (row S's bit is SVT_DEL's, row I's SVT_INS's); only the records differ:
//
//   rearr_kernel<true>     one lane per table record: B by one pass over the record's rows, the
//                          junction classified, the item's bucket counted per (row, bucket)
//   (one hipcub exclusive sum per row)
//   rearr_kernel<false>    the same walk again: every item through its bucket's atomic cursor
//   call_emit_kernel<true> (svt_call.inc) the types SVT_DUP / SVT_INV and end = the rounded mean of
//                          x + len for both rows
//   merge_lists_kernel     (svt_call.inc) the scan's two sorted lists -- the DEL / INS calls and the INV /
//                          DUP calls, each in (chrom, pos, type[, len]) order -- into one
// The order of the events inside a bucket is whatever the atomics give; nothing downstream reads it.  An
// item's x is at most its own segment's end (svtrek_rearr.h), so it lies in its bucket's 1 kb and never
// in a contig's last bucket.  Integer only, no LDS, no inline assembly.
constexpr int RR_NSTAT = 2;           // DUP items, INV items

struct RearrArgs {
    const uint64_t *off;          // [n + 1] the table's rows per record
    const svt_junction_seg *seg;
    uint64_t n;                   // table records
    BkFile f;                     // stat: [BK_SLOTS][RR_NSTAT]
};

template <bool COUNT>
__global__ __launch_bounds__(64 * WPB) void rearr_kernel(RearrArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * (64 * WPB) + threadIdx.x;
    uint32_t st[RR_NSTAT] = {0u, 0u};
    if (k < a.n) {
        svt_junction_seg A, B;
        if (jn_next(a.off, a.seg, k, A, B)) {
            const JnItem it = jn_classify<1u << JN_DUP | 1u << JN_INV>(A, B, jn_limits());
            if (it.kind != JN_NONE) {
                const bool T = it.kind == JN_INV;   // row S: DUP, row I: INV
                st[T] = 1u;
                const uint32_t nbt = a.f.cnb[it.tid];   // (>= 1: the record itself is a read of the contig)
                bk_file<COUNT>(a.f, T, a.f.cbase[it.tid] + min(it.x >> BKS, nbt - 1u), 0u,
                               make_uint4(it.x, it.len << 4 | (T ? OP_INS : OP_DEL), it.hi, it.lo | JN_MARK));
            }
        }
    }
    if (COUNT) {
        if (ballot((st[0] | st[1]) != 0u) != 0ull)   // (wave-uniform)
            bk_stat_add(a.f, st);
    }
}
