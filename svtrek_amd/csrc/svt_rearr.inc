// svt_rearr.inc -- DUP / INV items from split alignments (include/svtrek_rearr.h, svt_call_params.rearr;
// included by svt_engine.hip after svt_junction.inc, whose JN_MARK it shares; BkFile, bk_file, bk_stat_add,
// jn_less and jn_next are svt_callindex.inc's, the host side is svt_rearr_host.inc).
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
//   rearr_emit_kernel      call_emit_kernel with the types SVT_DUP / SVT_INV and end = the rounded mean
//                          of x + len for both rows
//   rearr_merge_kernel     the scan's two sorted lists -- the DEL / INS calls and the INV / DUP calls,
//                          each in (chrom, pos, type[, len]) order -- into one: a binary search per call
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
        if (jn_next(a.off, a.seg, k, A, B) && B.tid == A.tid) {
            int T = -1;   // 0 DUP, 1 INV
            int64_t x64 = 0, len64 = 0;
            uint32_t lo = 0, hi = 0;
            if (B.strand != A.strand) {
                const int64_t p = A.strand ? (int64_t)A.r_beg : (int64_t)A.r_end;
                const int64_t q = B.strand ? (int64_t)B.r_end : (int64_t)B.r_beg;
                const int64_t w = p > q ? p - q : q - p;
                if (w > (int64_t)SV_MIN_LENGTH) {
                    T = 1;
                    x64 = min(p, q);
                    len64 = w;
                }
            } else {
                const svt_junction_seg &Lf = A.strand ? B : A, &Rt = A.strand ? A : B;
                const int64_t dr = (int64_t)Rt.r_beg - (int64_t)Lf.r_end, dq = (int64_t)B.q_beg - (int64_t)A.q_end, d = dr - dq;
                if (dr < -(int64_t)SV_MIN_LENGTH && -d >= (int64_t)SV_MIN_LENGTH) {
                    T = 0;
                    x64 = (int64_t)Rt.r_beg;
                    len64 = -dr;
                }
            }
            if (T >= 0) {
                const uint32_t x = (uint32_t)min(x64, (int64_t)IX_SAT), len = (uint32_t)min(len64, (int64_t)CM_LEN_MAX);
                lo = min(min(A.r_beg, B.r_beg), JN_EXT_MAX);
                hi = min(max(A.r_end, B.r_end), JN_EXT_MAX);
                st[T] = 1u;
                const uint32_t nbt = a.f.cnb[A.tid];   // (>= 1: the record itself is a read of the contig)
                bk_file<COUNT>(a.f, T, a.f.cbase[A.tid] + min(x >> BKS, nbt - 1u), 0u,
                               make_uint4(x, len << 4 | (T ? OP_INS : OP_DEL), hi, lo | JN_MARK));
            }
        }
    }
    if (COUNT) {
        if (ballot((st[0] | st[1]) != 0u) != 0ull)   // (wave-uniform)
            bk_stat_add(a.f, st);
    }
}

// call_emit_kernel for the rearrangement index: one wave per call, row S's clusters are DUP calls, row
// I's INV calls, and both end at the rounded mean of x + len.
__global__ __launch_bounds__(64 * WPB) void rearr_emit_kernel(CallArgs a, uint32_t n_calls, svt_call *out) {
    const uint32_t g = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (g >= n_calls) return;
    const CallAcc q = a.acc[(uint32_t)uniform_i((int32_t)a.pick[g])];
    const unsigned long long c = q.cnt, h = c / 2;
    const int inv = q.seg >= (uint32_t)a.nt ? 1 : 0, tid = (int)(q.seg - (inv ? (uint32_t)a.nt : 0u));
    const uint32_t pos = (uint32_t)uniform_i((int32_t)(uint32_t)((q.sx + h) / c));
    const uint32_t len = (uint32_t)((q.slen + h) / c);
    const uint32_t end = (uint32_t)((q.sx + q.slen + h) / c);
    const uint32_t depth = ev_depth(a.pile, tid, pos);
    const uint32_t w[12] = {(uint32_t)(inv ? SVT_INV : SVT_DUP), (uint32_t)(tid + 1), pos, end, q.cnt, depth, len,
                            ~q.nlen_lo, q.len_hi, ~q.nx_lo, q.x_hi, 0u};
    const int ln = lane_id();
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) word = ln == i ? w[i] : word;
    if (ln < 12) reinterpret_cast<uint32_t *>(out + g)[ln] = word;
}

// The two lists of a scan with rearr != 0: la[0 .. na) the DEL / INS calls, lb[0 .. nb) the INV / DUP
// calls, each in (chrom, pos, type code[, len]) order.  Every type code of la is below every one of lb,
// so the merged order is decided by (chrom, pos) alone: a call of la goes behind the calls of lb
// strictly before it, a call of lb behind the calls of la at or before it.  One thread per call.
__global__ __launch_bounds__(256) void rearr_merge_kernel(const svt_call *la, uint32_t na, const svt_call *lb, uint32_t nb, svt_call *out) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= na + nb) return;
    const bool first = g < na;
    const svt_call *mine = first ? la + g : lb + (g - na), *other = first ? lb : la;
    auto key = [](const svt_call &c) { return (unsigned long long)(uint32_t)c.chrom << 32 | c.pos; };
    const unsigned long long k = key(*mine);
    uint32_t lo = 0, hi = first ? nb : na;
    while (lo < hi) {
        const uint32_t m = lo + (hi - lo) / 2;
        const unsigned long long o = key(other[m]);
        if (first ? o < k : o <= k) lo = m + 1;
        else hi = m;
    }
    const uint32_t rank = (first ? g : g - na) + lo;
    const uint4 *src = reinterpret_cast<const uint4 *>(mine);
    uint4 *dst = reinterpret_cast<uint4 *>(out + rank);
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
}
