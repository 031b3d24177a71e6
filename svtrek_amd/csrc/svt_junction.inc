// svt_junction.inc -- DEL / INS items from split alignments (include/svtrek_junction.h,
// svt_call_params.junctions = 1; included by svt_engine.hip after svt_callmerge.inc, the host side is
// svt_junction_host.inc).
//
// The junction items go into a THIRD index in the value buckets' shape: the UNION of the base view's
// events (the plain buckets' rows S and I, or the merged index's) and the junction events, bucket by
// bucket -- bucket g of the union holds the base view's events of g followed by the junction events of
// g, S's events before I's, the off[BA_N][nbk + 1] table with rows S and I filled -- so that
// call_sort_kernel .. call_emit_kernel and the split kernels run on it unchanged.  A junction event is
// {x, len << 4 | OP_DEL / OP_INS, extent end, extent begin | JN_MARK}: the scan's kernels read x and the
// op word alone, and only genotype_kernel's junction instantiation (svt_genotype.inc) looks at the mark,
// bit 31 of the word in which a CIGAR event keeps its read's pos (< 2^31).
//
//   junction_kernel<true>    one lane per table record: B by one pass over the record's rows, the
//                            junction classified, the item's bucket counted per (array, bucket)
//   junction_extent_kernel   the base view's extents added to those counts
//   (one hipcub exclusive sum per row)
//   junction_copy_kernel     the base events to their places, one wave per 64 buckets of a row
//   junction_kernel<false>   the same walk again: every item through its bucket's atomic cursor to a
//                            slot behind the bucket's base events
// The order of the junction events inside a bucket is whatever the atomics give; nothing downstream
// reads it.  A junction x lies in its bucket's 1 kb, a contig's last bucket takes everything past the
// others: the counting sort of a big bucket relies on both.  Integer only, no LDS, no inline assembly.
constexpr uint32_t JN_SLOTS = 1024;   // the stats are added into JN_SLOTS x JN_NSTAT counters by wave number
constexpr int JN_NSTAT = 5;           // junctions, DEL items, INS items, other, skipped
constexpr uint32_t JN_MARK = 0x80000000u, JN_EXT_MAX = 0x7fffffffu;
static_assert(sizeof(svt_junction_seg) == 24, "include/svtrek_junction.h");

struct JunctionArgs {
    const uint64_t *off;          // [n + 1] the table's rows per record
    const svt_junction_seg *seg;
    uint64_t n;                   // table records
    const uint64_t *cbase;        // the main index's
    const uint32_t *cnb;
    uint64_t nbk;
    const uint32_t *boff;         // the base view's off[BA_N][nbk + 1]
    uint32_t *uoff;               // the union's: COUNT the junction counts of rows S and I, else the extents
    uint32_t *cur;                // [2][nbk + 1] cursors of the filing pass (zeroed)
    uint4 *ev;                    // the union's events
    uint32_t n_ev;
    unsigned long long *stat;     // [JN_SLOTS][JN_NSTAT] (COUNT)
    uint32_t *err;                // set when a slot falls outside its bucket's extent
};

// a < b in the order of the tuple (q_beg, q_end, tid, r_beg, strand)
__device__ __forceinline__ bool jn_less(const svt_junction_seg &a, const svt_junction_seg &b) {
    if (a.q_beg != b.q_beg) return a.q_beg < b.q_beg;
    if (a.q_end != b.q_end) return a.q_end < b.q_end;
    if (a.tid != b.tid) return a.tid < b.tid;
    if (a.r_beg != b.r_beg) return a.r_beg < b.r_beg;
    return a.strand < b.strand;
}

template <bool COUNT>
__global__ __launch_bounds__(64 * WPB) void junction_kernel(JunctionArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * (64 * WPB) + threadIdx.x;
    uint32_t st[JN_NSTAT] = {0u, 0u, 0u, 0u, 0u};
    if (k < a.n) {
        const uint64_t r0 = a.off[k], r1 = a.off[k + 1];
        const svt_junction_seg A = a.seg[r0];
        svt_junction_seg B = A;
        bool have = false;
        for (uint64_t r = r0 + 1; r < r1; r++) {   // the smallest tuple strictly greater than A's
            const svt_junction_seg t = a.seg[r];
            if (jn_less(A, t) && (!have || jn_less(t, B))) {
                B = t;
                have = true;
            }
        }
        if (have) {
            st[0] = 1u;
            int T = -1;   // 0 DEL, 1 INS
            uint32_t x = 0, len = 0, lo = 0, hi = 0;
            if (B.tid != A.tid || B.strand != A.strand) {
                st[3] = 1u;
            } else {
                const svt_junction_seg &Lf = A.strand ? B : A, &Rt = A.strand ? A : B;
                const int64_t dr = (int64_t)Rt.r_beg - (int64_t)Lf.r_end, dq = (int64_t)B.q_beg - (int64_t)A.q_end, d = dr - dq;
                if (d > (int64_t)SV_MIN_LENGTH && dr > 0) T = 0;
                else if (-d >= (int64_t)SV_MIN_LENGTH && dq > 0) {
                    if (dr >= -(int64_t)SV_MIN_LENGTH) T = 1;
                    else st[3] = 1u;
                }
                if (T >= 0) {
                    x = min(Lf.r_end, IX_SAT);
                    len = (uint32_t)min(T ? -d : d, (int64_t)CM_LEN_MAX);
                    lo = min(min(Lf.r_beg, Rt.r_beg), JN_EXT_MAX);
                    hi = min(max(Lf.r_end, Rt.r_end), JN_EXT_MAX);
                }
            }
            if (T >= 0) {
                st[1 + T] = 1u;
                st[4] = x >= IX_SAT ? 1u : 0u;
                const uint32_t nbt = a.cnb[A.tid];   // (>= 1: the record itself is a read of the contig)
                const uint64_t row = (uint64_t)(T ? BA_I : BA_S) * (a.nbk + 1), g = a.cbase[A.tid] + min(x >> BKS, nbt - 1u);
                if (COUNT) {
                    atomicAdd(&a.uoff[row + g], 1u);
                } else {
                    const uint32_t o0 = a.uoff[row + g] + (a.boff[row + g + 1] - a.boff[row + g]), o1 = a.uoff[row + g + 1];
                    const uint32_t sl = atomicAdd(&a.cur[(uint64_t)T * (a.nbk + 1) + g], 1u);
                    if (o0 > o1 || sl >= o1 - o0 || o0 + sl >= a.n_ev) *a.err = 1u;
                    else a.ev[o0 + sl] = make_uint4(x, len << 4 | (T ? OP_INS : OP_DEL), hi, lo | JN_MARK);
                }
            }
        }
    }
    if (COUNT) {
        const bool any = ballot(st[0] != 0u) != 0ull;   // (wave-uniform)
        if (any) {
#pragma unroll
            for (int d = 32; d > 0; d >>= 1)
#pragma unroll
                for (int q = 0; q < JN_NSTAT; q++) st[q] += (uint32_t)__shfl_xor((int)st[q], d, WAVE);
            if (lane_id() == 0) {
                const uint64_t wv = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
                unsigned long long *q = a.stat + (uint64_t)JN_NSTAT * (uint32_t)(wv & (JN_SLOTS - 1u));
#pragma unroll
                for (int j = 0; j < JN_NSTAT; j++)
                    if (st[j]) atomicAdd(&q[j], (unsigned long long)st[j]);
            }
        }
    }
}

// uoff[row][g] (the junction counts) += the base view's events of bucket g, rows S and I.
__global__ __launch_bounds__(256) void junction_extent_kernel(const uint32_t *boff, uint32_t *uoff, uint64_t nbk) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= 2 * nbk) return;
    const uint64_t row = (uint64_t)(j >= nbk ? BA_I : BA_S) * (nbk + 1), g = j >= nbk ? j - nbk : j;
    uoff[row + g] += boff[row + g + 1] - boff[row + g];
}

// The base events to the union: one wave per 64 consecutive buckets of a row.  Their events are
// contiguous in the base view and nearly so in the union (the junction events of each bucket lie
// between), so both sides of the copy are coalesced 16-B accesses.  A lane holds its bucket's first
// base event and the distance to its place in the union; an event finds its bucket among the 64 by a
// binary search over the lanes (six shuffles) -- the last bucket starting at or before it.
__global__ __launch_bounds__(64 * WPB) void junction_copy_kernel(const uint4 *bev, const uint32_t *boff, const uint32_t *uoff,
                                                                 uint64_t nbk, uint4 *uev, uint32_t n_ev, uint32_t *err) {
    const uint64_t wv = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6), per = (nbk + WAVE - 1) / WAVE;
    if (wv >= 2 * per) return;
    const bool arr_i = wv >= per;
    const uint64_t row = (uint64_t)(arr_i ? BA_I : BA_S) * (nbk + 1), g0 = (wv - (arr_i ? per : 0)) * WAVE;
    const int ln = lane_id();
    const uint64_t g = g0 + (uint64_t)ln;
    const uint32_t first = g < nbk ? boff[row + g] : 0xffffffffu;
    const uint32_t delta = g < nbk ? uoff[row + g] - first : 0u;
    const uint32_t E0 = rdlane(first, 0), E1 = boff[row + min(g0 + WAVE, nbk)];
    for (uint32_t e0 = E0; e0 < E1; e0 += WAVE) {
        const uint32_t e = e0 + (uint32_t)ln;
        int b = 0;
#pragma unroll
        for (int step = WAVE / 2; step > 0; step >>= 1) {
            const uint32_t v = (uint32_t)__shfl((int)first, b + step, WAVE);
            b += v <= e ? step : 0;
        }
        const uint32_t dst = e + (uint32_t)__shfl((int)delta, b, WAVE);
        if (e < E1) {
            if (dst >= n_ev) *err = 1u;
            else uev[dst] = bev[e];
        }
    }
}
