// svt_junction.inc -- DEL / INS items from split alignments (include/svtrek_junction.h,
// svt_call_params.junctions = 1; included by svt_engine.hip after svt_callmerge.inc; BkFile, bk_file,
// bk_stat_add, JN_MARK and jn_limits are svt_callindex.inc's, jn_next and jn_classify -- the header's
// rules -- svt_jnclass.h's, the host side is svt_junction_host.inc).
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
constexpr int JN_NSTAT = 5;           // junctions, DEL items, INS items, other, skipped
static_assert(sizeof(svt_junction_seg) == 24, "include/svtrek_junction.h");

struct JunctionArgs {
    const uint64_t *off;          // [n + 1] the table's rows per record
    const svt_junction_seg *seg;
    uint64_t n;                   // table records
    const uint32_t *boff;         // the base view's off[BA_N][nbk + 1]
    BkFile f;                     // the union's: off COUNT the junction counts; stat: [BK_SLOTS][JN_NSTAT]
};

template <bool COUNT>
__global__ __launch_bounds__(64 * WPB) void junction_kernel(JunctionArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * (64 * WPB) + threadIdx.x;
    uint32_t st[JN_NSTAT] = {0u, 0u, 0u, 0u, 0u};
    if (k < a.n) {
        svt_junction_seg A, B;
        if (jn_next(a.off, a.seg, k, A, B)) {
            const JnItem it = jn_classify<1u << JN_DEL | 1u << JN_INS>(A, B, jn_limits());
            st[0] = 1u;
            st[3] = it.other ? 1u : 0u;
            if (it.kind != JN_NONE) {
                const bool T = it.kind == JN_INS;   // row S: DEL, row I: INS
                st[1 + T] = 1u;
                st[4] = it.past ? 1u : 0u;
                const uint32_t nbt = a.f.cnb[it.tid];   // (>= 1: the record itself is a read of the contig)
                const uint64_t row = (uint64_t)(T ? BA_I : BA_S) * (a.f.nbk + 1), g = a.f.cbase[it.tid] + min(it.x >> BKS, nbt - 1u);
                bk_file<COUNT>(a.f, T, g, COUNT ? 0u : a.boff[row + g + 1] - a.boff[row + g],   // (behind the bucket's base events)
                               make_uint4(it.x, it.len << 4 | (T ? OP_INS : OP_DEL), it.hi, it.lo | JN_MARK));
            }
        }
    }
    if (COUNT) {
        if (ballot(st[0] != 0u) != 0ull)   // (wave-uniform)
            bk_stat_add(a.f, st);
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
