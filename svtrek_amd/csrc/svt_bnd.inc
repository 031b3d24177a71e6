// svt_bnd.inc -- translocation breakends from split alignments (include/svtrek_bnd.h, svt_call_params.bnd;
// included by svt_engine.hip after svt_rearr.inc; svt_call.inc's merge_lists_kernel puts the BND calls behind
// the scan's other calls, call_store and call_copy are its too; jn_next and jn_classify -- the header's rule --
// are svt_jnclass.h's, jn_limits svt_callindex.inc's, ev_depth svt_evidence.inc's, the host side is
// svt_bnd_host.inc).
//
// No buckets: a breakend's x may be an SA row's coordinate on a contig without a single read, so the items
// are ONE LIST, in (class, x) order, of two 64-bit words an item -- cls = tid_lo << 33 | tid_hi << 2 | o and
// xy = x << 32 | y -- ordered by hipcub's stable radix sort.
//
//   build (once per pileup and table)
//     bnd_kernel         one lane per table record: B by jn_next, the item classified in signed 64 bits and
//                        appended in ONE pass -- a record gives at most one item, so n slots bound the list;
//                        one atomic per wave reserves the slots (ballot + popcount + lane rank)
//     (radix sort on x, then on the class word's bits in use)
//     bnd_head_kernel<0> with link = 2^30: a mark where the class changes; their sum is stats.classes
//   scan (link and min_support vary)
//     bnd_head_kernel<0> a mark where the class changes or x - prev > link; an inclusive sum numbers the
//                        start clusters
//     bnd_key_kernel     cluster << 30 | y beside x, and every cluster's class word
//     (radix sort on that key: every cluster by y)
//     bnd_head_kernel<1> a mark where the cluster changes or y - prev > link; an inclusive sum numbers the
//                        groups
//     bnd_accum_kernel   every item into its group's record with integer atomics (exact in any order)
//     bnd_pick_kernel    + one select: the groups of c >= min_support
//     bnd_emit_kernel    one wave per call: the rounded means, ev_depth, the 48-B record in 12 lanes' stores
//                        and the call's low order key
//     (radix sort of the call indices on the low key, bnd_hikey_kernel, radix sort on the high key)
//     bnd_gather_kernel  the records in (chrom, pos, mate chrom, o, end) order
// The order of items with equal keys is whatever the atomics and the sort's input give; nothing downstream
// reads it.  Integer only, no LDS, vector stores, no inline assembly.
constexpr uint32_t BND_SAT = 1u << 30;     // x, y at or past it: skipped
constexpr int BND_XBITS = 30;

struct BndBuild {
    const uint64_t *off;          // [n + 1] the table's rows per record
    const svt_junction_seg *seg;
    uint64_t n;                   // table records
    unsigned long long *cls, *xy; // [n] the items as appended
    uint32_t *ctr;                // [0] kept items (the append cursor), [1] skipped items
};

__global__ __launch_bounds__(64 * WPB) void bnd_kernel(BndBuild a) {
    const uint64_t k = (uint64_t)blockIdx.x * (64 * WPB) + threadIdx.x;
    bool keep = false, skip = false;
    unsigned long long cls = 0, xy = 0;
    if (k < a.n) {
        svt_junction_seg A, B;
        if (jn_next(a.off, a.seg, k, A, B)) {
            const JnItem it = jn_classify<1u << JN_BND>(A, B, jn_limits());
            skip = it.kind == JN_BND && it.past;
            keep = it.kind == JN_BND && !it.past;
            cls = (uint64_t)(uint32_t)it.tid << 33 | (uint64_t)(uint32_t)it.tid_hi << 2 | it.o;
            xy = (unsigned long long)it.x << 32 | it.y;
        }
    }
    const uint64_t mk = ballot(keep), ms = ballot(skip);   // (wave-uniform)
    const int ln = lane_id();
    if (mk) {
        uint32_t base = 0;
        if (ln == 0) base = atomicAdd(&a.ctr[0], (uint32_t)__popcll(mk));
        base = (uint32_t)uniform_i((int32_t)base);
        const uint32_t slot = base + (uint32_t)__popcll(mk & ((1ull << ln) - 1ull));
        if (keep && (uint64_t)slot < a.n) {   // (at most one item a record)
            a.cls[slot] = cls;
            a.xy[slot] = xy;
        }
    }
    if (ms && ln == 0) atomicAdd(&a.ctr[1], (uint32_t)__popcll(ms));
}

// The head marks of a list of n items ordered by (group word, value).  KIND 0: the item list, group word
// cls[i], value x = xy[i] >> 32.  KIND 1: the keys cluster << 30 | y, group word key >> 30, value the low
// 30 bits.  head[i] = 1 iff i == 0, the group word changes or value - previous value > link.
template <int KIND>
__global__ __launch_bounds__(256) void bnd_head_kernel(const unsigned long long *g, const unsigned long long *v, uint32_t n,
                                                       uint32_t link, uint32_t *head) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    bool h = i == 0;
    if (!h) {
        const unsigned long long g1 = KIND ? v[i] >> 30 : g[i], g0 = KIND ? v[i - 1] >> 30 : g[i - 1];
        const uint32_t v1 = KIND ? (uint32_t)v[i] & (BND_SAT - 1u) : (uint32_t)(v[i] >> 32);
        const uint32_t v0 = KIND ? (uint32_t)v[i - 1] & (BND_SAT - 1u) : (uint32_t)(v[i - 1] >> 32);
        h = g1 != g0 || v1 - v0 > link;   // (ascending inside a group word: no wrap)
    }
    head[i] = h ? 1u : 0u;
}

// Item i of the (class, x) list in start cluster cid[i] (1-based): its key for the sort by y, its x beside
// it, and the cluster's class word from the cluster's first item.
__global__ __launch_bounds__(256) void bnd_key_kernel(const unsigned long long *cls, const unsigned long long *xy, const uint32_t *cid,
                                                      uint32_t n, unsigned long long *key, uint32_t *x, unsigned long long *ccls) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t cl = cid[i] - 1u;
    const unsigned long long w = xy[i];
    key[i] = (unsigned long long)cl << 30 | (w & (BND_SAT - 1u));
    x[i] = (uint32_t)(w >> 32);
    if (i == 0 || cid[i - 1] != cid[i]) ccls[cl] = cls[i];
}

struct BndAcc {   // 48 B, zeroed before every scan (the two minima are kept as maxima of ~v)
    unsigned long long sx, sy, cls;
    uint32_t cnt, nx_lo, x_hi, ny_lo, y_hi, pad;
};

// Item i of the list ordered by (cluster, y), in group gid[i] (1-based).
__global__ __launch_bounds__(256) void bnd_accum_kernel(const unsigned long long *key, const uint32_t *x, const uint32_t *gid,
                                                        const unsigned long long *ccls, uint32_t n, BndAcc *acc) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned long long kw = key[i];
    const uint32_t y = (uint32_t)kw & (BND_SAT - 1u), xv = x[i], g = gid[i] - 1u;
    BndAcc *q = acc + g;
    atomicAdd(&q->sx, (unsigned long long)xv);
    atomicAdd(&q->sy, (unsigned long long)y);
    atomicAdd(&q->cnt, 1u);
    atomicMax(&q->nx_lo, ~xv);
    atomicMax(&q->x_hi, xv);
    atomicMax(&q->ny_lo, ~y);
    atomicMax(&q->y_hi, y);
    if (i == 0 || gid[i - 1] != gid[i]) q->cls = ccls[kw >> 30];   // (one writer a group)
}

__global__ __launch_bounds__(256) void bnd_pick_kernel(const BndAcc *acc, uint32_t n_groups, uint32_t min_support, uint8_t *flag) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < n_groups) flag[g] = acc[g].cnt >= min_support ? 1 : 0;
}

// One wave per call, call_emit_kernel's shape: the record of group pick[g], and the call's low order key
// mate chrom << 32 | o << 30 | end.  ev_depth is 0 for a contig without a pileup record (read_range
// returns before it reads a bucket of such a contig).
__global__ __launch_bounds__(64 * WPB) void bnd_emit_kernel(DevPileup pile, const BndAcc *acc, const uint32_t *pick, uint32_t n_calls,
                                                            svt_call *out, unsigned long long *klo, uint32_t *idx) {
    const uint32_t g = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (g >= n_calls) return;
    const BndAcc q = acc[(uint32_t)uniform_i((int32_t)pick[g])];
    const unsigned long long c = q.cnt, h = c / 2;
    const int tid = (int)(q.cls >> 33);
    const uint32_t mate = ((uint32_t)(q.cls >> 2) & 0x7fffffffu) + 1u, o = (uint32_t)q.cls & 3u;
    const uint32_t pos = (uint32_t)uniform_i((int32_t)(uint32_t)((q.sx + h) / c));
    const uint32_t end = (uint32_t)((q.sy + h) / c);
    const uint32_t depth = ev_depth(pile, tid, pos);
    const uint32_t w[12] = {(uint32_t)SVT_BND, (uint32_t)(tid + 1), pos, end, q.cnt, depth, 0u, ~q.ny_lo, q.y_hi, ~q.nx_lo, q.x_hi,
                            mate << 2 | o};
    call_store(out + g, w);
    if (lane_id() == 0) {
        klo[g] = (unsigned long long)mate << 32 | (unsigned long long)o << 30 | end;
        idx[g] = g;
    }
}

// The high order key chrom << 32 | pos of the calls in the order idx gives.
__global__ __launch_bounds__(256) void bnd_hikey_kernel(const svt_call *raw, const uint32_t *idx, uint32_t n, unsigned long long *khi) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const svt_call *c = raw + idx[j];
    khi[j] = (unsigned long long)(uint32_t)c->chrom << 32 | c->pos;
}

__global__ __launch_bounds__(256) void bnd_gather_kernel(const svt_call *raw, const uint32_t *idx, uint32_t n, svt_call *out) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < n) call_copy(out + j, raw + idx[j]);
}
